#!/bin/bash
# Collect the judged measurements on the GPU box: bench lines, rocprofv3 kernel stats and the HBM
# PMC passes (FETCH_SIZE and WRITE_SIZE in separate runs, no other trace domain).
#   gpurun -- 'bash tools/profile_round.sh <tag> [config]'
# Outputs go to $OUT_DIR/<tag>_* (default profile_out/); copy the summaries you keep into profiles/.
TAG=${1:-round}
CFG=${2:-c3}
R=$PWD
O=${OUT_DIR:-$R/profile_out}
mkdir -p $O
python3 $R/bench.py --full --config $CFG > $O/${TAG}_${CFG}_bench.json 2> $O/${TAG}_${CFG}_bench.err
cat $O/${TAG}_${CFG}_bench.json
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $O/${TAG}_${CFG}_kt -- python3 $R/bench.py --full --config $CFG --steps 5 --warmup 2 --no-cpu-baseline --no-cold > $O/${TAG}_${CFG}_kt.log 2>&1
DB=$(find $O/${TAG}_${CFG}_kt -name "*.db" | head -1)
python3 $R/tools/rocprof_summary.py $DB $O/${TAG}_${CFG}_kernel_stats.txt > /dev/null
for C in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $C -d $O/${TAG}_${CFG}_pmc_$C --output-format csv -- python3 $R/bench.py --full --config $CFG --steps 2 --warmup 1 --no-cpu-baseline --no-cold > $O/${TAG}_${CFG}_pmc_$C.log 2>&1
done
python3 $R/tools/pmc_summary.py $O/${TAG}_${CFG}_hbm_pmc.txt $O/${TAG}_${CFG}_hbm_pmc.json $O/${TAG}_${CFG}_pmc_FETCH_SIZE $O/${TAG}_${CFG}_pmc_WRITE_SIZE > /dev/null
# SQ counters of the same command (one pass, 8 SQ slots): VALU instructions per wave and issue / wait cycles
rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_BUSY_CYCLES -d $O/${TAG}_${CFG}_pmc_SQ --output-format csv -- python3 $R/bench.py --full --config $CFG --steps 2 --warmup 1 --no-cpu-baseline --no-cold > $O/${TAG}_${CFG}_pmc_SQ.log 2>&1
python3 $R/tools/pmc_summary.py $O/${TAG}_${CFG}_sq_pmc.txt $O/${TAG}_${CFG}_sq_pmc.json $O/${TAG}_${CFG}_pmc_SQ > /dev/null
find $O/${TAG}_${CFG}_pmc_* -name "*.csv" -delete
rm -rf $O/${TAG}_${CFG}_kt
head -20 $O/${TAG}_${CFG}_kernel_stats.txt
cat $O/${TAG}_${CFG}_hbm_pmc.txt | head -20
grep "k_shoot" $O/${TAG}_${CFG}_sq_pmc.txt | head -20
