#!/bin/bash
# end of a round: the GPU suite, smoke, and the --full bench line (every config, CPU baselines and parity)
# outputs under $OUT_DIR (default profile_out/)
ulimit -c 0
O=${OUT_DIR:-profile_out}
mkdir -p $O
timeout 2400 python -m pytest tests -m gpu -x -q 2>&1 | tail -3 > $O/final_tests.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2 > $O/final_smoke.log
SECONDS=0
timeout 900 python bench.py --full > $O/final_bench.json 2> $O/final_bench.err
echo "default bench wall: $SECONDS s" > $O/final_bench_wall.log
cat $O/final_tests.log $O/final_smoke.log $O/final_bench_wall.log
python - <<'PY'
import json
import os
d = json.loads([l for l in open(os.environ.get("OUT_DIR", "profile_out") + "/final_bench.json") if l.startswith("{")][-1])
print(d["ms_per_step"], d["value"], d["roofline"].get("frac"), d["roofline"].get("step", {}).get("frac"))
for k, c in d["extra"]["configs"].items():
    print(k, c.get("ms_per_step"), c.get("objects_per_s"), c.get("bit_identical"), c.get("wall_s"))
print(d["cpu_baseline"]["parity"])
PY
