"""Time the re-shooting stage (ims_fft_reshoot) beside the rest of the FFT branch and beside photon shooting of the same star.

One point source of `--flux` e- on an `--nfft` grid (stamp = grid) through Kolmogorov + Gaussian, imSim's default six-operator
chain, no sensor, no noise.  Per configuration, medians over `--reps` repetitions after `--warmup`, by device events:

  fft      the FFT branch without the stage (k-space fill, inverse transform, finish)
  reshoot  the same with the stage; the stage is the difference, and is also timed alone (the entry point on the drawn buffer)
  shoot    ims_shoot_accumulate of the same star with the same chain in a scene without a sensor (a FAINT-flagged row would skip the
           operators too): the existing kernel that does comparable work per photon

Prints one JSON line per configuration.  Not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flux", type=float, nargs="+", default=[1.0e7, 1.0e8])
    ap.add_argument("--nfft", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stage-only", action="store_true", help="time nothing but the stage (for a counter run of its own)")
    args = ap.parse_args()
    import torch
    from imsim_amd import _abi, catalog, configs, fft_draw
    from imsim_amd.engine import Renderer, Scene
    tests = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
    sys.path.insert(0, tests)
    import photon_ops_cases as pc                       # the optics block and WCS of the operator tests
    ops = configs.c3_ops(30.0, 620.0)
    for nfft in args.nfft:
        for flux in args.flux:
            sc = Scene(nx=4096, ny=4096, seed=pc.SEED, psf=[], ops=ops, optics=pc.optics_block())
            po = pc.rows(1)
            po["obj_id"], po["x0"], po["y0"], po["dcr_tanz"] = 9, 2048.3, 2048.6, 0.5
            po["winv"] = [[5.0, 0.0, 0.0, 5.0]]
            half = nfft // 2
            po["stamp_xmin"], po["stamp_xmax"], po["stamp_ymin"], po["stamp_ymax"] = 2048 - half, 2047 + half, 2048 - half, 2047 + half
            rows, order = fft_draw.build_fft_objects(po, np.array([flux]), np.array([_abi.IMS_PROF_POINT]))
            assert list(rows["nfft"]) == [nfft]
            kpsf = fft_draw.kolmogorov_gaussian_kpsf(0.7, 0.3)
            r = Renderer(sc)
            plain = fft_draw.FftDrawer(r, kpsf, add_noise=False).prepared(rows)
            R = fft_draw.Reshoot(r)
            drawer = fft_draw.FftDrawer(r, kpsf, add_noise=False, reshoot=R)
            state = drawer._upload(rows, photon_objects=po[order])
            shot = lambda: drawer._run(state, None)
            shot()
            r.synchronize()
            rs = state.reshoot
            raw = int(fft_draw.raw_inverse())
            rpre_t, rbuf = state[6], state[8]

            def stage():
                _abi.check(r.lib.ims_fft_reshoot(C.byref(drawer.P), C.byref(R.P), state[1].data_ptr(), rs["rows"].ctypes.data, rs["po"].data_ptr(),
                                                 1, rpre_t.data_ptr(), nfft * nfft, rbuf.data_ptr(), raw, 1.0, rs["work"].data_ptr(),
                                                 rs["out"].data_ptr(), None, None, None, 0, 0, r._stream()), "ims_fft_reshoot")
            stage()
            r.synchronize()
            n_phot = int(rs["work"].view(torch.int64)[-1].item())
            rec = dict(nfft=nfft, flux=flux, photons=n_phot)
            t = median_ms(torch, stage, args.warmup, args.reps)
            rec["stage_ms"], rec["stage_min_ms"], rec["stage_max_ms"] = t
            rec["stage_photons_per_s"] = n_phot / (t[0] * 1e-3)
            if not args.stage_only:
                rec["fft_ms"] = median_ms(torch, plain, args.warmup, args.reps)[0]
                rec["fft_with_stage_ms"] = median_ms(torch, shot, args.warmup, args.reps)[0]
                # the same star photon-shot.  A FAINT-flagged row would skip the operators as well as the sensor, so the
                # row stays bright and the scene has no sensor: the fused kernel then runs the chain and lands the photons plainly
                ph = np.array(po, copy=True)
                ph["n_phot"], ph["phot_first"], ph["flux_per_photon"] = int(flux), 0, 1.0
                prep = r.prepared(ph)
                t = median_ms(torch, prep, args.warmup, args.reps)
                rec["shoot_ms"], rec["shoot_photons_per_s"] = t[0], int(flux) / (t[0] * 1e-3)
            print(json.dumps(rec), flush=True)
            del r, drawer, plain, state


if __name__ == "__main__":
    main()
