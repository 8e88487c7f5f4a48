#!/usr/bin/env python
"""Time psf_map.adaptive() to convergence against one ims_psf_moments call on the same rows: 64 points x 1e5 photons, stage 1
(shoot + PSF) and stage 2 (+ the default operator chain).

  moments    one ims_psf_moments call (two launches)
  adaptive   psf_map.adaptive(): that call for the start, then rounds of (pass, update) in batches of 16 with the statuses read
             between batches, until no row is running

The two are run alternately, `--repeats` windows after `--warmup` untimed ones, every window between two device events (the
adaptive window includes the host's reads of the statuses, which are part of what a caller waits for); one JSON line per
(stage, path) with the median and the spread, and for `adaptive` the rounds enqueued and the rows' iteration counts.

    python tools/psf_adaptive_timing.py [--points 64] [--photons 100000] [--repeats 10] [--warmup 2] [--tol 1e-6]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from imsim_amd import configs, psf_map                           # noqa: E402


def timed(r, fn):
    torch = r.torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--photons", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tol", type=float, default=1e-6)
    a = ap.parse_args()
    scene = configs.scene_c3(nx=4096, ny=4096, sensor=False)
    side = int(round(a.points ** 0.5))
    xy = psf_map.grid_points(scene.nx, scene.ny, side) if side * side == a.points else \
        np.stack([np.linspace(100.0, 4000.0, a.points), np.linspace(4000.0, 100.0, a.points)], axis=1)
    for stage in ("psf", "ops"):
        sc = scene if stage == "ops" else dataclasses.replace(scene, ops=[])
        r = psf_map.renderer_for(sc)
        rows = psf_map.point_rows(sc, xy, a.photons, stage)
        mom = psf_map.Prepared(r, rows, stage)
        paths = {"moments": mom, "adaptive": lambda: psf_map.adaptive(sc, rows, stage=stage, tol=a.tol, renderer=r)}
        times, last = {k: [] for k in paths}, None
        for w in range(a.warmup + a.repeats):
            for k, fn in paths.items():                       # alternating: both see the same neighbours on the machine
                ms, out = timed(r, fn)
                if w >= a.warmup:
                    times[k].append(ms)
                if k == "adaptive":
                    last = out
        iters = last["iter"]
        rounds = -(-int(iters.max()) // psf_map.ADAPTIVE_ROUNDS) * psf_map.ADAPTIVE_ROUNDS
        unweighted = mom.result()
        for k in paths:
            v = sorted(times[k])
            line = {"stage": stage, "path": k, "points": a.points, "photons_per_point": a.photons,
                    "ms_median": round(statistics.median(v), 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4), "repeats": a.repeats}
            if k == "adaptive":
                line.update(tol=a.tol, rounds_enqueued=rounds, iter_min=int(iters.min()), iter_median=float(np.median(iters)),
                            iter_max=int(iters.max()), status_counts=np.bincount(last["status"], minlength=4).tolist(),
                            sigma_adaptive_median=float(np.median(last["sigma"])),
                            sigma_unweighted_median=float(np.median(unweighted["sigma"])))
            print(json.dumps(line))


if __name__ == "__main__":
    main()
