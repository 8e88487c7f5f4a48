#!/usr/bin/env python
"""Time ims_psf_profile against ims_psf_moments on the same rows: the same photons, reduced to a histogram instead of to six sums.

Rows on tools/psf_moments_timing.py's table (the C3 scene on a 4096^2 CCD; stage 1 shoot + PSF, stage 2 + the default operator
chain): one row of `--one-row` photons, and `--rows` rows of `--photons` each.  Shapes (n_r, n_phi) = (32, 0) and (64, 64),
log-spaced edges.  The paths are run alternately, `--repeats` windows of `--inner` calls each after `--warmup` untimed windows,
every window between two device events; one JSON line per (table, stage, path) with the median and the spread of the per-call
time and the ratio to the moments' median.

    python tools/psf_profile_timing.py [--one-row 100000000] [--rows 4096] [--photons 25000] [--repeats 10] [--inner 3] [--warmup 2]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from imsim_amd import configs, psf_map, psf_profile               # noqa: E402

SHAPES = ((32, 0), (64, 64))


def timed(r, fn, inner):
    torch = r.torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one-row", type=int, default=100_000_000)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--photons", type=int, default=25_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    scene = configs.scene_c3(nx=4096, ny=4096, sensor=False)
    side = int(round(a.rows ** 0.5))
    grid = psf_map.grid_points(scene.nx, scene.ny, side) if side * side == a.rows else \
        np.stack([np.linspace(100.0, 4000.0, a.rows), np.linspace(4000.0, 100.0, a.rows)], axis=1)
    tables = {"one_row": (np.array([[2048.5, 2048.5]]), a.one_row), "many_rows": (grid, a.photons)}
    for stage in ("psf", "ops"):
        sc = scene if stage == "ops" else dataclasses.replace(scene, ops=[])
        r = psf_map.renderer_for(sc)
        r_max = 20.0 if stage == "psf" else 100.0            # arcsec / pixels
        for name, (xy, n) in tables.items():
            rows = psf_map.point_rows(sc, xy, n, stage)
            paths = {"moments": psf_map.Prepared(r, rows, stage)}
            for n_r, n_phi in SHAPES:
                paths[f"profile_{n_r}x{n_phi}"] = psf_profile.Prepared(r, rows, stage, psf_profile.radial_edges(r_max * 1e-3, r_max, n_r),
                                                                      n_phi)
            times = {k: [] for k in paths}
            for w in range(a.warmup + a.repeats):
                for k, fn in paths.items():                   # alternating: all see the same neighbours on the machine
                    ms = timed(r, fn, a.inner)
                    if w >= a.warmup:
                        times[k].append(ms)
            used = paths["moments"].raw()[1][:, 0]
            base = statistics.median(times["moments"])
            for k, fn in paths.items():
                if k != "moments":
                    res = fn.result()
                    assert np.array_equal(res.n_used, used), "the two reductions count different photons"
                    inside = int(res.counts[:, 1:-1].sum())
                v = sorted(times[k])
                med = statistics.median(v)
                print(json.dumps({"table": name, "stage": stage, "path": k, "rows": len(rows), "photons_per_row": int(n),
                                  "ms_median": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                                  "ratio_to_moments": round(med / base, 3), "repeats": a.repeats, "calls_per_window": a.inner,
                                  "photons_per_s": round(len(rows) * n / (med * 1e-3), 1),
                                  **({} if k == "moments" else {"share_inside_edges": round(inside / max(int(used.sum()), 1), 4)})}),
                      flush=True)


if __name__ == "__main__":
    main()
