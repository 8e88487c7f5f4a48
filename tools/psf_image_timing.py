#!/usr/bin/env python
"""Time ims_psf_image against ims_psf_profile on the same rows: the same photons, binned into a stamp instead of a histogram.

Rows on tools/psf_profile_timing.py's scene (C3 on a 4096^2 CCD, the default operator chain, here with its Silicon sensor, of
which the renderer keeps the model and the absorption table only): one row of `--one-row` photons, and `--rows` rows of
`--photons` each (a 512 x 512 stamp is 2 MB per row).  Stamps of 64 x 64 cells (all in the LDS window) and 512 x 512 cells
(window plus global cells) of `--scale` pixels, in stages ops and sensor; the profile in stage ops with 32 radial bins, the
parent's kernel over the same photons.  The paths are run alternately, `--repeats` windows of `--inner` calls each after
`--warmup` untimed windows, every window between two device events; one JSON line per (table, path) with the median and the
spread of the per-call time, the ratio to the profile's median, and where the photons went.

    python tools/psf_image_timing.py [--one-row 100000000] [--rows 256] [--photons 400000] [--scale 0.25] [--repeats 10] [--inner 3]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from imsim_amd import configs, psf_image, psf_map, psf_profile    # noqa: E402

SIZES = (64, 512)
WIN = 64


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
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--photons", type=int, default=400_000)
    ap.add_argument("--scale", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    scene = configs.scene_c3(nx=4096, ny=4096, sensor=True)
    r = psf_image.renderer_for(scene, "sensor")
    side = int(round(a.rows ** 0.5))
    grid = psf_map.grid_points(scene.nx, scene.ny, side) if side * side == a.rows else \
        np.stack([np.linspace(100.0, 4000.0, a.rows), np.linspace(4000.0, 100.0, a.rows)], axis=1)
    tables = {"one_row": (np.array([[2048.5, 2048.5]]), a.one_row), "many_rows": (grid, a.photons)}
    for name, (xy, n) in tables.items():
        rows = psf_map.point_rows(scene, xy, n, "ops")
        paths = {"profile_32x0": psf_profile.Prepared(r, rows, "ops", psf_profile.radial_edges(0.1, 100.0, 32), 0)}
        for stage in ("ops", "sensor"):
            for size in SIZES:
                paths[f"image_{size}_{stage}"] = psf_image.Prepared(r, rows, stage, size, a.scale)
        times = {k: [] for k in paths}
        for w in range(a.warmup + a.repeats):
            for k, fn in paths.items():                   # alternating: all see the same neighbours on the machine
                ms = timed(r, fn, a.inner)
                if w >= a.warmup:
                    times[k].append(ms)
        prof = paths["profile_32x0"].result()
        base = statistics.median(times["profile_32x0"])
        for k, fn in paths.items():
            extra = {}
            if k != "profile_32x0":
                res = fn.result()
                assert np.array_equal(res.n_used + res.n_outside + res.n_dropped, rows["n_phot"]), "photons unaccounted for"
                assert np.array_equal(res.n_dropped, prof.n_dropped), "the two reductions drop different photons"
                ny, nx = res.counts.shape[1:]
                w0 = (nx - min(nx, WIN)) // 2
                in_window = int(res.counts[:, w0:w0 + WIN, w0:w0 + WIN].sum())
                total = int(rows["n_phot"].sum())
                extra = {"share_window": round(in_window / total, 5), "share_global_cells": round((int(res.n_used.sum()) - in_window) / total, 5),
                         "share_outside": round(int(res.n_outside.sum()) / total, 5), "share_dropped": round(int(res.n_dropped.sum()) / total, 5)}
            v = sorted(times[k])
            med = statistics.median(v)
            print(json.dumps({"table": name, "path": k, "rows": len(rows), "photons_per_row": int(n), "scale": a.scale,
                              "ms_median": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                              "ratio_to_profile": round(med / base, 3), "repeats": a.repeats, "calls_per_window": a.inner,
                              "photons_per_s": round(len(rows) * n / (med * 1e-3), 1), **extra}), flush=True)


if __name__ == "__main__":
    main()
