#!/usr/bin/env python
"""Time the PSF moments of 64 points x 1e5 photons two ways, in stage 1 (shoot + PSF) and stage 2 (+ the default operator chain):

  moments   ims_psf_moments: the photons reduced where they are made (two launches, 64 B of scratch per 256 photons)
  pool      ims_shoot_ops_photons into a pool that is not converted (x, y, flux, dxdz, dydz, wavelength: 48 B per photon written),
            then the same six sums and two counts with torch reductions over the pool

The two are run alternately, `--repeats` windows of `--inner` calls each after `--warmup` untimed windows, every window between two
device events; the median and the spread of the per-call time are printed as one JSON line per (stage, path), with the bytes
each path has to move by its algorithm (the torch reductions move more than that: every elementwise product is a pass of its own).

    python tools/psf_moments_timing.py [--points 64] [--photons 100000] [--repeats 20] [--inner 5] [--warmup 3]"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from imsim_amd import _abi, configs, psf_map                     # noqa: E402
from imsim_amd.engine import _seg_ptr                             # noqa: E402

POOL_FIELDS = ("x", "y", "flux", "dxdz", "dydz", "wavelength")


def pool_path(r, rows, stage):
    """(callable, result getter): shoot into a pool, reduce with torch.  Stage 1 shoots with no operators bound (the renderer of
    a scene without them)."""
    torch = r.torch
    rows, obj_t, prefix, pre_t = r._upload_objects(rows)
    n_pts, n = len(rows), int(rows["n_phot"][0])
    assert np.all(rows["n_phot"] == n), "equal counts: the pool is viewed as [points][photons]"
    offs = torch.arange(0, (n_pts + 1) * n, n, dtype=torch.int64, device=r.device)
    t = {f: torch.empty(n_pts * n, dtype=torch.float64, device=r.device) for f in POOL_FIELDS}
    ph = _abi.Photons()
    ph.n, ph.converted = n_pts * n, 0
    for f in POOL_FIELDS:
        setattr(ph, f, t[f].data_ptr())
    P = r.bound.params(obj_t.data_ptr(), n_pts, pre_t.data_ptr(), int(prefix[-1]), r.image.data_ptr(), None, _seg_ptr(pre_t))
    x0 = torch.from_numpy(np.ascontiguousarray(rows["x0"] if stage == "ops" else np.zeros(n_pts))).to(r.device)[:, None]
    y0 = torch.from_numpy(np.ascontiguousarray(rows["y0"] if stage == "ops" else np.zeros(n_pts))).to(r.device)[:, None]
    keep = (obj_t, pre_t, offs, t, P, ph)
    out = {}

    def run():
        _abi.check(r.lib.ims_shoot_ops_photons(C.byref(P), offs.data_ptr(), C.byref(ph), r._stream()), "ims_shoot_ops_photons")
        w = t["flux"].view(n_pts, n)
        dx, dy = t["x"].view(n_pts, n) - x0, t["y"].view(n_pts, n) - y0
        wx, wy = w * dx, w * dy
        out["sums"] = torch.stack([w.sum(1), wx.sum(1), wy.sum(1), (wx * dx).sum(1), (wx * dy).sum(1), (wy * dy).sum(1)], dim=1)
        out["used"] = (w != 0).sum(1)
    run.keep = keep
    return run, out


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
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--photons", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    scene = configs.scene_c3(nx=4096, ny=4096, sensor=False)
    side = int(round(a.points ** 0.5))
    xy = psf_map.grid_points(scene.nx, scene.ny, side) if side * side == a.points else \
        np.stack([np.linspace(100.0, 4000.0, a.points), np.linspace(4000.0, 100.0, a.points)], axis=1)
    n_phot = a.points * a.photons
    n_seg = a.points * -(-a.photons // 256)
    for stage in ("psf", "ops"):
        sc = scene if stage == "ops" else dataclasses.replace(scene, ops=[])
        r = psf_map.renderer_for(sc)
        rows = psf_map.point_rows(sc, xy, a.photons, stage)
        if stage == "psf":
            rows["x0"], rows["y0"] = 0.0, 0.0                 # stage 1 never adds the position; the pool then holds the kicks alone
        mom = psf_map.Prepared(r, rows, stage)
        pool, pool_out = pool_path(r, rows, stage)
        paths = {"moments": mom, "pool": pool}
        times = {k: [] for k in paths}
        for w in range(a.warmup + a.repeats):
            for k, fn in paths.items():                       # alternating: both see the same neighbours on the machine
                ms = timed(r, fn, a.inner)
                if w >= a.warmup:
                    times[k].append(ms)
        sums, counts = mom.raw()
        ref = pool_out["sums"].cpu().numpy()
        scale = np.abs(ref).max(axis=0)
        assert np.array_equal(counts[:, 0], pool_out["used"].cpu().numpy())
        assert np.all(np.abs(sums - ref) <= 1e-9 * scale), "the two paths disagree"
        algo = {"moments": 256 * a.points + 2 * 64 * n_seg + 64 * a.points,
                "pool": 256 * a.points + 48 * n_phot + 24 * n_phot + 56 * a.points}
        for k in paths:
            v = sorted(times[k])
            print(json.dumps({"stage": stage, "path": k, "points": a.points, "photons_per_point": a.photons,
                              "ms_median": round(statistics.median(v), 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                              "repeats": a.repeats, "calls_per_window": a.inner, "algorithmic_hbm_bytes": algo[k],
                              "photons_per_s": round(n_phot / (statistics.median(v) * 1e-3), 1)}))


if __name__ == "__main__":
    main()
