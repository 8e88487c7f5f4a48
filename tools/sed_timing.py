#!/usr/bin/env python3
"""sed.object_spectra (host, numpy) against sed.object_spectra_hip (ims_object_spectra) on the same synthetic inputs: a library
of two 3 801-point SEDs, a 530 - 710 nm band at 0.5 nm, 257-point tables, every object with its own redshift and A_v.

   python tools/sed_timing.py [--sizes 1000,10000,100000] [--repeats 3] [--host-max N]

Per size: host_s = wall clock of object_spectra; hip_s = wall clock of the whole object_spectra_hip call (packing the names,
uploads, launch, flux copy; the best of --repeats after one untimed call), of which pack_s = sed.pack_library alone and
launch_ms = the launch between two events; max_rel_flux = the largest relative difference of the two fluxes.  Sizes above
--host-max skip the host run.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,100000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-max", type=int, default=100000)
    args = ap.parse_args()
    import numpy as np
    import torch
    from imsim_amd import sed as sedmod
    d = tempfile.mkdtemp(prefix="sed_timing_")
    w = 100.0 + 0.5 * np.arange(3801)
    for name, temp in (("a.txt", 5500.0), ("b.txt", 3500.0)):
        np.savetxt(os.path.join(d, name), np.column_stack([w, 1.0e15 / w ** 5 / np.expm1(1.43877688e7 / (w * temp))]))
    library = sedmod.SedLibrary(d, None)
    wl = np.linspace(530.0, 710.0, 361)
    thr = 0.5 * np.clip(np.minimum(wl - 530.0, 710.0 - wl) / 15.0, 0.0, 1.0)
    out = {"device": torch.cuda.get_device_name(0), "n_pts": 257, "n_grid": len(sedmod.band_grid(wl, thr)[2]), "sizes": {}}
    for n in [int(s) for s in args.sizes.split(",")]:
        rng = np.random.default_rng(n)
        names = np.array(["a.txt", "b.txt"], dtype=object)[rng.integers(0, 2, n)]
        z, av, rv = rng.uniform(0.0, 2.0, n), rng.uniform(0.0, 1.0, n), np.where(rng.random(n) < 0.5, 3.1, 2.0)
        row = {}
        sedmod.object_spectra_hip(names, z, av, rv, wl, thr, library)            # untimed: library load, first launch
        best = None
        for _ in range(args.repeats):
            timing = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            flux, tabs, _ = sedmod.object_spectra_hip(names, z, av, rv, wl, thr, library, timing=timing)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if best is None or dt < best[0]:
                best = (dt, timing["launch_ms"])
        t0 = time.perf_counter()
        sedmod.pack_library(library, names)
        row.update(hip_s=best[0], launch_ms=best[1], pack_s=time.perf_counter() - t0)
        if n <= args.host_max:
            t0 = time.perf_counter()
            ref = sedmod.object_spectra(names, z, av, rv, wl, thr, library)
            row["host_s"] = time.perf_counter() - t0
            row["speedup"] = row["host_s"] / row["hip_s"]
            row["max_rel_flux"] = float(np.abs(flux / ref[0] - 1.0).max())
        out["sizes"][str(n)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
