"""One bright satellite trail, photon-shot against FFT-drawn, and the k-space fill of a batch of such trails.

    python tools/bench_streak_fft.py [--steps 3] [--batch 64] [--skip-phot] [--lib other/libimsim_hip.so]

A 5e7-electron streak of 30 x 0.5 arcsec on a 512^2 CCD with the Silicon sensor, through LSST_ImageBuilder: draw_method `phot`
(every photon through the sensor, the brighter-fatter rounds in sequence -- what every streak did before the box had a k-space
form) and draw_method `fft`; wall-clock per image, synchronised.  Then the fill kernel alone (ims_enable_timing(3)) on a batch of
such streaks.  --lib: another build of the library, e.g. one compiled with -DIMS_FILL_BOX_PLAIN (the box's sincs by dsincos at every
point instead of the angle-addition tables in LDS), to put the two forms of the fill side by side.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--skip-phot", action="store_true")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    import torch
    from imsim_amd import _abi, catalog, configs, fft_draw, lsst_image
    if args.lib:
        _abi._LIB_PATH = os.path.abspath(args.lib)
    from imsim_amd.engine import Renderer
    n, flux = 512, 5.0e7
    cat = catalog.synthetic_catalog(1, nx=n, ny=n)
    cat["x"][:], cat["y"][:], cat["kind"][:], cat["nominal_flux"][:], cat["pa"][:] = 256.3, 250.7, catalog.KIND_STREAK, flux, 37.0
    cat["sb_flux"] = cat["nominal_flux"] / 80.0
    cat["box_length"], cat["box_width"] = np.array([30.0]), np.array([0.5])
    phot = catalog.realize_fluxes(cat["nominal_flux"], 99)
    kpsf = [(_abi.IMS_KPSF_GAUSSIAN, 0, 0.7 / 2.3548200450309493)]
    out = {"flux": flux, "length": 30.0, "width": 0.5, "ccd": n, "lib": args.lib or "in-tree"}
    for method in ("fft",) if args.skip_phot else ("fft", "phot"):
        scene = configs.scene_c3(nx=n, ny=n)
        scene.sensor.scratch_cells = 2_000_000             # the trail's private brighter-fatter region: a stamp of 300 pixels and more
        r = Renderer(scene, "cuda:0")
        b = lsst_image.LSST_ImageBuilder()
        b.setup({"det_name": "R22_S11", "xsize": n, "ysize": n})
        make = lambda c, p: configs.c3_objects(c, p, scene)
        times = []
        for k in range(args.steps + 1):                    # the first pass warms up (hipFFT plans, kernel loads)
            r.image.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            truth = {}
            b.build_image(r, cat, phot, make, kpsf=kpsf, fwhm_total=0.7, draw_method=method, truth=truth)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        out[f"{method}_ms"] = float(np.median(times[1:]))
        out[f"{method}_mode"] = str(truth["mode"][0])
        out[f"{method}_realized"] = float(truth["realized_flux"][0])
        del r
    # the fill kernel on a batch of such streaks
    scene = configs.scene_c3(nx=n, ny=n, sensor=False)
    objects, _ = configs.c3_objects(cat, phot, scene)
    rows, _ = fft_draw.build_fft_objects(np.repeat(objects, args.batch), np.full(args.batch, flux), np.full(args.batch, _abi.IMS_PROF_BOX))
    r = Renderer(scene, "cuda:0")
    draw = fft_draw.FftDrawer(r, kpsf, add_noise=False).prepared(rows)
    draw()
    torch.cuda.synchronize()
    lib = _abi.load()
    lib.ims_enable_timing(3)
    ms, nl = _abi.C.c_float(), _abi.C.c_int()
    lib.ims_last_kernel_ms(_abi.C.byref(ms), _abi.C.byref(nl))
    for _ in range(args.steps):
        draw()
    torch.cuda.synchronize()
    lib.ims_last_kernel_ms(_abi.C.byref(ms), _abi.C.byref(nl))
    lib.ims_enable_timing(0)
    out.update(batch=args.batch, nfft=int(rows["nfft"][0]), fill_kernel_ms=ms.value / args.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
