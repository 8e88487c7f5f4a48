"""The stamp pass of the FFT branch alone (ims_fft_image_factor), and one bright FITS-stamp object photon-shot against FFT-drawn.

    python tools/bench_stamp_fft.py [--steps 5] [--grids 1024 4096] [--stamp 64] [--skip-render] [--ccd 512]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_stamp_fft.py --skip-render      (the kernel's own time)

The pass: a --stamp x --stamp stamp with every pixel positive (4 096 pixels at 64) on one grid of each --grids size, a buffer of
ones, sheared J'; HIP events round the entry point, the median of --steps launches after two.  The kernel time proper comes from a
kernel trace of the same run (k_fft_image_factor in the statistics), in a run of its own.
The render (unless --skip-render): a 1e7-electron stamp object alone on a --ccd^2 CCD with the Silicon sensor through
LSST_ImageBuilder with fft_sb_thresh 1e4 (the estimate of this stamp under a 0.7" PSF is 2.9e4 per pixel), fft_stamps off (every photon through the sensor, its brighter-fatter rounds in sequence:
the path of before, untouched by the switch) and on; wall clock per image, synchronised, the median of --steps passes after one.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--grids", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--stamp", type=int, default=64)
    ap.add_argument("--ccd", type=int, default=512)
    ap.add_argument("--skip-render", action="store_true")
    args = ap.parse_args()
    import torch
    from imsim_amd import _abi, catalog, configs, fft_draw, lsst_image
    from imsim_amd.engine import Renderer
    dev = "cuda:0"
    lib = _abi.load()
    img = np.random.default_rng(5).uniform(0.5, 2.0, size=(args.stamp, args.stamp))
    out = {"stamp": args.stamp, "pixels": int((img > 0).sum())}
    size, offset, ab, w = fft_draw.image_pixel_lists([img])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to(dev)
    side = [up(np.zeros(1, dtype=np.int32)), up(np.zeros(1, dtype=np.int32)), up(size), up(offset), up(ab), up(w)]
    P = _abi.FftParams()
    P.pixel_scale, P.n_alias = 0.2, 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for nfft in args.grids:
        rows = np.zeros(1, dtype=_abi.FFT_OBJECT_DTYPE)
        # the stamp spans a quarter of the grid along each axis
        rows["nfft"], rows["jac"], rows["obj_id"], rows["prof_ktable"] = nfft, (0.9, 0.3, -0.2, 0.7), 7, -1
        rows["prof_scale"] = 0.25 * nfft * 0.2 / args.stamp
        obj_t = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev)
        kbuf = torch.ones(nfft * (nfft // 2 + 1), dtype=torch.complex128, device=dev)
        ms = []
        for k in range(args.steps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _abi.check(lib.ims_fft_image_factor(C.byref(P), obj_t.data_ptr(), side[0].data_ptr(), 1, nfft, side[1].data_ptr(), 1,
                                                side[2].data_ptr(), side[3].data_ptr(), side[4].data_ptr(), side[5].data_ptr(), 1,
                                                kbuf.data_ptr(), st), "ims_fft_image_factor")
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        out[f"factor_{nfft}_ms"] = float(np.median(ms[2:]))
        out[f"factor_{nfft}_ms_all"] = [round(t, 4) for t in ms]
        out[f"factor_{nfft}_gflop"] = 8.0e-9 * nfft * (nfft // 2 + 1) * out["pixels"]
        del kbuf
    if not args.skip_render:
        n, flux = args.ccd, 1.0e7
        kpsf = [(_abi.IMS_KPSF_GAUSSIAN, 0, 0.7 / 2.3548200450309493)]
        cat = dict(x=np.array([0.5 * n + 0.3]), y=np.array([0.5 * n - 0.4]), mag=np.zeros(1), nominal_flux=np.array([flux]),
                   sb_flux=np.array([flux]), kind=np.array([catalog.KIND_IMAGE], dtype=np.int32), hlr=np.zeros(1), q=np.ones(1),
                   pa=np.array([30.0]), obj_id=np.array([1], dtype=np.int64), n_knots=np.zeros(1), box_length=np.zeros(1),
                   box_width=np.zeros(1), image_index=np.zeros(1, dtype=np.int64), image_scale=np.array([0.05]),
                   image_extent=np.array([args.stamp * 0.05]), g1=np.zeros(1), g2=np.zeros(1), mu=np.ones(1))
        phot = np.array([int(flux)])
        out.update(ccd=n, flux=flux, image_scale=0.05)
        for name, on in (("on", True), ("off", False)):
            scene = configs.scene_c3(nx=n, ny=n)
            scene.sensor.scratch_cells = 2_000_000
            scene.image_profiles = [img]
            r = Renderer(scene, dev)
            b = lsst_image.LSST_ImageBuilder()
            b.setup({"det_name": "R22_S11", "xsize": n, "ysize": n})
            make = lambda c, p: configs.c3_objects(c, p, scene)
            times = []
            for k in range(args.steps + 1):
                r.image.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                truth = {}
                b.build_image(r, cat, phot, make, fft_sb_thresh=1.0e4, kpsf=kpsf, fwhm_total=0.7, truth=truth,
                              fft_stamps=on)
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0))
            out[f"{name}_ms"] = float(np.median(times[1:]))
            out[f"{name}_ms_all"] = [round(t, 3) for t in times]
            out[f"{name}_mode"] = str(truth["mode"][0])
            out[f"{name}_realized"] = float(truth["realized_flux"][0])
            del r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
