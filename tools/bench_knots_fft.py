"""One very bright RandomKnots galaxy among faint objects, photon-shot against FFT-drawn, and the structure-factor pass alone.

    python tools/bench_knots_fft.py [--ccd 512] [--steps 3] [--skip-render]

A 1e8-electron knots object (50 knots, half-light radius 0.5") among 1 000 faint objects on a CCD with the Silicon sensor, through
LSST_ImageBuilder with fft_sb_thresh 2e5: fft_knots off (every photon of the galaxy through the sensor, its brighter-fatter rounds
in sequence) and on (the FFT branch); wall-clock per image, synchronised, the median of --steps passes after one that warms up.
Then k_fft_knots_factor alone (HIP events round the entry point) on one 4096^2 grid with 50 and with 500 knots.  Prints one JSON line."""
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
    ap.add_argument("--ccd", type=int, default=512)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-render", action="store_true")
    args = ap.parse_args()
    import torch
    from imsim_amd import _abi, catalog, configs, fft_draw, lsst_image
    from imsim_amd.engine import Renderer
    n, flux, n_knots = args.ccd, 1.0e8, 50
    out = {"ccd": n, "flux": flux, "n_knots": n_knots, "faint": 1000}
    kpsf = [(_abi.IMS_KPSF_GAUSSIAN, 0, 0.7 / 2.3548200450309493)]
    if not args.skip_render:
        cat = catalog.synthetic_catalog(1001, nx=n, ny=n, mag_min=22.0)
        cat["x"][0], cat["y"][0], cat["kind"][0], cat["hlr"][0], cat["q"][0] = 0.5 * n + 0.3, 0.5 * n - 0.4, catalog.KIND_KNOTS, 0.5, 0.8
        cat["sb_flux"][0] = cat["sb_flux"][0] * flux / cat["nominal_flux"][0]
        cat["nominal_flux"][0] = flux
        cat["n_knots"] = np.where(cat["kind"] == catalog.KIND_KNOTS, float(n_knots), 0.0)
        phot = catalog.realize_fluxes(cat["nominal_flux"], 99)
        out["faint_max_flux"] = float(cat["nominal_flux"][1:].max())
        for name, on in (("on", True), ("off", False)):
            scene = configs.scene_c3(nx=n, ny=n)
            scene.sensor.scratch_cells = 2_000_000
            r = Renderer(scene, "cuda:0")
            b = lsst_image.LSST_ImageBuilder()
            b.setup({"det_name": "R22_S11", "xsize": n, "ysize": n})
            make = lambda c, p: configs.c3_objects(c, p, scene)
            times = []
            for k in range(args.steps + 1):
                r.image.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                truth = {}
                b.build_image(r, cat, phot, make, fft_sb_thresh=configs.C5_FFT_SB_THRESH, kpsf=kpsf, fwhm_total=0.7, truth=truth,
                              fft_knots=on)
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0))
            out[f"{name}_ms"] = float(np.median(times[1:]))
            out[f"{name}_ms_all"] = [round(t, 3) for t in times]
            out[f"{name}_mode"] = str(truth["mode"][0])
            out[f"{name}_realized"] = float(truth["realized_flux"][0])
            del r
    # the pass alone: one 4096^2 grid, a buffer of ones
    lib = _abi.load()
    nfft = 4096
    rows = np.zeros(1, dtype=_abi.FFT_OBJECT_DTYPE)
    rows["nfft"], rows["jac"], rows["obj_id"], rows["prof_ktable"] = nfft, (0.9, 0.3, -0.2, 0.7), 7, -1
    obj_t = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    which = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    off = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    sig = torch.full((1,), 0.4, dtype=torch.float64, device="cuda:0")
    kbuf = torch.ones(nfft * (nfft // 2 + 1), dtype=torch.complex128, device="cuda:0")
    P = _abi.FftParams()
    P.pixel_scale, P.n_alias = 0.2, 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for N in (50, 500):
        nk = torch.full((1,), N, dtype=torch.int32, device="cuda:0")
        xy = torch.empty(2 * N, dtype=torch.float64, device="cuda:0")
        _abi.check(lib.ims_knot_positions(11, obj_t.data_ptr(), 1, nk.data_ptr(), sig.data_ptr(), off.data_ptr(), xy.data_ptr(), st), "ims_knot_positions")
        ms = []
        for k in range(args.steps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _abi.check(lib.ims_fft_knots_factor(C.byref(P), obj_t.data_ptr(), which.data_ptr(), 1, nfft, nk.data_ptr(), off.data_ptr(),
                                                xy.data_ptr(), kbuf.data_ptr(), st), "ims_fft_knots_factor")
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        out[f"factor_4096_N{N}_ms"] = float(np.median(ms[2:]))
        out[f"factor_4096_N{N}_ms_all"] = [round(t, 4) for t in ms]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
