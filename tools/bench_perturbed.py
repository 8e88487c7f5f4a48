#!/usr/bin/env python3
"""C3's catalog and step through the M2-decentred stand-in telescope (input.telescope.perturbations: M2 shift [100 um, 0, 0])
next to the nominal one: ms per step of each, and of the photon kernel.  bench.py's own measurement is left as it is.

   python tools/bench_perturbed.py [--steps 10] [--warmup 3] [--n-objects N]

Prints one JSON line: {"nominal_ms", "perturbed_ms", "ratio", ... }."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def perturbed_optics(nx, ny, perturbations):
    """configs.rubin_optics_struct for the stand-in with `perturbations` applied: the descriptor, the WCS pair fitted to the
    perturbed telescope and the spider geometry"""
    from imsim_amd import configs, diffraction, optics
    v = configs.VISIT
    tel = optics.apply_perturbations(optics.rubin_like_telescope(v["band"]), perturbations)
    fp = (100.0, 0.0, (nx - 1) / 2.0 + 1.0 - 0.5, 0.0, 100.0, (ny - 1) / 2.0 + 1.0 - 0.5)
    rot_tel = math.radians(v["rottelpos"])
    o = optics.make_optics(tel, fp, rot_tel)
    o.img_wcs, o.icrf_to_field, _ = optics.build_wcs_pair(tel, fp, math.radians(v["ra"]), math.radians(v["dec"]),
                                                          rot_sky=math.radians(v["rotskypos"]), rot_tel_pos=rot_tel, nx=nx, ny=ny)
    diffraction.fill_optics(o, math.radians(v["latitude"]), math.radians(v["azimuth"]), math.radians(v["altitude"]))
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-objects", type=int, default=0)
    args = ap.parse_args()
    import torch
    from imsim_amd import _abi, catalog, configs
    from imsim_amd.engine import Renderer
    cfg = configs.BENCH_CONFIGS["c3"]
    lib = _abi.load()
    out = {"perturbation": {"M2": {"shift": [100e-6, 0.0, 0.0]}}}
    for label in ("nominal", "perturbed"):
        scene = cfg["scene"]()
        if label == "perturbed":
            scene.optics = perturbed_optics(scene.nx, scene.ny, out["perturbation"])
        n_obj = args.n_objects or cfg["n_objects"]
        cat = catalog.synthetic_catalog(n_obj, nx=scene.nx, ny=scene.ny)
        phot = catalog.realize_fluxes(cat["nominal_flux"], scene.seed)
        objects, _ = cfg["objects"](cat, phot, scene)
        r = Renderer(scene, "cuda:0")
        r.touch_streams()
        step = cfg["make_step"](r, objects)
        for _ in range(args.warmup):
            r.image.zero_()
            step()
        torch.cuda.synchronize()
        lib.ims_enable_timing(cfg["timed_kernel"])
        ms, nl = _abi.C.c_float(), _abi.C.c_int()
        lib.ims_last_kernel_ms(_abi.C.byref(ms), _abi.C.byref(nl))
        t0 = time.perf_counter()
        for _ in range(args.steps):
            r.image.zero_()
            step()
        torch.cuda.synchronize()
        out[f"{label}_ms"] = 1e3 * (time.perf_counter() - t0) / args.steps
        lib.ims_last_kernel_ms(_abi.C.byref(ms), _abi.C.byref(nl))
        lib.ims_enable_timing(0)
        out[f"{label}_kernel_ms"] = ms.value / args.steps
        out[f"{label}_image_sum"] = float(r.image.sum().item())
        out["photons"] = int(objects["n_phot"].sum())
        del r
        torch.cuda.synchronize()
    out["ratio"] = out["perturbed_ms"] / out["nominal_ms"]
    out["kernel_ratio"] = out["perturbed_kernel_ms"] / out["nominal_kernel_ms"] if out["nominal_kernel_ms"] else None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
