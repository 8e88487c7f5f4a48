#!/usr/bin/env python3
"""C3b's catalog and step with the optical phase screen of AtmosphericPSF (input.atm_psf.doOpt) next to the same scene without it:
ms per step of each.  bench.py's own measurement (`--config c3b`, the component off) is left as it is.

   python tools/bench_doopt.py --data-dir DIR [--steps 10] [--warmup 3] [--n-objects N] [--only on|off]

DIR holds optics_data/ (an imSim data directory; tests/golden of this repository has the three tables, gzipped).
Prints one JSON line: {"off_ms", "on_ms", "ratio", ...}."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-objects", type=int, default=0)
    ap.add_argument("--data-dir", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", choices=("on", "off"), default=None)
    args = ap.parse_args()
    import torch
    from imsim_amd import catalog, configs
    from imsim_amd.engine import Renderer
    cfg = configs.BENCH_CONFIGS["c3b"]
    out = {}
    for label in ("off", "on"):
        if args.only and label != args.only:
            continue
        dev = torch.device("cuda", torch.cuda.current_device())
        scene = configs.scene_c3b(device=dev, optical=dict(doOpt=True, data_dir=args.data_dir) if label == "on" else None)
        scene.sensor.scratch_cells = 24_000_000
        scene.sensor.max_slots = 8192
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
        t0 = time.perf_counter()
        for _ in range(args.steps):
            r.image.zero_()
            step()
        torch.cuda.synchronize()
        out[f"{label}_ms"] = 1e3 * (time.perf_counter() - t0) / args.steps
        out[f"{label}_image_sum"] = float(r.image.sum().item())
        out["photons"] = int(objects["n_phot"].sum())
        del r, scene
        torch.cuda.synchronize()
    if "on_ms" in out and "off_ms" in out:
        out["ratio"] = out["on_ms"] / out["off_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
