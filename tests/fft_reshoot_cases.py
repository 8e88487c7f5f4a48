"""The hand-made batch of the re-shooting tests (tests/test_fft_reshoot.py on the restatement alone, tests/test_fft_reshoot_gpu.py
on the device): two FFT rows on grids of 32 and 64 with stamps smaller than their grids, off-centre and non-square (20 x 13 and
37 x 50), values everywhere -- those outside the stamps must be ignored -- and inside the stamps zeros, negatives, fractions below 1,
exactly 1.0, the next double above 1.0 (two photons), 2.5, and one pixel of BIG = 3 RUN + 100.5 e-: 12 389 photons, which no three of
the kernel's runs of RUN = IMS_RESHOOT_RUN photon numbers hold.  About 16 000 photons in all.

The reference of every chain is computed once per process and shared."""
import functools

import numpy as np

import fft_reshoot_ref as ref
import photon_ops_cases as pc
from imsim_amd import _abi, configs
from imsim_amd._abi import FFT_OBJECT_DTYPE

RUN = _abi.IMS_RESHOOT_RUN                        # photon numbers per run of the shooting kernel (include/imsim_hip.h)
BIG = 3.0 * RUN + 100.5
TIME_OP = (_abi.IMS_OP_TIME_SAMPLER, 0, [0.0, 30.0])
CHAINS = {
    "time": [TIME_OP],                                                            # moves nothing
    "default": configs.c3_ops(30.0, 620.0),                                       # the six operators: the CHAIN 1 kernels
    "descriptor": configs.c3_ops(30.0, 620.0)[:2] + [(_abi.IMS_OP_RUBIN_DIFFRACTION, 0, [1.0, 0.0])],      # CHAIN 0
}


def fft_rows():
    o = np.zeros(2, dtype=FFT_OBJECT_DTYPE)
    o["obj_id"] = [2 ** 32 + 5, 7]
    o["nfft"] = [32, 64]
    o["x0"], o["y0"] = [2000, 2100], [1990, 2050]
    o["stamp_xmin"] = o["x0"] + [5, 3]
    o["stamp_xmax"] = o["stamp_xmin"] + [19, 36]
    o["stamp_ymin"] = o["y0"] + [11, 9]
    o["stamp_ymax"] = o["stamp_ymin"] + [12, 49]
    o["r_offset"] = [0, 32 * 32]
    o["k_offset"] = [0, 32 * 17]
    o["cx"], o["cy"] = [15.0, 21.0], [17.0, 34.0]
    o["prof_ktable"] = _abi.IMS_PROF_POINT
    return o


def values(fft=None):
    """the real-space buffer as the image holds it"""
    fft = fft_rows() if fft is None else fft
    rng = np.random.default_rng(11)
    v = rng.uniform(-0.5, 3.0, int((fft["nfft"].astype(np.int64) ** 2).sum()))
    for i, o in enumerate(fft):
        n = int(o["nfft"])
        g = v[int(o["r_offset"]):int(o["r_offset"]) + n * n].reshape(n, n)
        ix, iy = int(o["stamp_xmin"] - o["x0"]), int(o["stamp_ymin"] - o["y0"])
        g[iy, ix:ix + 3] = 0.0                                                     # the stamp's first pixels spawn nothing
        g[iy + 1, ix + 4] = -0.0
        g[iy + 2, ix + 1], g[iy + 2, ix + 2], g[iy + 2, ix + 3] = 1.0, np.nextafter(1.0, 2.0), 2.5
        g[iy + 3, ix + 1], g[iy + 3, ix + 2], g[iy + 3, ix + 3] = -1.0, -np.nextafter(1.0, 2.0), -2.5
        g[iy + 4, ix + 5], g[iy + 4, ix + 6] = 0.25, -0.75
        if i == 0:
            g[iy + 6, ix + 9] = BIG
    fft["flux"] = [v[int(o["r_offset"]):int(o["r_offset"]) + int(o["nfft"]) ** 2].sum() for o in fft]
    return v


def sed_tables():
    u = np.linspace(0.0, 1.0, 64)
    return (540.0 + 160.0 * u ** 1.5)[None, :]


def photon_rows(fft=None):
    fft = fft_rows() if fft is None else fft
    o = pc.rows(2)
    o["obj_id"] = fft["obj_id"]
    o["phot_first"], o["n_phot"] = 0, 0
    for f in ("stamp_xmin", "stamp_xmax", "stamp_ymin", "stamp_ymax"):
        o[f] = fft[f]
    o["x0"], o["y0"] = fft["x0"] + fft["cx"], fft["y0"] + fft["cy"]
    o["sed_table"], o["sed_wave"] = [-1, 0], [620.0, 0.0]
    return o


def scene(chain):
    ops = CHAINS[chain]
    needs_optics = any(k in (pc.R_OPT, pc.R_DIFF, pc.R_DOPT) for k, _, _ in ops)
    return pc._scene(ops, optics=pc.optics_block() if needs_optics else None, sed_tables=sed_tables())


def blocks(sc):
    return dict(seed=sc.seed, optics=sc.optics, ratio_tables=None, ratio_wl_min=0.0, ratio_wl_step=1.0)


@functools.lru_cache(maxsize=None)
def reference(chain):
    """(fft rows, photon rows, values, scene, out, made, result of the operators) of a chain, computed once"""
    fft = fft_rows()
    v = values(fft)
    po = photon_rows(fft)
    sc = scene(chain)
    out, made, res = ref.reshoot(fft, po, v, sc.seed, sc.ops, blocks(sc), sed_tables=sed_tables())
    return fft, po, v, sc, out, made, res
