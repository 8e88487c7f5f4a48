"""ims_fft_reshoot restated in numpy: an FFT-drawn stamp turned into photons (GalSim's PhotonArray.makeFromImage, stated from its
source), the photon operators through tests/photon_ops_ref.py, the fixed-point binning.

Imports nothing of imsim_amd but constants of _abi.  The arithmetic that has to be bit for bit is exact here: the counts are one IEEE
division and a ceil, a photon's flux one IEEE division, its position an integer plus (w + 1/2) / 2^32 - 1/2 (46 significant bits at
most for |pixel| < 2^20), the deposit rint(flux * 2^32) in int64, the sums integer sums.  Only the wavelength (a table lookup) and
what the operators do carry a tolerance: photon_source_ref's and photon_ops_ref's own.

A batch is (fft rows, photon rows, values): FFT_OBJECT_DTYPE rows, the OBJECT_DTYPE rows of the same catalog objects, and the
real-space buffer AS THE IMAGE HOLDS IT (1 / nfft^2 applied), all grids back to back."""
import numpy as np

import photon_ops_ref as ops_ref
from photon_source_ref import LD, lin_lookup, w01, words
from imsim_amd import _abi

SLOT_RESHOOT = _abi.IMS_SLOT_RESHOOT
RUN = _abi.IMS_RESHOOT_RUN
Q32 = 2.0 ** 32


def counts(v, max_flux=1.0):
    """photons per pixel: 0 for v == 0, 1 for |v| <= max_flux, else ceil(|v| / max_flux)"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.ceil(a / np.float64(max_flux))
        n = np.where(a == 0.0, 0.0, np.where(a <= max_flux, 1.0, np.where(q < 2.0 ** 62, q, 0.0)))
    return n.astype(np.int64)


def in_stamp(o):
    """[nfft][nfft] mask of the grid points inside the row's stamp rectangle (k_fft_finish's test), and their CCD pixels"""
    n = int(o["nfft"])
    px = int(o["x0"]) + np.arange(n)[None, :] + np.zeros((n, 1), dtype=np.int64)
    py = int(o["y0"]) + np.arange(n)[:, None] + np.zeros((1, n), dtype=np.int64)
    ok = (px >= o["stamp_xmin"]) & (px <= o["stamp_xmax"]) & (py >= o["stamp_ymin"]) & (py <= o["stamp_ymax"])
    return ok, px, py


def make_photons(fft_rows, phot_rows, values, seed, sed_tables=None, max_flux=1.0):
    """The photons as made, before the operators, in pool order (object after object, ordinal ascending).
    Returns dict(fields: {name: float64[n]} of photon_ops_ref.FIELDS, wl_bound, obj_index int32, ordinal int64, source int64 (grid
    point the photon came from), offset int64 [n_objects + 1], n_per_pixel: list of int64 [nfft * nfft])"""
    out = {q: [] for q in ops_ref.FIELDS}
    wl_bound, obj_index, ordinal, source, n_pp, offset = [], [], [], [], [], [0]
    for i, (o, po) in enumerate(zip(fft_rows, phot_rows)):
        n = int(o["nfft"])
        v = np.asarray(values[int(o["r_offset"]):int(o["r_offset"]) + n * n], dtype=np.float64).reshape(n, n)
        ok, px, py = in_stamp(o)
        cnt = np.where(ok, counts(v, max_flux), 0).reshape(-1)                 # row-major over the grid = row-major over the stamp
        n_pp.append(cnt)
        tot = int(cnt.sum())
        src = np.repeat(np.arange(n * n, dtype=np.int64), cnt)
        k = np.arange(tot, dtype=np.int64)
        w = words(seed, int(po["obj_id"]), k, SLOT_RESHOOT)
        vv, nn = v.reshape(-1)[src], cnt[src]
        flux = np.where(nn == 1, vv, vv / np.maximum(nn, 1).astype(np.float64))
        x = (px.reshape(-1)[src].astype(LD) + (w01(w[1]) - LD(0.5))).astype(np.float64)
        y = (py.reshape(-1)[src].astype(LD) + (w01(w[2]) - LD(0.5))).astype(np.float64)
        if int(po["sed_table"]) >= 0:
            wl, wb = lin_lookup(np.asarray(sed_tables, dtype=np.float64)[int(po["sed_table"])], w01(w[0]))
        else:
            wl, wb = np.full(tot, LD(po["sed_wave"])), np.zeros(tot, dtype=LD)
        zero = np.zeros(tot)
        for q, a in (("x", x), ("y", y), ("flux", flux), ("dxdz", zero), ("dydz", zero), ("wavelength", wl.astype(np.float64)),
                     ("pupil_u", zero), ("pupil_v", zero), ("time", zero)):
            out[q].append(np.asarray(a, dtype=np.float64))
        wl_bound.append(wb + np.abs(wl - wl.astype(np.float64).astype(LD)))
        obj_index.append(np.full(tot, i, dtype=np.int32))
        ordinal.append(k)
        source.append(src)
        offset.append(offset[-1] + tot)
    cat = lambda a, dt: np.concatenate(a).astype(dt) if a else np.zeros(0, dtype=dt)
    return dict(fields={q: cat(out[q], np.float64) for q in ops_ref.FIELDS}, wl_bound=cat(wl_bound, LD), obj_index=cat(obj_index, np.int32),
                ordinal=cat(ordinal, np.int64), source=cat(source, np.int64), offset=np.asarray(offset, dtype=np.int64), n_per_pixel=n_pp)


def ops_objects(phot_rows, offset):
    """the photon rows as photon_ops_ref.apply wants them for the re-shot photons: photon number = ordinal (phot_first 0)"""
    o = np.array(phot_rows, copy=True)
    o["phot_first"] = 0
    o["n_phot"] = np.diff(offset)
    return o


def apply_ops(ops, blocks, phot_rows, made, loose=True):
    """photon_ops_ref.apply on the photons of make_photons: a photon_ops_ref.Result in pool order.  The wavelength is no planted
    field here but a table lookup: it keeps the bound photon_source_ref.lin_lookup gives it (no operator changes a wavelength; what
    that bound does to a DCR shift, 0.05 px / nm x 1e-13 nm, is a thousandth of the 8 EPS |x| the shift's own bound starts from)."""
    res = ops_ref.apply(ops, blocks, ops_objects(phot_rows, made["offset"]), made["fields"], loose=loose)
    res.bounds["wavelength"] = res.bounds["wavelength"] + made["wl_bound"]
    return res


def bin_photons(fft_rows, x, y, flux, obj_index):
    """The fixed-point binning.  Returns (out float64 [n_pix], sums int64 [n_pix], land int32 [n]: gy * nfft + gx or -1)"""
    n_pix = int(sum(int(o["nfft"]) ** 2 for o in fft_rows))
    sums = np.zeros(n_pix, dtype=np.int64)
    x, y, flux = (np.asarray(a, dtype=np.float64) for a in (x, y, flux))
    land = np.full(len(x), -1, dtype=np.int32)
    for i, o in enumerate(fft_rows):
        sel = np.flatnonzero(np.asarray(obj_index) == i)
        fx, fy = np.floor(x[sel] + 0.5), np.floor(y[sel] + 0.5)
        ok = ((flux[sel] != 0.0) & (fx >= o["stamp_xmin"]) & (fx <= o["stamp_xmax"]) & (fy >= o["stamp_ymin"]) & (fy <= o["stamp_ymax"]))
        gx = fx[ok].astype(np.int64) - int(o["x0"])
        gy = fy[ok].astype(np.int64) - int(o["y0"])
        at = gy * int(o["nfft"]) + gx
        land[sel[ok]] = at.astype(np.int32)
        np.add.at(sums, int(o["r_offset"]) + at, np.rint(flux[sel][ok] * Q32).astype(np.int64))
    return sums.astype(np.float64) * 2.0 ** -32, sums, land


def reshoot(fft_rows, phot_rows, values, seed, ops, blocks, sed_tables=None, max_flux=1.0):
    """the whole stage: (out, made, result of the operators)"""
    made = make_photons(fft_rows, phot_rows, values, seed, sed_tables, max_flux)
    res = apply_ops(ops, blocks, phot_rows, made)
    f = {q: res.fields[q].astype(np.float64) for q in ("x", "y", "flux")}
    out, _, _ = bin_photons(fft_rows, f["x"], f["y"], f["flux"], made["obj_index"])
    return out, made, res
