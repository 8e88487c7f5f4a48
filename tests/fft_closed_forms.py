"""Host references of the FFT branch that owe nothing to the library or the oracle: closed forms of what
LSST_SiliconBuilder.draw's method 'fft' (imsim/stamp.py:482-525) must produce, and bounds on the two approximations the branch
makes on purpose.  Plain numpy, math.erf and Gauss-Legendre nodes.

Conventions (the ones the closed forms pin): pixel (iy, ix) of a grid is the unit square centred on the integer point (ix, iy);
an object's centre (cx, cy) is in those pixel coordinates; ix runs along x, the first coordinate of `jac`; a profile tabulated
as T(q) with `jac` = (j0, j1, j2, j3) and prof_scale = p is T(p |M^T k|), M = [[j0, j1], [j2, j3]] in arcsec -- the image of the
round unit profile under x = p M u.  The image of a DFT is periodic: the references wrap round the grid."""
import math

import numpy as np

from imsim_amd._abi import FFT_OBJECT_DTYPE

ALIAS_REACH = 8           # aliases |a|, |b| <= 8 enter the bound: a Gaussian MTF of sigma >= 0.05" is below 1e-38 beyond


def make_rows(specs):
    """FFT_OBJECT_DTYPE rows by hand.  specs: dicts with nfft, x0, y0, cx, cy, flux and optionally obj_id (default: the
    position in `specs`), prof_ktable (-1: a point source), prof_scale (1), jac (identity) and stamp = (xmin, xmax, ymin, ymax)
    (default: the whole grid).  Sorted by nfft (stable); k_offset / r_offset are the running sums of the half spectra and of the
    grids, as build_fft_objects leaves them."""
    specs = sorted(enumerate(specs), key=lambda t: int(t[1]["nfft"]))
    rows = np.zeros(len(specs), dtype=FFT_OBJECT_DTYPE)
    k_at = r_at = 0
    for r, (pos, s) in zip(rows, specs):
        n = int(s["nfft"])
        r["obj_id"] = s.get("obj_id", pos)
        r["flux"], r["nfft"] = s["flux"], n
        r["x0"], r["y0"], r["cx"], r["cy"] = s["x0"], s["y0"], s["cx"], s["cy"]
        r["prof_ktable"], r["prof_scale"] = s.get("prof_ktable", -1), s.get("prof_scale", 1.0)
        r["jac"] = s.get("jac", (1.0, 0.0, 0.0, 1.0))
        r["stamp_xmin"], r["stamp_xmax"], r["stamp_ymin"], r["stamp_ymax"] = s.get(
            "stamp", (s["x0"], s["x0"] + n - 1, s["y0"], s["y0"] + n - 1))
        r["k_offset"], r["r_offset"] = k_at, r_at
        k_at += n * (n // 2 + 1)
        r_at += n * n
    return rows


def shifted(rows, dx, dy):
    """the same rows on a CCD whose origin moved by (dx, dy): every pixel coordinate moves, nothing relative to the grid does"""
    out = rows.copy()
    for f in ("x0", "stamp_xmin", "stamp_xmax"):
        out[f] += dx
    for f in ("y0", "stamp_ymin", "stamp_ymax"):
        out[f] += dy
    return out


def grids(rows, rbuf):
    """the real-space buffer of a draw as one [nfft][nfft] view per row"""
    return [rbuf[int(o["r_offset"]):int(o["r_offset"]) + int(o["nfft"]) ** 2].reshape(int(o["nfft"]), int(o["nfft"])) for o in rows]


def _erf_axis(n, c, sigma_pix, wraps=3):
    """integral of the unit Gaussian centred on c over the pixels of one axis, summed over the periodic images of the grid"""
    out = np.zeros(n)
    root = math.sqrt(2.0) * sigma_pix
    for i in range(n):
        for p in range(-wraps, wraps + 1):
            x = i + p * n - c
            out[i] += 0.5 * (math.erf((x + 0.5) / root) - math.erf((x - 0.5) / root))
    return out


def erf_image(n, cx, cy, sigma_pix, flux):
    """A round Gaussian of `sigma_pix` pixels centred on (cx, cy), integrated over every pixel of an n x n grid: the image of a
    point source through a Gaussian PSF.  Summed over the wraps p, q in [-3, 3] of the grid."""
    return flux * np.outer(_erf_axis(n, cy, sigma_pix), _erf_axis(n, cx, sigma_pix))


def elliptical_gaussian_image(n, cx, cy, cov_arcsec2, flux, pixel_scale):
    """The Gaussian of covariance `cov_arcsec2` ([[xx, xy], [xy, yy]]) centred on (cx, cy), integrated over every pixel of an
    n x n grid by a 10-point Gauss-Legendre rule per axis.  Not wrapped: for grids the profile is far inside of."""
    cov = np.asarray(cov_arcsec2, dtype=np.float64) / (pixel_scale * pixel_scale)
    det = cov[0, 0] * cov[1, 1] - cov[0, 1] * cov[1, 0]
    ixx, ixy, iyy = cov[1, 1] / det, -cov[0, 1] / det, cov[0, 0] / det
    t, w = np.polynomial.legendre.leggauss(10)
    t, w = 0.5 * t, 0.5 * w                                         # nodes and weights on [-1/2, 1/2]
    x = (np.arange(n)[:, None] + t[None, :] - cx)[None, None, :, :]          # [1][1][ix][node]
    y = (np.arange(n)[:, None] + t[None, :] - cy)[:, :, None, None]          # [iy][node][1][1]
    dens = np.exp(-0.5 * (ixx * x * x + 2.0 * ixy * x * y + iyy * y * y)) / (2.0 * math.pi * math.sqrt(det))
    return flux * np.einsum("iajb,a,b->ij", dens, w, w)


def _grid_k(n, pixel_scale):
    """the signed frequencies of an n-point DFT axis [rad / arcsec]"""
    j = np.arange(n)
    return np.where(j < n // 2, j, j - n) * (2.0 * math.pi / (n * pixel_scale))


def _abs_sinc(k, pixel_scale):
    h = 0.5 * k * pixel_scale
    return np.abs(np.where(h == 0.0, 1.0, np.sin(h) / np.where(h == 0.0, 1.0, h)))


def _abs_spectrum(kx, ky, kpsf_sigma, pixel_scale):
    """|MTF(k) sinc(kx s / 2) sinc(ky s / 2)| of a unit point source through a Gaussian PSF, on the outer grid ky x kx"""
    gx = np.exp(-0.5 * kpsf_sigma ** 2 * kx * kx) * _abs_sinc(kx, pixel_scale)
    gy = np.exp(-0.5 * kpsf_sigma ** 2 * ky * ky) * _abs_sinc(ky, pixel_scale)
    return np.outer(gy, gx)


def omitted_alias_bound(kpsf_sigma, n, m, pixel_scale):
    """Per-pixel error, per unit flux, of folding only the aliases -m .. m of the sampling frequency into the spectrum.  The image
    sampled at the pixel centres has the continuous spectrum folded at 2 pi / s: every alias (a, b) left out is missing from the
    spectrum at each of the n^2 grid frequencies, and a pixel of the inverse DFT is 1 / n^2 times a sum of unit-modulus multiples of
    them:  (1 / n^2) sum_k sum_{(a, b) omitted, |a|, |b| <= 8} |MTF(k + (a, b) 2 pi / s) sinc sinc|.  (A profile factor is at most
    1 in modulus: the bound holds for galaxies too.)"""
    k = _grid_k(n, pixel_scale)
    ks = 2.0 * math.pi / pixel_scale
    total = 0.0
    for b in range(-ALIAS_REACH, ALIAS_REACH + 1):
        for a in range(-ALIAS_REACH, ALIAS_REACH + 1):
            if abs(a) <= m and abs(b) <= m:
                continue
            total += float(_abs_spectrum(k + a * ks, k + b * ks, kpsf_sigma, pixel_scale).sum())
    return total / (n * n)


def interp_bound(q_step, kpsf_sigma, n, pixel_scale):
    """Per-pixel error, per unit flux, of reading a profile exp(-q^2 / 2) from a table of step q_step by linear interpolation:
    the interpolant of f misses by at most q_step^2 / 8 max|f''|, and |f''| = |q^2 - 1| exp(-q^2 / 2) <= 1; every grid frequency
    carries that error times the rest of the spectrum:  (q_step^2 / 8) (1 / n^2) sum_k |MTF(k) sinc sinc|."""
    k = _grid_k(n, pixel_scale)
    return q_step * q_step / 8.0 * float(_abs_spectrum(k, k, kpsf_sigma, pixel_scale).sum()) / (n * n)


# ---------------------------------------------------------------------------------------------
# the cases the CPU test (oracle) and the GPU test (kernels) both hold to the closed forms
# ---------------------------------------------------------------------------------------------
PIXEL_SCALE = 0.2
POINT_SIGMAS = (0.5, 0.2, 0.12, 0.08)                         # arcsec; alias orders 0, 1, 1, 2
ALIAS_ORDERS = {0.5: 0, 0.2: 1, 0.12: 1, 0.08: 2}
POINT_GRIDS = ((32, 13.3, 17.8, 2.0e6, 10, 12),               # nfft, cx, cy, flux, x0, y0
               (32, 0.4, 31.2, 3.0e6, 60, 14),                # wraps round the grid's corner
               (96, 40.25, 50.5, 1.5e6, 110, 100))            # not a power of two


def point_rows():
    return make_rows([dict(nfft=n, cx=cx, cy=cy, flux=f, x0=x0, y0=y0) for n, cx, cy, f, x0, y0 in POINT_GRIDS])


def point_references(rows, sigma):
    return [erf_image(int(o["nfft"]), float(o["cx"]), float(o["cy"]), sigma / PIXEL_SCALE, float(o["flux"])) for o in rows]


SHEAR_JAC = (0.5, 0.2, -0.1, 0.35)
SHEAR_SIGMA = 0.3
SHEAR_GRID = (64, 30.3, 33.6)                                  # nfft, cx, cy
SHEAR_FLUX = (2.0e6, 3.0e6)


def shear_rows(prof_ktable=2):
    """the sheared Gaussian profile twice: as given, and with `jac` doubled and prof_scale halved -- the same image"""
    n, cx, cy = SHEAR_GRID
    return make_rows([dict(nfft=n, cx=cx, cy=cy, flux=SHEAR_FLUX[0], x0=20, y0=30, prof_ktable=prof_ktable, jac=SHEAR_JAC),
                      dict(nfft=n, cx=cx, cy=cy, flux=SHEAR_FLUX[1], x0=120, y0=130, prof_ktable=prof_ktable,
                           jac=tuple(2.0 * j for j in SHEAR_JAC), prof_scale=0.5)])


def shear_references(rows, transposed=False):
    """M M^T + sigma^2 I (transposed: M^T M, what acting with `jac` the wrong way round would give)"""
    M = np.array(SHEAR_JAC).reshape(2, 2)
    cov = (M.T @ M if transposed else M @ M.T) + SHEAR_SIGMA ** 2 * np.eye(2)
    n, cx, cy = SHEAR_GRID
    return [elliptical_gaussian_image(n, cx, cy, cov, float(o["flux"]), PIXEL_SCALE) for o in rows]
