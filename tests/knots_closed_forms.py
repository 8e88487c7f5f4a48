"""Closed forms for RandomKnots objects on the FFT branch that owe nothing to the library: numpy only.

A knots object is N delta functions of equal flux at the displacements d_m [arcsec along the pixel axes] from its centre.  Its spectrum
is the point source's times the structure factor S(k) = (1 / N) sum_m exp(-i k . d_m) (S_ref, the direct sum in extended precision);
through a round Gaussian PSF its image is a sum of separable erf pixel integrals (image_ref).  The conventions are those of
tests/fft_closed_forms.py: pixel (iy, ix) is the unit square centred on (ix, iy), the centre (cx, cy) is in those coordinates, ix runs
along x, the first component of d.

numpy_pipeline restates the branch (spectrum, structure factor, inverse transform) in numpy, so that the closed forms can be held
against each other on the host (tests/test_fft_knots.py) and a tolerance never has to come from the kernel."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def factor_bound(nfft):
    """Absolute bound on a double-precision structure factor on a grid of nfft: every term has modulus 1; its argument is at most
    pi nfft / 2 in magnitude (|d| <= nfft pixel_scale / 2, |k| <= pi / pixel_scale) and is formed with three roundings; the sine and
    cosine are good to a few eps absolutely; the mean of N such terms has the bound of one."""
    return 16.0 * EPS * (1.0 + math.pi * nfft / 2.0)


def S_ref(d, nfft, pixel_scale):
    """S(kx_j, ky_i) = (1 / N) sum_m exp(-i (kx_j dx_m + ky_i dy_m)) on the half-spectrum grid [nfft][nfft / 2 + 1]: dk = 2 pi /
    (nfft pixel_scale), kx = j dk, ky = (i < nfft / 2 ? i : i - nfft) dk.  The direct sum in np.longdouble; returns (re, im)."""
    L = np.longdouble
    d = np.asarray(d, dtype=np.float64).reshape(-1, 2)
    two_pi = L(8) * np.arctan(L(1))
    dk = two_pi / (L(nfft) * L(pixel_scale))
    j = np.arange(nfft // 2 + 1)
    i = np.arange(nfft)
    kx = j.astype(L) * dk
    ky = np.where(i < nfft // 2, i, i - nfft).astype(L) * dk
    re = np.zeros((nfft, nfft // 2 + 1), dtype=L)
    im = np.zeros((nfft, nfft // 2 + 1), dtype=L)
    for dx, dy in d:
        arg = ky[:, None] * L(dy) + kx[None, :] * L(dx)
        re += np.cos(arg)
        im -= np.sin(arg)
    return re / L(len(d)), im / L(len(d))


def _erf_axis(n, c, sigma_pix):
    root = math.sqrt(2.0) * sigma_pix
    return np.array([0.5 * (math.erf((i + 0.5 - c) / root) - math.erf((i - 0.5 - c) / root)) for i in range(n)])


def image_ref(nfft, cx, cy, d, sigma, pixel_scale, flux):
    """The knots through a round Gaussian PSF of `sigma` arcsec, integrated over every pixel of an nfft x nfft grid: pixel (y, x) is
    F / N sum_m 1/4 [erf((x + 1/2 - xm) / (sqrt 2 s)) - erf((x - 1/2 - xm) / (sqrt 2 s))] [the same in y], s = sigma / pixel_scale and
    (xm, ym) = (cx, cy) + d_m / pixel_scale.  NOT periodic (the grid of a DFT is): for knots far inside the grid."""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 2)
    s = sigma / pixel_scale
    out = np.zeros((nfft, nfft))
    for dx, dy in d:
        out += np.outer(_erf_axis(nfft, cy + dy / pixel_scale, s), _erf_axis(nfft, cx + dx / pixel_scale, s))
    return out * (flux / len(d))


def margin_in_sigmas(nfft, cx, cy, d, sigma, pixel_scale):
    """how far, in PSF sigmas, the knot nearest to an edge of the grid (the pixels' outer edges, -1/2 and nfft - 1/2) lies inside it"""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 2)
    x, y = cx + d[:, 0] / pixel_scale, cy + d[:, 1] / pixel_scale
    edge = min(x.min() + 0.5, nfft - 0.5 - x.max(), y.min() + 0.5, nfft - 0.5 - y.max())
    return edge * pixel_scale / sigma


def point_spectrum(nfft, cx, cy, sigma, pixel_scale, flux):
    """half spectrum of a point source through the Gaussian PSF and the pixel: flux exp(-sigma^2 k^2 / 2) sinc sinc exp(-i k . c s)"""
    dk = 2.0 * math.pi / (nfft * pixel_scale)
    j, i = np.arange(nfft // 2 + 1), np.arange(nfft)
    kx = (j * dk)[None, :]
    ky = (np.where(i < nfft // 2, i, i - nfft) * dk)[:, None]
    amp = flux * np.exp(-0.5 * sigma * sigma * (kx * kx + ky * ky)) * np.sinc(0.5 * kx * pixel_scale / math.pi) \
        * np.sinc(0.5 * ky * pixel_scale / math.pi)
    return amp * np.exp(-1j * (kx * cx + ky * cy) * pixel_scale)


def numpy_pipeline(nfft, cx, cy, d, sigma, pixel_scale, flux):
    """the branch restated: the point's half spectrum times S_ref, through numpy's inverse real transform"""
    re, im = S_ref(d, nfft, pixel_scale)
    spec = point_spectrum(nfft, cx, cy, sigma, pixel_scale, flux) * (re.astype(np.float64) + 1j * im.astype(np.float64))
    return np.fft.irfft2(spec, s=(nfft, nfft))
