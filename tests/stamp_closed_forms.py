"""Closed forms for FITS-stamp objects (galsim.InterpolatedImage) on the FFT branch that owe nothing to the library: numpy only.

A stamp object is a lattice of interpolant kernels: pixel (a, b) of a w x h stamp of pixel scale p, of weight w_m (the non-negative
pixels normalised to sum 1, row-major), sits at d_m = J' (p (a + 1/2 - w / 2), p (b + 1/2 - h / 2)) [arcsec along the CCD's pixel axes]
and carries the separable kernel K(u / p) K(v / p) / p^2 along the stamp's own axes.  Its spectrum is therefore

    F(k) = [ sum_m w_m exp(-i k . d_m) ] Qhat(q_u p / 2 pi) Qhat(q_v p / 2 pi),      q = J'^T k,

with Qhat(u) = integral K(x) cos(2 pi u x) dx (quintic_hat: the closed form of the piecewise quintic; sinc for the nearest
interpolant).  F_ref is that sum in np.longdouble.  Through a round Gaussian PSF and with J' the identity the image is separable:
axis_integral is the integral over every CCD pixel of (K of width p) convolved with (the Gaussian), by Gauss-Legendre quadrature in
np.longdouble; image_ref sums it over the stamp's pixels.  The conventions are those of tests/fft_closed_forms.py: pixel (iy, ix) is
the unit square centred on (ix, iy), the centre (cx, cy) is in those coordinates.

numpy_pipeline restates the branch (point spectrum, F, inverse transform) in numpy, so that the closed forms can be held against each
other on the host (tests/test_fft_stamps.py) and a tolerance never has to come from the kernel."""
import math

import numpy as np

L = np.longdouble
EPS = float(np.finfo(np.float64).eps)
PI = L(4) * np.arctan(L(1))


def quintic_kernel(x):
    """GalSim's Quintic interpolant (Bernstein & Gruen 2014) restated in np.longdouble: the piecewise quintic on [-3, 3]"""
    x = np.abs(np.asarray(x, dtype=L))
    a = L(1) + x ** 3 * (L(-95) + L(138) * x - L(55) * x * x) / L(12)
    b = (x - 1) * (x - 2) * (L(-138) + L(348) * x - L(249) * x * x + L(55) * x ** 3) / L(24)
    c = (x - 2) * (x - 3) ** 2 * (L(-54) + L(50) * x - L(11) * x * x) / L(24)
    return np.where(x <= 1, a, np.where(x <= 2, b, np.where(x <= 3, c, L(0))))


def _sinc(u):
    u = np.asarray(u, dtype=L)
    x = PI * u
    safe = np.where(x == 0, L(1), x)
    return np.where(x == 0, L(1), np.sin(safe) / safe)


def quintic_hat(u):
    """Qhat(u) = s^5 (s (55 - 19 x^2) + 2 cos(x) (x^2 - 27)), x = pi u, s = sin(x) / x: the transform of quintic_kernel at u cycles
    per pixel, in np.longdouble.  tests/test_fft_stamps.py holds it to the quadrature of the kernel."""
    u = np.asarray(u, dtype=L)
    x = PI * u
    s = _sinc(u)
    return s ** 5 * (s * (L(55) - L(19) * x * x) + L(2) * np.cos(x) * (x * x - L(27)))


def nearest_hat(u):
    """transform of the unit box (the nearest interpolant: a photon lands uniformly inside its pixel)"""
    return _sinc(u)


def gauss_legendre_hat(kernel, u, nodes=32, support=3):
    """integral of kernel(x) cos(2 pi u x) over [-support, support], piece by piece between the integers, with `nodes` Gauss-Legendre
    nodes per piece, in the precision the kernel returns"""
    gx, gw = np.polynomial.legendre.leggauss(nodes)
    total = 0.0
    for a in range(-support, support):
        x = a + 0.5 + 0.5 * gx
        total = total + 0.5 * np.sum(gw * kernel(x) * np.cos(2.0 * math.pi * u * x))
    return total


def stamp_pixels(img):
    """(a, b, w) of the positive pixels of a stamp [h][w], row-major, w normalised to sum 1 over them"""
    v = np.clip(np.asarray(img, dtype=np.float64), 0.0, None)
    b, a = np.nonzero(v > 0.0)
    return a, b, v[b, a] / v.sum()


def pixel_centres(img, p, jac):
    """d_m [N][2] in np.longdouble, and the weights"""
    h, w = np.asarray(img).shape
    a, b, wt = stamp_pixels(img)
    gx = L(p) * (a.astype(L) + L(0.5) - L(w) / 2)
    gy = L(p) * (b.astype(L) + L(0.5) - L(h) / 2)
    j = [L(float(v)) for v in jac]
    return np.stack([j[0] * gx + j[1] * gy, j[2] * gx + j[3] * gy], axis=1), wt


def extent(img, p, jac):
    """largest |d_m| component: the premise of factor_bound (a stamp inside half the grid)"""
    d, _ = pixel_centres(img, p, jac)
    return float(np.abs(d).max())


def grid_k(nfft, pixel_scale):
    dk = 2 * PI / (L(nfft) * L(pixel_scale))
    j, i = np.arange(nfft // 2 + 1), np.arange(nfft)
    return j.astype(L) * dk, np.where(i < nfft // 2, i, i - nfft).astype(L) * dk


def F_ref(img, p, jac, nfft, pixel_scale, interpolant="quintic"):
    """F on the half-spectrum grid [nfft][nfft / 2 + 1] (dk = 2 pi / (nfft pixel_scale), kx = j dk, ky = (i < nfft / 2 ? i : i - nfft)
    dk): the direct sum in np.longdouble; returns (re, im)."""
    d, wt = pixel_centres(img, p, jac)
    kx, ky = grid_k(nfft, pixel_scale)
    re = np.zeros((nfft, nfft // 2 + 1), dtype=L)
    im = np.zeros((nfft, nfft // 2 + 1), dtype=L)
    for (dx, dy), w in zip(d, wt):
        arg = ky[:, None] * dy + kx[None, :] * dx
        re += L(float(w)) * np.cos(arg)
        im -= L(float(w)) * np.sin(arg)
    j = [L(float(v)) for v in jac]
    qu = j[0] * kx[None, :] + j[2] * ky[:, None]
    qv = j[1] * kx[None, :] + j[3] * ky[:, None]
    hat = quintic_hat if interpolant == "quintic" else nearest_hat
    q = hat(qu * L(p) / (2 * PI)) * hat(qv * L(p) / (2 * PI))
    return re * q, im * q


def factor_bound(nfft):
    """tests/knots_closed_forms.py's bound for the same accumulation -- every term's argument is at most pi nfft / 2 in magnitude and
    formed with three roundings, the sine and cosine are good to a few eps absolutely -- with sum |w_m| = 1 in place of N x (1 / N):
    a weighted mean of such terms has the bound of one.  The interpolant's factor is at most 1 in modulus."""
    return 16.0 * EPS * (1.0 + math.pi * nfft / 2.0)


def axis_integral(n, c, p, sigma, pixel_scale, nodes=32):
    """I(i), i = 0 .. n - 1: the integral over the pixel [i - 1/2, i + 1/2] of (K(x / p) / p) convolved with (the Gaussian of `sigma`),
    centred on c [pixels]; p, sigma in arcsec.  I(i) = int K(t) int_pixel G(x s - c s - p t) s dx dt: Gauss-Legendre in t piece by
    piece between the integers of [-3, 3] and in x over the pixel, `nodes` nodes each, in np.longdouble.  NOT periodic."""
    gx, gw = np.polynomial.legendre.leggauss(nodes)
    gx, gw = gx.astype(L), gw.astype(L)
    t = np.concatenate([a + L(0.5) + L(0.5) * gx for a in range(-3, 3)])          # [6 nodes]
    tw = np.concatenate([L(0.5) * gw for _ in range(6)]) * quintic_kernel(t)
    x = (np.arange(n).astype(L)[:, None] + L(0.5) * gx[None, :] - L(c)) * L(pixel_scale)      # [pixel][node], arcsec from the centre
    xw = L(0.5) * gw * L(pixel_scale)
    z = (x[:, :, None] - L(p) * t[None, None, :]) / L(sigma)
    g = np.exp(L(-0.5) * z * z) / (np.sqrt(2 * PI) * L(sigma))
    return np.einsum("ijk,j,k->i", g, xw, tw)


def image_ref(nfft, cx, cy, img, p, sigma, pixel_scale, flux):
    """the stamp with J' the identity through a round Gaussian PSF, integrated over every pixel of an nfft x nfft grid:
    F sum_m w_m I_y(iy; cy + dy_m) I_x(ix; cx + dx_m).  Not periodic: for stamps far inside the grid.  np.longdouble."""
    d, wt = pixel_centres(img, p, (1.0, 0.0, 0.0, 1.0))
    out = np.zeros((nfft, nfft), dtype=L)
    for (dx, dy), w in zip(d, wt):
        out += L(float(w)) * np.outer(axis_integral(nfft, L(cy) + dy / L(pixel_scale), p, sigma, pixel_scale),
                                      axis_integral(nfft, L(cx) + dx / L(pixel_scale), p, sigma, pixel_scale))
    return out * L(flux)


def wrap_bound(nfft, cx, cy, img, p, sigma, pixel_scale):
    """Per unit flux: what the periodic images of the grid add to a pixel at most.  A periodic image of the object is at least one
    grid away; seen from any pixel of the grid it lies beyond r = (the distance of the nearest kernel's support from the nearest
    grid edge).  The mass of a 1-D Gaussian beyond r, times the kernel's absolute mass per axis (1.2587), times the 8 nearest images,
    bounds it; the further ones are smaller still."""
    d, _ = pixel_centres(img, p, (1.0, 0.0, 0.0, 1.0))
    x = float(cx) + d[:, 0].astype(np.float64) / pixel_scale
    y = float(cy) + d[:, 1].astype(np.float64) / pixel_scale
    reach = 3.0 * p / pixel_scale
    edge = min(x.min() + 0.5, nfft - 0.5 - x.max(), y.min() + 0.5, nfft - 0.5 - y.max()) - reach
    assert edge > 0.0
    return 8.0 * 1.2587 ** 2 * math.erfc(edge * pixel_scale / (math.sqrt(2.0) * sigma))


def point_spectrum(nfft, cx, cy, sigma, pixel_scale, flux):
    """half spectrum of a point source through the Gaussian PSF and the pixel: flux exp(-sigma^2 k^2 / 2) sinc sinc exp(-i k . c s)"""
    dk = 2.0 * math.pi / (nfft * pixel_scale)
    j, i = np.arange(nfft // 2 + 1), np.arange(nfft)
    kx = (j * dk)[None, :]
    ky = (np.where(i < nfft // 2, i, i - nfft) * dk)[:, None]
    amp = flux * np.exp(-0.5 * sigma * sigma * (kx * kx + ky * ky)) * np.sinc(0.5 * kx * pixel_scale / math.pi) \
        * np.sinc(0.5 * ky * pixel_scale / math.pi)
    return amp * np.exp(-1j * (kx * cx + ky * cy) * pixel_scale)


def numpy_pipeline(nfft, cx, cy, img, p, jac, sigma, pixel_scale, flux, interpolant="quintic"):
    """the branch restated: the point's half spectrum times F_ref, through numpy's inverse real transform"""
    re, im = F_ref(img, p, jac, nfft, pixel_scale, interpolant)
    spec = point_spectrum(nfft, cx, cy, sigma, pixel_scale, flux) * (re.astype(np.float64) + 1j * im.astype(np.float64))
    return np.fft.irfft2(spec, s=(nfft, nfft))


def footprint_pixels(img, p, jac, pixel_scale):
    """area of the stamp's parallelogram on the CCD, in CCD pixels"""
    h, w = np.asarray(img).shape
    return w * h * p * p * abs(jac[0] * jac[3] - jac[1] * jac[2]) / (pixel_scale * pixel_scale)


# ---------------------------------------------------------------------------------------------
# the stamps the CPU test (numpy restatement) and the GPU test (kernel) both hold to the closed forms
# ---------------------------------------------------------------------------------------------
PIXEL_SCALE = 0.2
JACS = ((1.0, 0.0, 0.0, 1.0), (0.9, 0.35, -0.3, 0.8))         # the identity; sheared and rotated, determinant 0.825


def factor_stamps():
    """(name, stamp [h][w], pixel scale): one pixel (pure Qhat Qhat and a half-pixel phase: the centre of a 1 x 1 stamp is the object's,
    so the 3 x 5 case carries the half-pixel offsets); 3 x 5 with a zero and a negative pixel (non-square, compacted list of 13); 9 x 8 =
    72 positive pixels (two chunks of 32 and a remainder of 8); 6 x 6 with three pixels out = 33 (a chunk and one)."""
    rng = np.random.default_rng(20261020)
    one = np.array([[2.5]])
    s35 = rng.uniform(0.5, 3.0, size=(3, 5))
    s35[1, 2], s35[2, 4] = 0.0, -1.5
    s98 = rng.uniform(0.2, 4.0, size=(9, 8))
    s33 = rng.uniform(0.2, 4.0, size=(6, 6))
    s33[0, 0], s33[3, 4], s33[5, 5] = -0.7, 0.0, 0.0
    assert (s35 > 0).sum() == 13 and (s98 > 0).sum() == 72 and (s33 > 0).sum() == 33
    return (("1x1", one, 0.27), ("3x5", s35, 0.23), ("9x8", s98, 0.17), ("33", s33, 0.31))
