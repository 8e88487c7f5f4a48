"""Host references for FFT-drawn streaks (galsim.Box on the FFT branch): plain numpy and math.erf, nothing of the library or the
oracle.  Conventions as in tests/fft_closed_forms.py: pixel (iy, ix) is the unit square centred on the integer point (ix, iy), an
object's centre (cx, cy) is in those coordinates, ix runs along x, the first coordinate of `jac`; the image of a DFT is periodic.

(a) `half_spectrum` / `image_a`: the whole spectrum restated -- profile factor (box: sinc(qx / 2) sinc(qy / 2) at q = J^T k; a point:
    1; a radial k-table: linear interpolation) x Gaussian MTF x pixel sinc x centring phase on the half grid -- and numpy.fft.irfft2.
(b) `image_b`: an axis-aligned box of L x W arcsec behind a Gaussian of sigma: flux F(x - cx; L) F(y - cy; W) with
    F(t; L) = [H(t + L/2 + s/2) - H(t + L/2 - s/2) - H(t - L/2 + s/2) + H(t - L/2 - s/2)] / L,  H(u) = u Phi(u / sigma) + sigma phi(u / sigma),
    summed over the periodic images of the grid (wraps -2 .. 2: the DFT's image is periodic, and on the grid of 32 a Gaussian tail
    of 1e-5 of the peak reaches the border).
(c) `moments` against `exact_moments`: sum = flux, centroid = (cx, cy), covariance = R diag(L^2 / 12, W^2 / 12) R^T + (sigma^2 + s^2 / 12) I.
    The moments of a periodic image are taken about the centre by the minimum-image convention; what (a) misses of (c) is the part of
    the Gaussian tail that wraps round the grid or is cut by it.

Residuals of (a) against (b) and (c) on the host at CASES (run from tests/, `python streak_closed_forms.py` prints them; numpy only), per unit flux for
(b) and the sum, in pixels / pixels^2 for centroid and covariance:
  (b), worst pixel, pa 0 and 90:            3.1e-12 of the flux (the aliases (a) leaves out: 2.7e-9 at Nyquist x the sincs)
  (c) |sum / flux - 1|:                     2.3e-16
  (c) centroid, grids of 32 / 64 [pixels]:  2.8e-5 / 1.1e-10   (32: 1.7" from the box's end to the border, 4.2 sigma)
  (c) covariance, grids of 32 / 64 [px^2]:  2.4e-5 / 2.4e-9
The largest is 2.8e-5.  These are the RESIDUAL_* constants at the end of this file; the tests allow four times each.
At LARGE_CASES (grids of 256 / 512, no axis-aligned case at pa 0; (b) from the pa 90 case): (b) 1.7e-13; sum 2.3e-16; centroid
2.3e-11 / 2.9e-13 pixels; covariance 2.3e-11 / 6.9e-12 pixels^2."""
import math

import numpy as np


PIXEL_SCALE = 0.2
SIGMA = 0.4                    # arcsec: the MTF at the Nyquist frequency is exp(-0.5 (0.4 pi / 0.2)^2) = 2.7e-9, no alias folding needed
PROF_BOX = -2                  # ims_fft_object_t.prof_ktable of a unit-flux box (IMS_PROF_BOX)


def box_jac(length, width, pa_deg):
    """the folded affine along the pixel axes (winv s = 1): R(pa) diag(length, width), row-major"""
    t = math.radians(pa_deg)
    c, s = math.cos(t), math.sin(t)
    return (c * length, -s * width, s * length, c * width)


# nfft, length, width [arcsec], position angle [deg], cx, cy [grid pixels], flux
CASES = (
    (32, 3.0, 0.6, 0.0, 16.0, 16.0, 2.0e6),          # integer centre
    (32, 3.0, 0.6, 90.0, 15.5, 16.5, 3.0e6),         # half-integer centre
    (32, 3.0, 0.6, 37.0, 15.37, 16.81, 1.5e6),       # arbitrary sub-pixel centre
    (32, 0.6, 0.6, 0.0, 16.3, 15.7, 2.5e6),          # a square
    (64, 3.0, 0.6, 0.0, 30.25, 33.6, 4.0e6),
    (64, 3.0, 0.6, 90.0, 32.0, 31.5, 1.0e6),
    (64, 3.0, 0.6, 37.0, 31.37, 32.81, 5.0e6),
    (64, 0.6, 0.6, 37.0, 33.5, 30.0, 2.0e6),         # the square, turned
)

# grids whose half spectra are wider than 64 columns -- the second level of the fill kernel's column tables -- with trails of 12" and
# 30" (what such grids are for): a centre off the pixel, a quarter turn on a pixel centre, and the 30 x 0.5" trail on 512
LARGE_CASES = (
    (256, 12.0, 0.5, 37.0, 127.37, 128.81, 3.0e6),
    (256, 12.0, 0.5, 90.0, 128.0, 127.0, 2.0e6),
    (512, 30.0, 0.5, 37.0, 255.3, 250.7, 5.0e7),
)


def box_specs(cases=CASES, origin=(4, 6)):
    """one box per case as the keyword sets of fft_closed_forms.make_rows, side by side on the CCD from `origin` on (the real-space
    buffer does not care where); also what half_spectrum / image_a take in place of a table row"""
    specs, x = [], origin[0]
    for n, L, W, pa, cx, cy, flux in cases:
        specs.append(dict(nfft=n, cx=cx, cy=cy, flux=flux, x0=x, y0=origin[1], prof_ktable=PROF_BOX, prof_scale=1.0,
                          jac=box_jac(L, W, pa)))
        x += n
    return specs


def box_rows(cases=CASES, origin=(4, 6)):
    """the same as FFT_OBJECT_DTYPE rows (this alone needs the package)"""
    import fft_closed_forms as cf
    return cf.make_rows(box_specs(cases, origin))


def _sinc(h):
    h = np.asarray(h, dtype=np.float64)
    safe = np.where(h == 0.0, 1.0, h)
    return np.where(h == 0.0, 1.0, np.sin(safe) / safe)


def profile_factor(o, kx, ky, ktables=None, q_step=None):
    """the profile's transform at q = J^T k: a box, a point, or a radial k-table read as the library reads it"""
    j = np.asarray(o["jac"], dtype=np.float64)
    qx = j[0] * kx + j[2] * ky
    qy = j[1] * kx + j[3] * ky
    t = int(o["prof_ktable"])
    if t == PROF_BOX:
        return _sinc(0.5 * qx) * _sinc(0.5 * qy)
    if t < 0:
        return np.ones(np.broadcast(kx, ky).shape)
    v = np.asarray(ktables[t], dtype=np.float64)
    f = np.sqrt(qx * qx + qy * qy) * float(o["prof_scale"]) / q_step
    i = np.minimum(f.astype(np.int64), len(v) - 2)
    val = v[i] + (f - i) * (v[i + 1] - v[i])
    return np.where(f > 0.0, np.where(f >= len(v) - 1, 0.0, val), v[0])


def half_spectrum(o, sigma=SIGMA, pixel_scale=PIXEL_SCALE, ktables=None, q_step=None):
    """(a): the half spectrum [nfft][nfft / 2 + 1] of one FFT_OBJECT_DTYPE row behind a Gaussian PSF of `sigma` arcsec"""
    n = int(o["nfft"])
    dk = 2.0 * math.pi / (n * pixel_scale)
    i = np.arange(n)
    ky = (np.where(i < n // 2, i, i - n) * dk)[:, None]
    kx = (np.arange(n // 2 + 1) * dk)[None, :]
    amp = float(o["flux"]) * profile_factor(o, kx, ky, ktables, q_step)
    amp = amp * np.exp(-0.5 * sigma * sigma * (kx * kx + ky * ky))
    amp = amp * _sinc(0.5 * kx * pixel_scale) * _sinc(0.5 * ky * pixel_scale)
    ph = (kx * float(o["cx"]) + ky * float(o["cy"])) * pixel_scale
    return amp * np.cos(ph) - 1j * amp * np.sin(ph)


def image_a(o, **kw):
    n = int(o["nfft"])
    return np.fft.irfft2(half_spectrum(o, **kw), s=(n, n))


def _Phi(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def _H(u, sigma):
    return u * _Phi(u / sigma) + sigma * math.exp(-0.5 * (u / sigma) ** 2) / math.sqrt(2.0 * math.pi)


def _F_axis(n, c, length, sigma, pixel_scale, wraps=2):
    out = np.zeros(n)
    s = pixel_scale
    for i in range(n):
        for p in range(-wraps, wraps + 1):
            t = (i + p * n - c) * s
            out[i] += (_H(t + 0.5 * length + 0.5 * s, sigma) - _H(t + 0.5 * length - 0.5 * s, sigma)
                       - _H(t - 0.5 * length + 0.5 * s, sigma) + _H(t - 0.5 * length - 0.5 * s, sigma)) / length
    return out


def image_b(n, cx, cy, len_x, len_y, flux, sigma=SIGMA, pixel_scale=PIXEL_SCALE):
    """(b): the box of len_x arcsec along x and len_y along y"""
    return flux * np.outer(_F_axis(n, cy, len_y, sigma, pixel_scale), _F_axis(n, cx, len_x, sigma, pixel_scale))


def moments(img, cx, cy):
    """(sum, centroid x, centroid y, [[xx, xy], [xy, yy]]) of a periodic image about (cx, cy), in pixels"""
    n = img.shape[0]
    d = np.arange(n, dtype=np.float64)
    dx = (d - cx + 0.5 * n) % n - 0.5 * n
    dy = (d - cy + 0.5 * n) % n - 0.5 * n
    total = float(img.sum())
    mx = float((img * dx[None, :]).sum()) / total
    my = float((img * dy[:, None]).sum()) / total
    xx = float((img * (dx[None, :] - mx) ** 2).sum()) / total
    yy = float((img * (dy[:, None] - my) ** 2).sum()) / total
    xy = float((img * (dx[None, :] - mx) * (dy[:, None] - my)).sum()) / total
    return total, cx + mx, cy + my, np.array([[xx, xy], [xy, yy]])


def exact_moments(length, width, pa_deg, sigma=SIGMA, pixel_scale=PIXEL_SCALE):
    """(c): the covariance in pixels^2"""
    t = math.radians(pa_deg)
    R = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
    cov = R @ np.diag([length ** 2 / 12.0, width ** 2 / 12.0]) @ R.T + (sigma ** 2 + pixel_scale ** 2 / 12.0) * np.eye(2)
    return cov / pixel_scale ** 2


def moment_errors(img, case):
    """(|sum / flux - 1|, centroid error [pixels], covariance error [pixels^2]) of one case's image"""
    n, L, W, pa, cx, cy, flux = case
    total, mx, my, cov = moments(img, cx, cy)
    return abs(total / flux - 1.0), max(abs(mx - cx), abs(my - cy)), float(np.abs(cov - exact_moments(L, W, pa)).max())


def image_b_of(case):
    n, L, W, pa, cx, cy, flux = case
    assert pa in (0.0, 90.0)
    return image_b(n, cx, cy, L if pa == 0.0 else W, W if pa == 0.0 else L, flux)


def host_residuals(cases=CASES):
    """(a) against (b) and (c) at `cases` -> (worst (b) per unit flux, worst sum, {nfft: centroid}, {nfft: covariance})"""
    rb, rs, rc, rv = 0.0, 0.0, {}, {}
    for o, case in zip(box_specs(cases), cases):
        n, L, W, pa, cx, cy, flux = case
        img = image_a(o)
        if pa in (0.0, 90.0):
            rb = max(rb, float(np.abs(img - image_b_of(case)).max()) / flux)
        es, ec, ev = moment_errors(img, case)
        rs = max(rs, es)
        rc[n] = max(rc.get(n, 0.0), ec)
        rv[n] = max(rv.get(n, 0.0), ev)
    return rb, rs, rc, rv


# what host_residuals() gave (numpy 2, x86-64); the tests allow four times each
RESIDUAL_B = 3.1e-12
RESIDUAL_SUM = 2.3e-16
RESIDUAL_CENTROID = {32: 2.8e-5, 64: 1.1e-10, 256: 2.3e-11, 512: 2.9e-13}
RESIDUAL_COV = {32: 2.4e-5, 64: 2.4e-9, 256: 2.3e-11, 512: 6.9e-12}
RESIDUAL_B_LARGE = 1.7e-13


if __name__ == "__main__":
    print(host_residuals())
    print(host_residuals(LARGE_CASES))
