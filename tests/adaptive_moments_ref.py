"""Adaptive moments restated in numpy, independent of the package (it is not imported): the iteration of ims_psf_adaptive on
plain (dx, dy, w) arrays, in np.longdouble with np.exp.

Per row the state is the centre (x0, y0) and the weight matrix (Mxx, Mxy, Myy).

Pass, over the photons with w != 0:
    u = dx - x0, v = dy - y0, det = Mxx Myy - Mxy^2, rho2 = (Myy u u - 2 Mxy u v + Mxx v v) / det, g = w exp(-rho2 / 2)
    A = sum g; Bx, By = sum g u, g v; Cxx, Cxy, Cyy = sum g u u, g u v, g v v; R = sum g rho2^2
Update:
    T = Mxx + Myy, D = sqrt((Mxx - Myy)^2 + 4 Mxy^2), a2 = (T + D) / 2, b2 = (T - D) / 2, s = sqrt(b2)
    ex = 2 Bx / (A s), ey = 2 By / (A s), exx = 4 (Cxx / A - Mxx / 2) / b2, exy and eyy likewise, each clipped to [-1/4, 1/4]
    conv = max |e.| sqrt(a2 / b2);  x0 += ex s, y0 += ey s, Mxx += exx b2, Mxy += exy b2, Myy += eyy b2;  iter += 1
Status: 0 converged (conv < tol after the update), 1 running or max_iter reached, 2 failed (A not finite or <= 0, or the new
matrix not finite or not positive definite: the state stays, iter is not advanced), 3 no photon arrived (NaN)."""
import numpy as np

LD = np.longdouble
CONVERGED, RUNNING, FAILED, EMPTY = 0, 1, 2, 3
FWHM_PER_SIGMA = 2.3548200450309493
NAMES = ("A", "Bx", "By", "Cxx", "Cxy", "Cyy", "R")


def pass_terms(dx, dy, w, state):
    """the seven per-photon terms [7][n_used] of the pass and rho2 [n_used], in longdouble, over the photons with w != 0"""
    ok = np.asarray(w) != 0
    dx, dy, w = np.asarray(dx)[ok].astype(LD), np.asarray(dy)[ok].astype(LD), np.asarray(w)[ok].astype(LD)
    x0, y0, mxx, mxy, myy = (LD(t) for t in state)
    u, v = dx - x0, dy - y0
    det = mxx * myy - mxy * mxy
    rho2 = (myy * u * u - 2 * mxy * u * v + mxx * v * v) / det
    g = w * np.exp(-rho2 / 2)
    return np.stack([g, g * u, g * v, g * u * u, g * u * v, g * v * v, g * rho2 * rho2]), rho2


def pass_sums(dx, dy, w, state):
    """(sums [7], sums of the absolute terms [7], used, dropped)"""
    t, _ = pass_terms(dx, dy, w, state)
    w = np.asarray(w)
    return t.sum(axis=1), np.abs(t).sum(axis=1), int((w != 0).sum()), int((w == 0).sum())


def clip(e):
    return LD(-0.25) if e < -0.25 else (LD(0.25) if e > 0.25 else e)


def update(state, sums):
    """one update of the weight: (new state, conv, rho4), or None when it fails"""
    x0, y0, mxx, mxy, myy = (LD(t) for t in state)
    A, Bx, By, Cxx, Cxy, Cyy, R = sums
    if not (np.isfinite(A) and A > 0):
        return None
    T = mxx + myy
    D = np.sqrt((mxx - myy) ** 2 + 4 * mxy * mxy)
    a2, b2 = (T + D) / 2, (T - D) / 2
    s = np.sqrt(b2)
    ex, ey = clip(2 * Bx / (A * s)), clip(2 * By / (A * s))
    exx, exy, eyy = clip(4 * (Cxx / A - mxx / 2) / b2), clip(4 * (Cxy / A - mxy / 2) / b2), clip(4 * (Cyy / A - myy / 2) / b2)
    conv = max(abs(ex), abs(ey), abs(exx), abs(exy), abs(eyy)) * np.sqrt(a2 / b2)
    nxx, nxy, nyy = mxx + exx * b2, mxy + exy * b2, myy + eyy * b2
    if not (np.isfinite(nxx) and np.isfinite(nxy) and np.isfinite(nyy) and nxx > 0 and nxx * nyy - nxy * nxy > 0):
        return None
    return (x0 + ex * s, y0 + ey * s, nxx, nxy, nyy), conv, R / A


def unweighted_start(dx, dy, w):
    """the default start: the unweighted centroid and M = (Ixx + Iyy) / 2 times the identity; None without a usable one"""
    ok = np.asarray(w) != 0
    if not ok.any():
        return None
    dx, dy, w = np.asarray(dx)[ok].astype(LD), np.asarray(dy)[ok].astype(LD), np.asarray(w)[ok].astype(LD)
    W = w.sum()
    xb, yb = (w * dx).sum() / W, (w * dy).sum() / W
    m = ((w * dx * dx).sum() / W - xb * xb + (w * dy * dy).sum() / W - yb * yb) / 2
    return (xb, yb, m, LD(0), m)


def iterate(dx, dy, w, start=None, tol=1e-6, max_iter=100):
    """The iteration from `start` (x0, y0, Mxx, Mxy, Myy; None: unweighted_start) -> dict of the reported quantities.  The values
    are longdouble; status and iter are ints."""
    w = np.asarray(w)
    used, dropped = int((w != 0).sum()), int((w == 0).sum())
    nan = LD(np.nan)
    out = dict(status=EMPTY, iter=0, xbar=nan, ybar=nan, Mxx=nan, Mxy=nan, Myy=nan, sigma=nan, e1=nan, e2=nan, rho4=nan, fwhm=nan,
               n_used=used, n_dropped=dropped, flux=w[w != 0].astype(LD).sum() if used else LD(0))
    if used == 0:
        return out
    state = unweighted_start(dx, dy, w) if start is None else tuple(LD(t) for t in start)
    status, it, rho4 = RUNNING, 0, nan
    if not (all(np.isfinite(t) for t in state) and state[2] > 0):
        status = FAILED
    while status == RUNNING and it < max_iter:
        sums = pass_sums(dx, dy, w, state)[0]
        step = update(state, sums)
        if step is None:
            status = FAILED
            break
        state, conv, rho4 = step
        it += 1
        if conv < tol:
            status = CONVERGED
    x0, y0, mxx, mxy, myy = state
    with np.errstate(invalid="ignore", divide="ignore"):
        sigma = np.sqrt(np.sqrt(mxx * myy - mxy * mxy))
        out.update(status=status, iter=it, xbar=x0, ybar=y0, Mxx=mxx, Mxy=mxy, Myy=myy, sigma=sigma, e1=(mxx - myy) / (mxx + myy),
                   e2=2 * mxy / (mxx + myy), rho4=rho4, fwhm=LD(FWHM_PER_SIGMA) * sigma)
    return out


def mixture_root(variances, fractions):
    """The adaptive M = m I of an isotropic mixture of Gaussians of variances s_i^2 and fractions f_i: the root m of
    sum_i f_i s_i^2 m^2 / (s_i^2 + m)^2 = (m / 2) sum_i f_i m / (s_i^2 + m), by bisection between the smallest and the largest
    variance (the product of component i with the weight is a Gaussian of variance s_i^2 m / (s_i^2 + m) and mass m / (s_i^2 + m))."""
    v, f = np.asarray(variances, dtype=LD), np.asarray(fractions, dtype=LD)

    def excess(m):
        return (f * v * m * m / (v + m) ** 2).sum() - (m / 2) * (f * m / (v + m)).sum()
    lo, hi = v.min(), v.max()                                  # excess(lo) >= 0 >= excess(hi): every term changes sign at m = s_i^2
    for _ in range(200):
        mid = (lo + hi) / 2
        if excess(mid) > 0:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2
