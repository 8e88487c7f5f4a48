"""numpy restatement of the optical phase screen's device functions (imsim_amd/csrc/ims_optical.h), operation by operation in
the order include/imsim_hip.h documents (ims_optical_screen_t).  Written from that description, not from the kernel source.

numpy has no fused multiply-add.  The per-object part (field angle -> 19 coefficients -> 28 pupil monomials -> 2 x 21 gradient
coefficients) is specified with separate rounded products and sums and is restated with plain numpy arithmetic.  The per-photon
part (two Horner evaluations of degree 5) is specified with fma steps: they are emulated EXACTLY here -- a * b + c in rational
arithmetic (fractions.Fraction of the three doubles), rounded once by float(), which rounds a Fraction correctly to nearest even.
"""
from fractions import Fraction

import numpy as np

DEG_PER_RAD = 57.29577951308232
NZ, NFIELD, NPUPIL = 19, 15, 28


def row(deg, q):
    return q * (deg + 1) - q * (q - 1) // 2


def fma(a, b, c):
    """elementwise fma of three f64 arrays, exactly rounded"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    out = np.empty(a.shape)
    fa, fb, fc, fo = a.ravel(), b.ravel(), c.ravel(), out.ravel()
    for i in range(fa.size):
        fo[i] = float(Fraction(float(fa[i])) * Fraction(float(fb[i])) + Fraction(float(fc[i])))
    return out


def poly_plain(c, deg, x, y):
    """c: [..., n_monomials]; rows by Horner in x from the highest power, then Horner in y; separate * and +"""
    acc = None
    for q in range(deg, -1, -1):
        s = c[..., row(deg, q) + (deg - q)]
        for p in range(deg - q - 1, -1, -1):
            s = s * x + c[..., row(deg, q) + p]
        acc = s if q == deg else acc * y + s
    return acc


def poly_fma(c, deg, x, y):
    acc = None
    for q in range(deg, -1, -1):
        s = c[..., row(deg, q) + (deg - q)]
        for p in range(deg - q - 1, -1, -1):
            s = fma(s, x, c[..., row(deg, q) + p])
        acc = s if q == deg else fma(acc, y, s)
    return acc


def coefficients(field, remap, atm_tan_x, atm_tan_y):
    """a [n, 19] at the objects' field angles [rad]"""
    thx = (np.asarray(atm_tan_x, dtype=np.float64) * DEG_PER_RAD) * remap
    thy = (np.asarray(atm_tan_y, dtype=np.float64) * DEG_PER_RAD) * remap
    return np.stack([poly_plain(field[j], 4, thx, thy) for j in range(NZ)], axis=-1)


def gradient_coefficients(pupil, a):
    """(gx [n, 21], gy [n, 21]) from a [n, 19]: w_t = a_0 pupil[0][t], + a_j pupil[j][t] in order; then (double)p w, (double)q w"""
    n = a.shape[0]
    gx, gy = np.zeros((n, 21)), np.zeros((n, 21))
    for q in range(7):
        for p in range(7 - q):
            t = row(6, q) + p
            w = a[:, 0] * pupil[0, t]
            for j in range(1, NZ):
                w = w + a[:, j] * pupil[j, t]
            if p >= 1:
                gx[:, row(5, q) + (p - 1)] = float(p) * w
            if q >= 1:
                gy[:, row(5, q - 1) + p] = float(q) * w
    return gx, gy


def gradient(gx, gy, inv_r, grad_scale, u, v):
    """(dW/du, dW/dv) [nm/m]"""
    x, y = np.asarray(u, dtype=np.float64) * inv_r, np.asarray(v, dtype=np.float64) * inv_r
    return grad_scale * poly_fma(gx, 5, x, y), grad_scale * poly_fma(gy, 5, x, y)


def screen_arrays(S):
    """(field [19, 15], pupil [19, 28]) of an _abi.OpticalScreen"""
    field = np.array([[S.field[j][t] for t in range(NFIELD)] for j in range(NZ)])
    pupil = np.array([[S.pupil[j][t] for t in range(NPUPIL)] for j in range(NZ)])
    return field, pupil


def evaluate(S, atm_tan_x, atm_tan_y, u, v):
    """what ims_test_optical_screen returns: (coef [n, 19], dwdu [n], dwdv [n])"""
    field, pupil = screen_arrays(S)
    a = coefficients(field, S.remap, atm_tan_x, atm_tan_y)
    gx, gy = gradient_coefficients(pupil, a)
    du, dv = gradient(gx, gy, S.inv_r, S.grad_scale, u, v)
    return a, du, dv


# ---------------- textbook forms, independent of the product's expansion code ----------------
def noll_nm(j):
    n = 0
    while (n + 1) * (n + 2) // 2 < j:
        n += 1
    k = j - n * (n + 1) // 2                      # 1 .. n + 1 within the order
    m = (n % 2) + 2 * ((k - 1 + ((n + 1) % 2)) // 2)
    return n, (m if j % 2 == 0 else -m)


def circular_zernike(j, x, y):
    """Noll Z_j on the unit disk, unit rms (Noll 1976): sqrt(n + 1) R_n^m(rho) {1, sqrt 2 cos m t, sqrt 2 sin m t}"""
    from math import factorial as f
    n, m = noll_nm(j)
    am = abs(m)
    rho, th = np.hypot(x, y), np.arctan2(y, x)
    R = sum((-1) ** k * f(n - k) / (f(k) * f((n + am) // 2 - k) * f((n - am) // 2 - k)) * rho ** (n - 2 * k)
            for k in range((n - am) // 2 + 1))
    ang = 1.0 if m == 0 else np.sqrt(2.0) * (np.cos(am * th) if m > 0 else np.sin(am * th))
    return np.sqrt(n + 1.0) * R * ang


def annular_zernike(j, x, y, eps):
    """Noll Z_j orthonormal over the annulus eps <= rho <= 1 (Mahajan 1981), built here from scratch: the radial polynomial of
    (n, |m|) is rho^|m|, rho^(|m|+2), ..., rho^n orthogonalised in that order by Gram-Schmidt under the area weight (Gauss-Legendre
    in rho^2, exact for these degrees), scaled to unit mean square with the angular factor, positive at rho = 1."""
    n, m = noll_nm(j)
    am = abs(m)
    node, wt = np.polynomial.legendre.leggauss(16)
    s = 0.5 * (1.0 - eps * eps) * node + 0.5 * (1.0 + eps * eps)        # rho^2 over [eps^2, 1], uniform = the area measure
    w = 0.5 * wt
    q = np.sqrt(s)
    val = lambda cc: sum(cc[i] * q ** (am + 2 * i) for i in range(len(cc)))
    basis = []                                                          # each: coefficients of rho^am, rho^(am+2), ...
    for k in range((n - am) // 2 + 1):
        c = np.zeros((n - am) // 2 + 1)
        c[k] = 1.0
        for b in basis:
            c = c - (w * val(c) * val(b)).sum() / (w * val(b) * val(b)).sum() * b
        basis.append(c)
    c = basis[-1]
    c = c / np.sqrt((w * val(c) ** 2).sum()) * (1.0 if c.sum() > 0 else -1.0)
    rho, th = np.hypot(x, y), np.arctan2(y, x)
    R = sum(c[i] * rho ** (am + 2 * i) for i in range(len(c)))
    ang = 1.0 if m == 0 else np.sqrt(2.0) * (np.cos(am * th) if m > 0 else np.sin(am * th))
    return R * ang
