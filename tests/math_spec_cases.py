"""Inputs of the numerics spec's elementary functions (csrc/ims_math.h, oracle/orc_math.h), shared by the CPU accuracy tests
(test_math_spec.py: oracle against long double) and the GPU parity test (test_math_spec_gpu.py: device against oracle, bit
for bit).  Per function: random bulk over the range its callers can produce, every branch point of the evaluation with both
float64 neighbours, and out-of-domain points.  Deterministic; at most 2e5 points per function.

Each function has `NAME_in()` (the in-domain points: the accuracy bound is asserted on all of them) and `NAME_out()` (the
out-of-domain points: only device == oracle is asserted, and a few special values)."""
import math
from fractions import Fraction

import numpy as np

LN2 = math.log(2.0)
INV_LN2 = 1.44269504088896338700e+00        # the spec's constant
TAN_PI_8 = 0.41421356237309503              # atan's inner breakpoint, as written in the spec
INF, NAN = np.inf, np.nan
NEG_NAN = np.copysign(np.nan, -1.0)        # a NaN with the sign bit set: the sign of a NaN result is compared too


def nbrs(v):
    """v and both float64 neighbours"""
    v = np.float64(v)
    return [np.nextafter(v, -INF), v, np.nextafter(v, INF)]


def around(v, n):
    """v and n float64 neighbours on each side"""
    lo, hi, out = np.float64(v), np.float64(v), [np.float64(v)]
    for _ in range(n):
        lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
        out += [lo, hi]
    return sorted(out)


def _cat(*parts):
    return np.concatenate([np.atleast_1d(np.asarray(p, dtype=np.float64)).ravel() for p in parts])


# ---- exp ------------------------------------------------------------------------------------------------------------
def exp_k(x):
    """the spec's k = floor(fma(x, INV_LN2, 1/2)) of a finite x, in exact rational arithmetic rounded once as the fma does"""
    return math.floor(float(Fraction(float(x)) * Fraction(INV_LN2) + Fraction(1, 2)))


def exp_in():
    """Callers: Gaussian / Kolmogorov / Sersic profile values exp(-t), t in [0, 700) (ims_fft.h, sersic_edge_max); the
    extinction exp(k_av (a + b / rv) ln 10) of ims_sed.h, either sign, refused by the host beyond +-690; tanh's exp(-2 x),
    x in [0, 20]; pow's exp(y ln x) on [-40, 40].  In domain: -1000 <= k <= 1000."""
    rng = np.random.default_rng(101)
    ties = [t for k in (-1000, -999, -500, -2, -1, 0, 1, 2, 37, 999) for t in around((k + 0.5) * LN2, 2)]
    edges = [t for t in around(-1000.5 * LN2, 4) + around(1000.5 * LN2, 4)]
    pts = _cat([0.0, -0.0], nbrs(0.0), ties, edges, nbrs(LN2), nbrs(-LN2), [-693.0, 693.0])
    k = np.array([exp_k(v) for v in pts])
    return _cat(rng.uniform(-693.0, 693.0, 150000), rng.uniform(-1.0, 1.0, 20000), pts[(k >= -1000) & (k <= 1000)])


def exp_out():
    """the flushed side of the lower edge (k = -1001: exactly 0), the capped side of the upper one (k = 1001: finite, of
    unspecified magnitude), and the far field"""
    edges = np.array(around(-1000.5 * LN2, 4) + around(1000.5 * LN2, 4))
    k = np.array([exp_k(v) for v in edges])
    return _cat(edges[(k < -1000) | (k > 1000)], [-745.0, -1e5, -1e300, -INF, 700.0, 709.0, 1e5, 1e300, INF, NAN, NEG_NAN])


# ---- sin, cos of 2 pi u ---------------------------------------------------------------------------------------------
def sincos2pi_in():
    """Callers: the Box-Muller angle and the profile angle u in [0, 1) (ims_photon.h), dsincos's u - floor(u) in [0, 1]."""
    rng = np.random.default_rng(102)
    eighths = [t for k in range(9) for t in nbrs(k / 8.0)]
    u = _cat(rng.uniform(0.0, 1.0, 150000), eighths, [0.0, 1.0, 1e-300, 5e-324, np.nextafter(1.0, 0.0)])
    return u[(u >= 0.0) & (u <= 1.0)]


def sincos2pi_out():
    return _cat([-0.0, -5e-324, np.nextafter(1.0, 2.0), -0.25, 2.0, 5.3, 1.5e9, 3.0e9, -3.0e9, 1e300, -1e300, INF, -INF, NAN, NEG_NAN])


# ---- sin, cos of x --------------------------------------------------------------------------------------------------
def sincos_in():
    """Callers: kx * x of the FFT-stamp and knots structure factors (|x| up to 1e4: k <= pi per pixel times a stamp of a few
    thousand pixels), the spike and rotation angles (|x| <= 2 pi), the phase-screen kicks; |x| <= 1e6 is the stated domain."""
    rng = np.random.default_rng(103)
    bulk = [rng.uniform(-r, r, 40000) for r in (10.0, 1e2, 1e4, 1e6)]
    tiny = [-1e-17, -1e-20, -2.0 ** -54, -1e-300, -5e-324, 1e-17, 5e-324]           # u - floor(u) rounds to 1 for the negative ones
    halfpi = [t for k in list(range(-9, 10)) + [100, 1001, 65536, 636619, -636619] for t in nbrs(k * (np.pi / 2))]
    x = _cat(*bulk, tiny, halfpi, [0.0, -0.0, 1e6, -1e6])
    return x[np.abs(x) <= 1e6]


def sincos_out():
    return _cat([1e7, 1e15, 2.0 ** 53, 1e22, 1e300, -1e300, INF, -INF, NAN, NEG_NAN])


# ---- atan -----------------------------------------------------------------------------------------------------------
def atan_in():
    """Callers: atan2's y / x (any finite quotient), the spike profile datan((r +- 1/2) scale / r0) (1e-3 .. 1e5), the
    refraction term datan(1 / (2 k d)) (ims_photon.h).  In domain: every finite x and +-inf."""
    rng = np.random.default_rng(104)
    mag = 10.0 ** rng.uniform(-300.0, 300.0, 100000)
    sgn = np.where(rng.integers(0, 2, 100000) == 1, 1.0, -1.0)
    pts = [t for v in (1.0, TAN_PI_8, 1.0 + math.sqrt(2.0), 1.0 / TAN_PI_8) for t in nbrs(v)]
    return _cat(mag * sgn, rng.uniform(-5.0, 5.0, 60000), 10.0 ** rng.uniform(-6.0, -3.0, 20000),
                pts, [-p for p in pts], [0.0, -0.0, 5e-324, -5e-324, 1e300, -1e300, 1.7e308, INF, -INF])


def atan_out():
    return _cat([NAN, NEG_NAN])


# ---- atan2 (pairs y, x) ---------------------------------------------------------------------------------------------
def atan2_in():
    """Caller: the spike arms' datan2(y, x) of pixel offsets (ims_fft.h), |y|, |x| <= a few thousand, either may be 0.
    In domain: finite y and x whose quotient neither overflows nor underflows; the axes; (0, 0)."""
    rng = np.random.default_rng(105)
    n = 70000

    def signed(v):
        return v * np.where(rng.integers(0, 2, v.size) == 1, 1.0, -1.0)
    bulk = np.stack([_cat(signed(10.0 ** rng.uniform(-3.0, 3.0, n)), rng.uniform(-1.0, 1.0, n)),
                     _cat(signed(10.0 ** rng.uniform(-3.0, 3.0, n)), rng.uniform(-1.0, 1.0, n))], axis=1)
    grid = np.arange(-8.0, 9.0)
    pix = np.stack(np.meshgrid(grid, grid), axis=-1).reshape(-1, 2)                     # integer pixel offsets, (0, 0) among them
    axes = [(y, x) for y in (0.0, -0.0, 1.0, -1.0, 3.5, -3.5, 5e-324, -5e-324) for x in (0.0, -0.0)] + \
           [(y, x) for y in (0.0, -0.0) for x in (1.0, -1.0, 3.5, -3.5, 5e-324, -5e-324, 1e300, -1e300)]
    ratio = [(sy * 10.0 ** (e / 2.0), sx * 10.0 ** (-e / 2.0)) for e in range(-300, 301, 12) for sy in (1.0, -1.0) for sx in (1.0, -1.0)]
    ratio += [(sy * 10.0 ** e, sx) for e in (-300, -200, -17, -8, 8, 17, 200, 300) for sy in (1.0, -1.0) for sx in (1.0, -1.0)]
    diag = [(sy * v, sx) for v in nbrs(1.0) + nbrs(TAN_PI_8) + nbrs(1.0 + math.sqrt(2.0)) for sy in (1.0, -1.0) for sx in (1.0, -1.0)]
    return np.concatenate([bulk, pix, np.array(axes), np.array(ratio), np.array(diag)]).astype(np.float64)


def atan2_out():
    """a quotient that overflows or underflows, infinities and NaN"""
    return np.array([(1e300, 1e-300), (-1e300, 1e-300), (1e300, -1e-300), (1e-300, 1e300), (1e-300, -1e300), (-1e-300, -1e300),
                     (INF, 1.0), (-INF, 1.0), (INF, -1.0), (1.0, INF), (1.0, -INF), (-1.0, -INF), (INF, INF), (INF, -INF),
                     (NAN, 1.0), (1.0, NAN), (NAN, -1.0), (0.0, NAN), (NAN, 0.0), (NAN, NAN),
                     (NEG_NAN, 1.0), (NEG_NAN, -1.0), (1.0, NEG_NAN)], dtype=np.float64)


# ---- tanh, x >= 0 ---------------------------------------------------------------------------------------------------
def tanh_in():
    """Callers: the sensor's zfactor dtanh_pos(z / 12), conversion depth z in [0, 100] um -> [0, 8.4] (ims_photon.h,
    imsim_hip.hip).  In domain: x >= 0, +inf included."""
    rng = np.random.default_rng(106)
    return _cat(rng.uniform(0.0, 30.0, 50000), 10.0 ** rng.uniform(-20.0, 0.0, 50000), rng.uniform(0.0, 8.4, 20000),
                [0.0, 5e-324, 1e-300], nbrs(20.0), nbrs(0.5 * LN2), [30.0, 1e300, INF])


def tanh_out():
    return _cat([-0.0, -1e-3, -1.0, -30.0, -400.0, -INF, NAN, NEG_NAN])


# ---- pow (pairs x, y) -----------------------------------------------------------------------------------------------
def pow_in():
    """Callers: the chromatic PSF scaling (wl / base)^alpha, wl / base in [0.3, 3], alpha in [-1, 1] (ims_photon.h); the
    Kolmogorov k-space factor (k / k0)^(5/3), 1e-6 .. 1e4 (ims_fft.h); the Sersic profile r^(1/n), r in 1e-8 .. 1e3,
    n in 0.3 .. 6.2 (sersic_edge_max).  In domain: x > 0 normal, |y ln x| <= 690."""
    rng = np.random.default_rng(107)
    n = 50000
    a = np.stack([rng.uniform(0.3, 3.0, n), rng.uniform(-1.0, 1.0, n)], axis=1)
    b = np.stack([10.0 ** rng.uniform(-6.0, 4.0, n), np.full(n, 5.0 / 3.0)], axis=1)
    c = np.stack([10.0 ** rng.uniform(-8.0, 3.0, n), 1.0 / rng.uniform(0.3, 6.2, n)], axis=1)
    one = [(v, y) for v in nbrs(1.0) for y in (-1.0, -0.2, 0.0, 0.25, 5.0 / 3.0, 1.0 / 0.3)]
    y0 = [(x, y) for x in (1e-8, 0.3, 2.0, 1e4, 2.2250738585072014e-308, 1.7e308) for y in (0.0, -0.0)]
    more = [(2.0, 0.5), (2.0, 10.0), (0.5, 3.0), (10.0, -3.0), (1.4142135623730951, 2.0), (np.nextafter(1.4142135623730951, 2.0), 2.0)]
    return np.concatenate([a, b, c, np.array(one), np.array(y0), np.array(more)]).astype(np.float64)


def pow_zero():
    """x = 0 and a subnormal x: a record of what the spec's log gives there (it reads the exponent field alone, -1023)"""
    return np.array([(x, y) for x in (0.0, -0.0, 5e-324, 1e-310) for y in (0.0, 0.1, 0.5, 1.0, 5.0 / 3.0, -1.0)], dtype=np.float64)


def pow_out():
    return np.concatenate([pow_zero(), np.array([(-1.0, 2.0), (2.0, 2000.0), (2.0, -2000.0), (INF, 1.0), (2.0, INF), (2.0, -INF),
                                                 (NAN, 1.0), (2.0, NAN), (INF, 0.0), (NAN, 0.0), (NEG_NAN, 1.0), (2.0, NEG_NAN)])]).astype(np.float64)


# ---- division and square roots: the ends of their stated 2^+-500 range (the bulk is in test_lean_div_sqrt) ----------
def sqrt_ends():
    return _cat([t for v in (2.0 ** -500, 2.0 ** 500) for t in nbrs(v)], [2.0 ** -499, 2.0 ** 499, 3.0 * 2.0 ** -500, 1.5 * 2.0 ** 499])


def div_ends():
    """pairs (a, b) with |b| and |a / b| at the ends of 2^+-500"""
    ends = [2.0 ** -500, np.nextafter(2.0 ** -500, 1.0), 2.0 ** 500, np.nextafter(2.0 ** 500, 1.0), 3.0 * 2.0 ** -500, 1.5 * 2.0 ** 499]
    out = []
    for b in ends:
        for q in ends + [1.0, 1.0 / 3.0, 7.0]:
            a = q * b
            if 0.0 < abs(a) < INF and abs(a) >= 2.0 ** -1000:
                out += [(a, b), (-a, b), (a, -b)]
    return np.array(out, dtype=np.float64)
