"""The numerics spec's elementary functions (oracle/orc_math.h, the CPU statement of csrc/ims_math.h) against long double,
each held to a bound derived from its evaluation scheme.  u = 2^-53 throughout (half an ulp of a number in [1, 2)); "half-ulp
of [a, b)" is the largest rounding error of a result in that binade.  The inputs are those of tests/math_spec_cases.py, which
the GPU test (test_math_spec_gpu.py) sends through the device and compares with the oracle bit for bit -- together the two
files hold the device to these bounds.  The long-double reference itself is good to 2^-63 relative, 1e-3 u."""
import math

import numpy as np
import pytest

import math_spec_cases as mc
from oracle import orc_loader

U = 2.0 ** -53
LD = np.longdouble
PI_L = 4 * np.arctan(LD(1))                    # pi to long double


def _report(name, err, bound):
    ratio = float(np.max(err / bound))
    print(f"{name}: worst error / bound {ratio:.3f}")
    return ratio


def test_exp_is_good_to_two_u():
    """|exp - e^x| <= 2 u e^x for every x with -1000 <= k <= 1000, k = floor(x / ln 2 + 1/2) (that is -693.49 < x < 693.49).
    r = x - k LN2_HI - k LN2_LO: the first fma is exact (LN2_HI has 21 significant bits and |k| < 2^10, so k LN2_HI is exact; the
    difference of two numbers that close is a multiple of 2^-54 below 1/2, or r = x when k = 0); the second rounds a number below
    0.347 (half-ulp of [1/4, 1/2): u / 4); LN2_HI + LN2_LO misses ln 2 by at most half an ulp of LN2_LO, 2^-86, times |k| <= 1000:
    1e-7 u.  exp has unit slope, so the reduction costs 0.2501 u relative.  The series stops after r^13 / 13!: the rest is below
    0.3466^14 / 14! x 1.03 = 4.3e-18, against e^r >= 0.707: 0.054 u.  Horner: the accumulators before the last three steps are
    1/6 + ... (rounding u / 8, the rounded 1/6 another u / 8, what they inherit 0.02 u: 0.27 u), then 1/2 + ... (u / 2 + 0.347 x
    0.27 u = 0.6 u), then p2 = (e^r - 1) / r <= 1.2 (u + 0.347 x 0.6 u = 1.21 u); the last fma gives 1 + r p2 with |r| 1.21 u
    <= 0.42 u against a result of at least 0.707 (0.593 u relative) and its own rounding (u relative).  The scale 2^k is exact and
    the result normal (0.707 x 2^-1000).  Sum: 0.2501 + 0.054 + 0.593 + 1 = 1.9 u.
    Measured: worst error / bound 0.595."""
    x = mc.exp_in()
    want = np.exp(x.astype(LD))
    err = np.abs(orc_loader.math_probe(1, x).astype(LD) - want)
    bound = 2.0 * U * want
    _report("exp", err, bound)
    assert np.all(err <= bound)


def _sincos2pi_ref(u):
    """sin, cos of 2 pi u for u in [0, 1]: u - q / 4 is exact in float64 (q = nearest quarter turn), the rest in long double"""
    q = np.floor(4.0 * u + 0.5)
    r = (u - 0.25 * q).astype(LD)                           # exact: a multiple of ulp(u) no larger than u
    t = r * (2 * PI_L)
    s, c = np.sin(t), np.cos(t)
    qi = q.astype(np.int64) & 3
    return (np.choose(qi, [s, c, -s, -c]), np.choose(qi, [c, -s, -c, s]))


def test_sincos2pi_is_good_to_1p6_u_absolute():
    """|sin - sin 2 pi u|, |cos - cos 2 pi u| <= 1.6 u for u in [0, 1].  q = floor(4 u + 1/2) and r = u - q / 4 are exact (r is a
    multiple of ulp(u) no larger than u), |r| <= 1/8.  t = r TWO_PI: the product rounds (|t| <= 0.7854, half-ulp of [1/2, 1):
    u / 2) and TWO_PI misses 2 pi by 2.45e-16 = 0.351 u relative (0.276 u of t): t is off by 0.776 u, which sin passes on with slope
    <= 1 and cos with slope <= sin(pi / 4) (0.55 u).  Sine kernel t + t^3 p: z = t^2 and t z carry u and 2 u relative, p = -1/6 + ...
    0.26 u absolute (its last rounding u / 8, the rounded 1/6 u / 8, the rest 0.01 u), 1.6 u relative; the term t^3 p <= 0.0807 is
    good to 3.6 u relative, 0.29 u; the last fma rounds a result below 0.7072 (u / 2); t^19 / 19! = 8e-20.  Sine: 0.776 + 0.29 +
    0.5 = 1.57 u.  Cosine kernel 1 + z p: p = -1/2 + ... 0.32 u (rounding u / 4, inherited 0.04 u, z's error through slope 1/24
    0.026 u); z p <= 0.3085 carries z's u (0.3085 u) and p's error times z (0.197 u); the last rounding u / 2 (result in [0.707, 1]).
    Cosine: 0.55 + 1.006 = 1.56 u.  The quadrant is a swap and exact negations.
    Measured: worst error / bound 0.817."""
    u = mc.sincos2pi_in()
    got = orc_loader.math_probe(2, u).reshape(-1, 2).astype(LD)
    s, c = _sincos2pi_ref(u)
    err = np.maximum(np.abs(got[:, 0] - s), np.abs(got[:, 1] - c))
    _report("sincos2pi", err, np.full(u.size, 1.6 * U, dtype=LD))
    assert np.all(err <= 1.6 * U)
    # the pair stays on the unit circle to the same accuracy
    assert float(np.max(np.abs(got[:, 0] ** 2 + got[:, 1] ** 2 - 1))) <= 2 * 1.6 * U * 1.01


def test_sincos_error_is_linear_in_the_argument():
    """|sin - sin x|, |cos - cos x| <= (1.8 |x| + 4.8) u for |x| <= 1e6: the guarantee the FFT-stamp and knots structure factors
    lean on (phases kx * x of a few thousand radians lose a few thousand u, 1e-12).  u0 = x INV_TWO_PI: INV_TWO_PI misses
    1 / (2 pi) by at most half an ulp of [1/8, 1/4), 2^-56, 0.785 u relative, and the product rounds (u relative): the phase
    2 pi u0 is off by 1.785 u |x|.  u1 = u0 - floor(u0) is exact when |u0| >= 1 (a multiple of ulp(u0) >= 2^-52 in [0, 1]) and
    for 0 <= u0 < 1; for -1 < u0 < 0 the sum u0 + 1 rounds by at most u / 2 of a turn, pi u = 3.15 u of phase (and may give
    exactly 1, where sincos2pi returns (0, 1) to 1e-16).  sin and cos pass a phase error on with slope <= 1, and sincos2pi adds
    its own 1.6 u: (1.785 |x| + 3.15 + 1.6) u, asserted as (1.8 |x| + 4.8) u.  The reference is the long-double sine and cosine
    of the float64 argument itself.
    Measured: worst error / bound 0.854 (for |x| up to 10, 1e2, 1e4, 1e6: 0.702, 0.795, 0.850, 0.854)."""
    x = mc.sincos_in()
    got = orc_loader.math_probe(4, x).reshape(-1, 2).astype(LD)
    xl = x.astype(LD)
    err = np.maximum(np.abs(got[:, 0] - np.sin(xl)), np.abs(got[:, 1] - np.cos(xl)))
    bound = (1.8 * np.abs(xl) + 4.8) * U
    _report("sincos", err, bound)
    for hi in (10.0, 1e2, 1e4, 1e6):
        sel = np.abs(x) <= hi
        print(f"   |x| <= {hi:g}: worst error / bound {float(np.max(err[sel] / bound[sel])):.3f}")
    assert np.all(err <= bound)


def _atan_bound(ax):
    """the bound of test_atan_bounds at |x| = ax (float64 array), as a long-double absolute error"""
    ax = np.asarray(ax, dtype=np.float64)
    small = 4.5 * U * np.arctan(ax.astype(LD)) + np.where(ax < 2.0 ** -1021, LD(2.0) ** -1073, LD(0))
    return np.where(ax <= mc.TAN_PI_8, small, np.where(ax <= 1.0, LD(3.7 * U), LD(5.8 * U)))


def test_atan_bounds():
    """|atan - atan x| <= 4.5 u |atan x| for |x| <= tan(pi/8); <= 3.7 u absolute (9.4 u relative) for tan(pi/8) < |x| <= 1;
    <= 5.8 u absolute (7.4 u relative) for |x| > 1, +-inf included.
    Core, b the reduced argument, |b| <= tan(pi/8): cc = b / (1 + sqrt(1 + b^2)) = tan(atan(b) / 2): the fma rounds 1 + b^2 (u, which
    the root halves), dsqrt_n rounds (u): 1.5 u of a root <= 1.083, 0.81 u of the sum 1 + root >= 2, which rounds itself (u); ddiv
    rounds (u): cc is good to 2.81 u + eb (eb: the relative error of b; d ln cc / d ln b = cos(atan b) <= 1).  Series in z = cc^2
    (6.6 u + 2 eb relative): p = -1 + z / 3 - ... in [-1, -0.987]: last rounding u / 2, inherited 0.02 u, z's error through slope 1/3
    0.09 u: 0.61 u; the series after z^13 / 27 leaves 0.199^28 / 29 = 1e-21.  at = -(cc p) rounds once: atan(cc) to 2.81 + 0.61 + 1 =
    4.42 u + eb relative; res = 2 at + 0 is exact.  |x| <= tan(pi/8): b = x, eb = 0: 4.42 u relative, asserted as 4.5 u.  Below
    2^-1021 cc = b / 2 and at are subnormal and round to the grid of 2^-1074 instead (2^-1075 each, doubled): 2^-1073 is added.
    Above tan(pi/8), a = |x| or 1 / |x| (rounded: ea = u): b = (a - 1) / (a + 1): a - 1 rounds when a < 1/2 (u relative), a + 1
    rounds (u), ddiv rounds (u): eb = 3 u, and a's own error reaches atan(b) as at most ea / 2 (db/da = 2 / (a + 1)^2, a / (a + 1)^2
    <= 1/4).  atan(a) = PI_4 + 2 at: |2 atan(cc)| <= pi/8 = 0.3927 carries 7.42 u relative, 2.914 u; PI_4 misses pi/4 by 0.276 u;
    the fma rounds a result in [0.39, 0.79] (u / 2): 3.69 u for |x| <= 1, 4.19 u for 1 < |x| <= 1 + sqrt 2.  atan |x| = PI_2 - atan(a):
    PI_2 misses pi/2 by 0.552 u and the fma rounds a result in [0.785, 1.571] (u): 5.74 u; for |x| > 1 + sqrt 2 the first stage is
    2 at with 5.42 u of at most 0.3927, 2.13 u, and the total 3.68 u.  The sign of x is applied exactly.
    Measured: worst error / bound 0.852 (|x| <= tan(pi/8): 0.852; <= 1: 0.409; above: 0.464)."""
    x = mc.atan_in()
    want = np.arctan(x.astype(LD))
    err = np.abs(orc_loader.math_probe(3, x).astype(LD) - want)
    bound = _atan_bound(np.abs(x))
    ok = err <= bound                                        # 0 <= 0 at x = 0
    nz = bound > 0
    _report("atan", err[nz], bound[nz])
    ax = np.abs(x)
    for name, sel in (("|x| <= tan(pi/8)", nz & (ax <= mc.TAN_PI_8)), ("<= 1", (ax > mc.TAN_PI_8) & (ax <= 1)), ("> 1", ax > 1)):
        print(f"   {name}: worst error / bound {float(np.max(err[sel] / bound[sel])):.3f}")
    assert np.all(ok)


def _atan2_ref(y, x):
    """atan2 with the spec's conventions: libm's, except that (0, 0) of any signs gives 0 and y = -0.0 with x < 0 gives +pi"""
    want = np.arctan2(y.astype(LD), x.astype(LD))
    want = np.where((y == 0) & (x == 0), LD(0), want)
    return np.where((y == 0) & (x < 0), PI_L, want)


def test_atan2_bounds():
    """atan2(y, x) = atan(q) (+- PI for x < 0), q = y / x rounded once (u relative; the cases keep q normal): the rounding moves
    atan q by at most u |q| / (1 + q^2) <= u min(1/2, |atan q|); atan's own bound at q (test_atan_bounds) adds to it; for x < 0 PI
    misses pi by 1.22e-16 = 1.11 u and the sum rounds by up to half an ulp of pi, 2 u.  On the y axis (x = +-0, y != 0) the result is
    +-PI_2, 0.552 u from pi/2 (asserted as 0.56 u); on the x axis q = 0 and the result is 0 or PI.
    Measured: worst error / bound 0.997 (3.10 u at results next to +-pi: PI's own 1.10 u and a full half-ulp of pi do occur together)."""
    p = mc.atan2_in()
    y, x = p[:, 0].copy(), p[:, 1].copy()
    want = _atan2_ref(y, x)
    err = np.abs(orc_loader.math_probe(14, p).astype(LD) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.abs(y / x)
    assert np.all((q[x != 0] == 0) | (q[x != 0] >= 2.2250738585072014e-308)) and np.all(np.isfinite(q[x != 0]))
    q = np.where(x == 0, 0.0, q)
    at = np.arctan(q.astype(LD))
    bound = _atan_bound(q) + np.minimum(LD(0.5), at) * U + np.where(x < 0, LD(3.11 * U), LD(0))
    bound = np.where(x == 0, np.where(y == 0, LD(0), LD(0.56 * U)), bound)
    nz = bound > 0
    _report("atan2", err[nz], bound[nz])
    assert np.all(err <= bound)


def test_tanh_is_good_to_2p5_u_absolute():
    """|tanh - tanh x| <= 2.5 u for x >= 0, absolute only: T = (1 - e) / (1 + e) with e = exp(-2 x) (-2 x is exact; e to 2 u relative).
    1 - e rounds by at most u / 2 and carries e's 2 u e; 1 + e rounds by at most u and carries the same; ddiv rounds (u T):
    u [(1/2 + 2 e) / (1 + e) + T (1 + 2 e) / (1 + e) + T], which grows from 1.25 u at e = 1 (x = 0) to 2.5 u at e = 0.  For small x
    the difference 1 - e cancels: the error stays 1.25 u while tanh x ~ x, so the relative error is unbounded (1e-4 at x = 1e-12).
    That is what its callers need: the sensor multiplies tanh(z / 12) into pixel-boundary distortions of order one, where an
    absolute 3e-16 is far below the 2^-32 grid they are compared on.  Above 20 the function returns 1; 1 - tanh 20 = 8.5e-18 = 0.08 u.
    Measured: worst error / bound 0.595."""
    x = mc.tanh_in()
    want = np.tanh(x.astype(LD))
    err = np.abs(orc_loader.math_probe(5, x).astype(LD) - want)
    _report("tanh", err, np.full(x.size, 2.5 * U, dtype=LD))
    assert np.all(err <= 2.5 * U)


def test_pow_error_grows_with_the_exponent_of_e():
    """|pow - x^y| <= (2 |y ln x| + 4 |y| + 2.01) u x^y for normal x > 0 and |y ln x| <= 690.  pow = exp(y log x): log x is good to
    u |ln x| + 4 u (test_log_is_good_to_an_ulp), y times it rounds once (u |y ln x|): the argument of exp is off by
    d = (2 |y ln x| + 4 |y|) u, which exp turns into the relative error e^d - 1 = d (1 + 1e-13) -- this amplification, 140 u at
    r^(1/0.3) for r = 1e-8, is why pow has a bound of its own -- and exp adds its 2 u.  x^0 = 1 and 1^y = 1 exactly.
    Measured: worst error / bound 0.737."""
    p = mc.pow_in()
    x, y = p[:, 0].astype(LD), p[:, 1].astype(LD)
    t = np.abs(y * np.log(x))
    assert float(t.max()) <= 690.0
    want = np.power(x, y)
    got = orc_loader.math_probe(15, p)
    err = np.abs(got.astype(LD) - want)
    bound = (2 * t + 4 * np.abs(y) + 2.01) * U * want
    _report("pow", err, bound)
    assert np.all(err <= bound)
    assert np.all(got[(p[:, 1] == 0) | (p[:, 0] == 1)] == 1.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_special_values_are_spec():
    """The values at the ends of each domain, stated as the spec (the GPU test holds the device to the same bits)."""
    f = orc_loader.math_probe
    PI, PI_2 = 3.14159265358979323846, 1.57079632679489661923
    # exp: 1 at +-0; exactly 0 below the flush edge (k < -1000), -inf included; finite and positive on the capped side of the
    # upper edge (k = 1001: the scale stays 2^1000), whose magnitude is not specified
    assert np.array_equal(_bits(f(1, [0.0, -0.0])), _bits([1.0, 1.0]))
    edge = np.array(mc.around(-1000.5 * mc.LN2, 4))
    k = np.array([mc.exp_k(v) for v in edge])
    assert (k == -1001).any() and (k == -1000).any()
    assert np.all(f(1, edge[k == -1001]) == 0.0) and np.all(f(1, edge[k == -1000]) > 0.0)
    assert np.array_equal(_bits(f(1, [-745.0, -1e5, -1e300, -np.inf])), _bits([0.0] * 4))
    cap = np.array(mc.around(1000.5 * mc.LN2, 4))
    cap = cap[np.array([mc.exp_k(v) for v in cap]) == 1001]
    v = f(1, np.concatenate([cap, [700.0, 709.0, 1e5]]))
    assert cap.size and np.all(np.isfinite(v)) and np.all(v > 0)
    assert np.all(np.isnan(f(1, [np.inf, np.nan])))          # a NaN, not the silent 0 of a wrapped integer conversion
    # sincos2pi: both ends of [0, 1] give exactly (0, 1)
    assert np.array_equal(_bits(f(2, [0.0, 1.0])), _bits([0.0, 1.0, 0.0, 1.0]))
    assert np.array_equal(_bits(f(4, [0.0, -0.0])), _bits([0.0, 1.0, 0.0, 1.0]))
    assert np.all(np.isnan(f(4, [np.inf, -np.inf, np.nan])))
    # atan: +-inf give +-PI_2 as rounded; atan(-0.0) is +0.0 on both sides (the sign is applied for x < 0 only) -- pinned, not libm's
    assert np.array_equal(_bits(f(3, [np.inf, -np.inf, 0.0, -0.0])), _bits([PI_2, -PI_2, 0.0, 0.0]))
    # atan2: (0, 0) of any signs is 0; the axes; y = -0.0 with x < 0 is +PI (the device's `y >= 0` rule, which the spike kernel
    # was validated with), not libm's -pi
    z = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]
    assert np.array_equal(_bits(f(14, np.array(z))), _bits([0.0] * 4))
    ax = np.array([(-0.0, -1.0), (0.0, -1.0), (0.0, 1.0), (-0.0, 1.0), (1.0, 0.0), (-1.0, -0.0), (-5e-324, 0.0)])
    assert np.array_equal(_bits(f(14, ax)), _bits([PI, PI, 0.0, 0.0, PI_2, -PI_2, -PI_2]))
    # tanh: 0 at 0, exactly 1 above 20
    assert np.array_equal(_bits(f(5, [0.0, np.nextafter(20.0, 21.0), 30.0, 1e300, np.inf])), _bits([0.0, 1.0, 1.0, 1.0, 1.0]))
    assert f(5, [20.0])[0] == 1.0                            # rounds to 1 already
    # pow(0, y) and pow(subnormal, y): the spec's log reads the exponent field alone (-1023) and gives -1023 ln 2 there, so the
    # result is 2^(-1023 y): exactly 0 once that is flushed (y >= 0.98), 1 at y = 0, tiny but positive between, huge for y < 0.
    # Recorded, not endorsed: every caller guards x > 0.
    p = mc.pow_zero()
    got = f(15, p)
    want = np.exp(p[:, 1].astype(LD) * (-1023 * np.log(LD(2))))
    flushed = p[:, 1] * 1023 > 1000.6
    assert np.all(got[flushed] == 0.0) and np.all(got[p[:, 1] == 0] == 1.0)
    sel = ~flushed & (p[:, 1] > 0) & (p[:, 0] != 1e-310)
    assert np.all(np.abs(got[sel].astype(LD) - want[sel]) <= 1e-12 * want[sel])
    assert np.all(np.isfinite(got[p[:, 1] < 0])) and np.all(got[p[:, 1] < 0] > 1e300)       # beyond exp's cap: finite, unspecified


def test_extinction_beyond_exp_domain_is_refused():
    """ims_sed.h forms exp(-0.4 ln 10 Av (a + b / Rv)) from catalog values: Rv = 0, a NaN or an exponent past +-690 would leave
    exp's domain on the device, so the host refuses them before anything is launched."""
    from imsim_amd import sed
    grid = np.linspace(300.0, 1100.0, 50)
    a, b = sed.ccm89_terms(grid)
    sed.check_extinction([0.0, 0.3, 3.0], [3.1, 2.0, 5.5], a, b)
    for av, rv in (([0.1], [0.0]), ([np.nan], [3.1]), ([0.1], [np.nan]), ([np.inf], [3.1]), ([0.1], [1e-5]), ([1e4], [3.1]),
                   ([-1e4], [3.1])):
        with pytest.raises(ValueError):
            sed.check_extinction(av, rv, a, b)
