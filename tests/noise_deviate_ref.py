"""The counter-addressed Poisson deviate restated in plain numpy, its exact law, and a bound for log Gamma.

Independent of oracle/, of the kernels and of imsim_amd's samplers: the inputs are the written spec ("The Poisson
deviate") and the published algorithm (W. Hoermann, "The transformed rejection method for generating Poisson random
variables", Insurance: Mathematics and Economics 12 (1993) 39-45, algorithm PTRS).  Philox4x32-10 is
tests/photon_source_ref.py's integer restatement; after the integer words everything is np.longdouble, and log Gamma comes
from mpmath at 40 digits -- never from a Stirling series.

poisson_ref(mean, seed, obj_id, pixel)
    block of (seed, obj_id, pixel, slot), slot = 32, 33, ...; a = (w0 2^32 + w1) >> 11, b = (w2 2^32 + w3) >> 11;
    u01(k) = k / 2^53, u01_open(k) = (k + 1) / 2^53.
    not (mean > 0) (NaN included): 0.
    mean < 10:  L = exp(-mean), p = 1, k = 0; per block: p *= u01_open(a); p <= L -> k; k += 1; the same with b; after 64
                blocks: k (= 128).
    mean >= 10: PTRS with U = u01(a) - 1/2, V = u01_open(b), at most 64 trips, then floor(mean + 1/2).

Near ties -- the draws left out of an equality.  A draw is flagged when a comparison of the algorithm is decided by less than
what the f64 evaluation of the spec may differ by from the exact value; eps = 2^-53 below.

* multiplication branch, |p - L| <= n eps p + (1e-15 + eps) L after n factors: the factors are exact doubles, so the f64
  product carries at most n - 1 roundings, each relative eps; exp is held to 1e-15 relative by tests/test_oracle_math.py, and
  its argument -mean is exact.
* PTRS, the argument x = (2 a / us + b) U + mean + 0.43 of floor within T_x of an integer,
      T_x = 16 eps (|2 a U / us| + b |U| + mean + 1):
  U and us = 1/2 - |U| are exact (multiples of 2^-53 below 1/2); b = 0.931 + 2.53 sqrt(mean) carries three roundings and
  a = -0.059 + 0.02483 b two more with a cancellation of at most 1.4 (b >= 8.9), the division, the product and the three sums
  one each: under 8 eps of the largest partial sum, doubled.
* PTRS, V within 8 eps of vr = 0.9277 - 3.6224 / (b - 2) (three roundings of a number below 1).
  us >= 0.07, us < 0.013 and V > us compare exact doubles: no tie is possible.
* PTRS, the acceptance inequality lhs <= rhs with
      lhs = log V + log invalpha - log(a / us^2 + b),     rhs = -mean + k log(mean) - lgamma(k + 1),
  |lhs - rhs| <= T_acc,
      T_acc = E(V) + E(invalpha) + E(a / us^2 + b) + 16 eps                       the three logs, and 8 eps relative in each of
            + 4 eps (|log V| + |log invalpha| + |log(a / us^2 + b)|)              the two computed arguments; the two sums
            + k E(mean) + eps |k log(mean)|                                        the log of the mean times k; the product
            + eps (|k log(mean) - mean| + |rhs|)                                   the two sums: a sum is off by eps of its RESULT
            + lgamma_bound(k + 1)
  with E(x) = 2^-53 |log x| + 2^-51, the bound tests/test_oracle_math.py asserts for log (test_log_is_good_to_an_ulp, where
  it is derived from the spec's evaluation).  At mean 1e9, where k log(mean) = 2e10 has an ulp of 4e-6, T_acc = 2e-5: 3e-6
  from k E(mean), 5e-6 from the three roundings above and 1.2e-5 from lgamma_bound.

lgamma_bound(x), for the spec's evaluation (upward recurrence to x' = x + n >= 8, then
(x' - 1/2) log x' - x' + log(2 pi) / 2 + (1/12 - 1/(360 x'^2) + 1/(1260 x'^4) - 1/(1680 x'^6)) / x' minus the summed logs):
      1 / (1188 x'^9)                                   first omitted term of the (alternating, enveloping) series at x' >= 8
    + (x' - 1/2) E(x') + eps x' |log x'|                the log; the product (x' - 1/2 is exact)
    + eps (3 |lgamma(x')| + 8)                          the three sums, each off by eps of its result, which is lgamma(x') up to
                                                        terms below 1; the series itself (a number below 1/96) in the 8
    + sum_i E(x + i) + (n + 2) eps (sum_i |log(x + i)| + |lgamma(x')|)            the recurrence: n logs, n sums, the subtraction

A flagged draw's value is still returned (from the long double evaluation); every later trip it would have taken is not
followed.  The share of flagged draws is a condition: at most EDGE_SHARE_CAP of a case's draws, asserted before anything is
compared.  Measured from this module alone (2^17 draws per case, seed 11, object ids 3 and 0x7F00000003): 2.3e-5 and 5.3e-5
at mean 1e9, none at any other law mean, on the ramp or at the edge means.

Observed worst |error| / bound of log Gamma (probe 13; 1e5 points log-spaced over [1, 1e10], the integers 1..64, the
neighbours of 8):

    oracle (CPU)   MI355X
    0.968          0.968          (what the tests print; they assert a ratio of at most 1)

law_pvalue(values, mean): Pearson chi^2 against scipy.stats.poisson.  One bin per integer where sigma / 8 < 2, bins of width
floor(sigma / 8) through the CDF otherwise, from mean - 9 sigma to mean + 9 sigma with both tails kept as bins; neighbours
merged from the left until every expected count is at least 50 (the last bin takes what is left).  The pass mark
P_PASS = 1e-6 is the chi^2 law's: a correct sampler falls below it once in a million cases, and the draws are
counter-addressed, so a case passes or fails for good.
"""
import mpmath
import numpy as np
from scipy import stats

from photon_source_ref import philox4x32_10, LD, U64, M32

EPS = LD(2.0) ** -53
TWO53 = LD(2.0) ** 53
EDGE_SHARE_CAP = 1.0e-4
P_PASS = 1.0e-6
LOG_RTOL, LOG_ATOL, EXP_RTOL = LD(2.0) ** -53, LD(2.0) ** -51, LD(1e-15)      # tests/test_oracle_math.py
FIRST_SLOT, MAX_TRIPS, BRANCH = 32, 64, 10.0

# the constants of PTRS as published, and the two choices of the spec; a test passes a changed copy to prove it can fail
PTRS = dict(shift=0.43, vr=None, squeeze=0.07, squeeze_lo=0.013, invalpha_scale=1.0, stirling_c1=None, v_open=True)


def draw_ab(seed, obj_id, pixel, slot):
    """the two 53-bit integers of the block (seed, obj_id, pixel, slot): counter = (pixel lo, pixel hi, slot, obj_id lo),
    key = (seed lo, seed hi ^ obj_id hi); obj_id a number or an array like pixel (two's complement, as pixel)"""
    pixel = np.atleast_1d(np.asarray(pixel, dtype=np.int64)).astype(U64)
    n = len(pixel)
    obj = np.broadcast_to(np.atleast_1d(np.asarray(obj_id, dtype=np.int64)).astype(U64), (n,))
    seed = int(seed) & (2 ** 64 - 1)
    w = philox4x32_10((pixel & M32, pixel >> U64(32), np.full(n, slot, dtype=U64), obj & M32),
                      (np.full(n, seed & 0xFFFFFFFF, dtype=U64), U64(seed >> 32) ^ (obj >> U64(32))))
    return ((w[0] << U64(32)) | w[1]) >> U64(11), ((w[2] << U64(32)) | w[3]) >> U64(11)


def u01(k):
    return k.astype(LD) / TWO53


def u01_open(k):
    return (k.astype(LD) + 1) / TWO53


def log_err(x):
    """E(x): what the spec's log may differ by from the exact one"""
    return LOG_RTOL * np.abs(np.log(x)) + LOG_ATOL


_mp = mpmath.mp.clone()
_mp.dps = 40


def _to_ld(v):
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def lgamma_exact(x):
    """log Gamma of positive doubles, long double rounded from mpmath's 40 digits"""
    x = np.asarray(x, dtype=np.float64)
    uniq, inv = np.unique(x.ravel(), return_inverse=True)
    vals = np.array([_to_ld(_mp.loggamma(_mp.mpf(float(v)))) for v in uniq], dtype=LD) if len(uniq) else np.zeros(0, dtype=LD)
    return vals[inv].reshape(x.shape)


def lgamma_bound(x, exact=None):
    """bound on |spec's lgamma(x) - log Gamma(x)| for doubles x > 0 (derivation in the module docstring)"""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    n = np.maximum(np.ceil(8 - x), 0)
    xs = x + n
    if exact is None:
        exact = lgamma_exact(xs.astype(np.float64))           # only its size is used
    lx = np.abs(np.log(xs))
    out = 1 / (1188 * xs ** 9) + (xs - LD(0.5)) * log_err(xs) + EPS * xs * lx
    shift_err, shift_abs = np.zeros_like(x), np.zeros_like(x)
    for i in range(8):
        on = i < n
        xi = np.where(on, x + i, LD(1))
        shift_err = shift_err + np.where(on, log_err(xi), 0)
        shift_abs = shift_abs + np.where(on, np.abs(np.log(xi)), 0)
    big = shift_abs + np.abs(exact)                            # at least |lgamma(x')|
    return out + EPS * (3 * big + 8) + shift_err + (n + 2) * EPS * big


def _stirling_shift(x, c1):
    """what the spec's lgamma moves by when the series' first coefficient is c1 instead of 1/12: (c1 - 1/12) / x', x' >= 8"""
    xs = x + np.maximum(np.ceil(8 - x), 0)
    return (LD(c1) - LD(1) / 12) / xs


def poisson_ref(mean, seed, obj_id, pixel, constants=None):
    """(value, near_tie) per draw; mean, obj_id and pixel broadcast against each other.  constants: a changed copy of PTRS."""
    C = dict(PTRS)
    C.update(constants or {})
    mean, pixel, obj_id = np.broadcast_arrays(np.asarray(mean, dtype=np.float64), np.asarray(pixel, dtype=np.int64),
                                              np.asarray(obj_id, dtype=np.int64))
    shape = mean.shape
    mean64, pixel, obj_id = mean.ravel(), pixel.ravel(), obj_id.ravel()
    n = len(mean64)
    value = np.zeros(n, dtype=np.float64)
    tie = np.zeros(n, dtype=bool)
    with np.errstate(invalid="ignore"):
        pos = mean64 > 0.0
        small = pos & (mean64 < BRANCH)
        large = pos & ~small

    # ---- multiplication method
    idx = np.flatnonzero(small)
    if len(idx):
        m = mean64[idx].astype(LD)
        L = np.exp(-m)
        p = np.ones(len(idx), dtype=LD)
        k = np.zeros(len(idx))
        nf = 0
        for trip in range(MAX_TRIPS):
            halves = list(draw_ab(seed, obj_id[idx], pixel[idx], FIRST_SLOT + trip))
            for h in range(2):
                nf += 1
                p = p * u01_open(halves[h])
                near = np.abs(p - L) <= nf * EPS * p + (EXP_RTOL + EPS) * L
                done = (p <= L) | near
                tie[idx[near]] = True
                value[idx[done]] = k[done]
                go = ~done
                idx, L, p, k, halves[1] = idx[go], L[go], p[go], k[go] + 1, halves[1][go]
            if not len(idx):
                break
        value[idx] = 2.0 * MAX_TRIPS

    # ---- PTRS
    idx = np.flatnonzero(large)
    if len(idx):
        m = mean64[idx].astype(LD)
        slam, loglam = np.sqrt(m), np.log(m)
        b_ = LD(0.931) + LD(2.53) * slam
        a_ = LD(-0.059) + LD(0.02483) * b_
        inva = (LD(1.1239) + LD(1.1328) / (b_ - LD(3.4))) * LD(C["invalpha_scale"])
        vr = LD(0.9277) - LD(3.6224) / (b_ - LD(2.0)) if C["vr"] is None else np.full(len(idx), LD(C["vr"]))
        for trip in range(MAX_TRIPS):
            ka, kb = draw_ab(seed, obj_id[idx], pixel[idx], FIRST_SLOT + trip)
            U = u01(ka) - LD(0.5)
            V = u01_open(kb) if C["v_open"] else u01(kb)
            us = LD(0.5) - np.abs(U)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                x = (2 * a_ / us + b_) * U + m + LD(C["shift"])
                k = np.floor(x)
                tx = 16 * EPS * (np.abs(2 * a_ * U / us) + b_ * np.abs(U) + m + 1)
                near = ~(np.abs(x - np.rint(x)) > tx)
                near |= (us >= LD(C["squeeze"])) & (np.abs(V - vr) <= 8 * EPS)
                fast = (us >= LD(C["squeeze"])) & (V <= vr)
                skip = (k < 0) | ((us < LD(C["squeeze_lo"])) & (V > us))
                full = ~fast & ~skip & ~near
                acc = np.zeros(len(idx), dtype=bool)
                if full.any():
                    f = np.flatnonzero(full)
                    kf, Vf = k[f], V[f]
                    arg3 = a_[f] / (us[f] * us[f]) + b_[f]
                    lg = lgamma_exact((kf + 1).astype(np.float64))
                    tl = lgamma_bound((kf + 1).astype(np.float64), lg)
                    if C["stirling_c1"] is not None:
                        lg = lg + _stirling_shift(kf + 1, C["stirling_c1"])
                    logV = np.log(Vf)
                    lhs = logV + np.log(inva[f]) - np.log(arg3)
                    kl = kf * loglam[f]
                    rhs = -m[f] + kl - lg
                    t = (np.where(Vf > 0, LOG_RTOL * np.abs(logV), 0) + LOG_ATOL + log_err(inva[f]) + log_err(arg3) + 16 * EPS
                         + 4 * EPS * (np.where(Vf > 0, np.abs(logV), 0) + np.abs(np.log(inva[f])) + np.abs(np.log(arg3)))
                         + kf * log_err(m[f]) + EPS * (np.abs(kl) + np.abs(kl - m[f]) + np.abs(rhs)) + tl)
                    nearf = np.abs(lhs - rhs) <= t
                    near[f[nearf]] = True
                    acc[f] = (lhs <= rhs) & ~nearf
            done = fast | acc | near
            tie[idx[near]] = True
            value[idx[done]] = k[done].astype(np.float64)
            go = ~done
            idx, m, loglam, b_, a_, inva, vr = idx[go], m[go], loglam[go], b_[go], a_[go], inva[go], vr[go]
            if not len(idx):
                break
        if len(idx):
            fb = m + LD(0.5)
            tie[idx[np.abs(fb - np.rint(fb)) <= 4 * EPS * fb]] = True
            value[idx] = np.floor(fb).astype(np.float64)
    return value.reshape(shape), tie.reshape(shape)


def assert_equal_apart_from_ties(got, mean, seed, obj_id, pixel, what, ref=None):
    """the reference's flagged share is within the cap, THEN every other draw is equal; returns the share"""
    want, tie = poisson_ref(mean, seed, obj_id, pixel) if ref is None else ref
    share = float(tie.mean()) if tie.size else 0.0
    assert share <= EDGE_SHARE_CAP, f"{what}: {share:.3g} of the draws are near ties"
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    bad = (got != want) & ~tie
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} draws differ from the reference, first at "
                           f"{np.flatnonzero(bad.ravel())[:5]}: got {got[bad][:5]}, want {want[bad][:5]}, "
                           f"flagged {int(tie.sum())}")
    return share


# ---------------- the law ----------------
def law_bins(mean, n):
    """(lower edges of the inner bins [e_i, e_i+1), expected counts of: the lower tail, the inner bins, the upper tail) after merging"""
    sigma = np.sqrt(mean)
    w = int(np.floor(sigma / 8))
    if w < 2:
        w = 1
    lo = max(int(np.floor(mean - 9 * sigma)), 0)
    hi = int(np.ceil(mean + 9 * sigma)) + 1
    edges = np.arange(lo, hi + w, w, dtype=np.float64)
    cdf = stats.poisson.cdf(edges - 1, mean)                  # P(k < e)
    sf = stats.poisson.sf(edges - 1, mean)                    # P(k >= e)
    # differences of the cdf below the median, of the survival function above: no cancellation in either tail
    inner = np.where(edges[:-1] < mean, cdf[1:] - cdf[:-1], sf[:-1] - sf[1:])
    expect = n * np.concatenate([[cdf[0]], inner, [sf[-1]]])
    # merge from the left; bins: (-inf, e0), [e0, e1), ..., [e_last, inf)
    keep_edges, merged, run = [], [], 0.0
    for i, e in enumerate(expect):
        run += e
        if run >= 50.0 and i < len(expect) - 1:
            merged.append(run)
            keep_edges.append(edges[i])                        # upper edge of the bin just closed
            run = 0.0
    if merged and run < 50.0:
        merged[-1] += run
        keep_edges.pop()
    else:
        merged.append(run)
    return np.array(keep_edges), np.array(merged)


def law_pvalue(values, mean):
    """upper-tail p-value of Pearson's chi^2 of `values` against Poisson(mean)"""
    values = np.asarray(values, dtype=np.float64).ravel()
    edges, expect = law_bins(float(mean), len(values))
    if len(expect) < 2:
        return 1.0 if np.all(values == values[0]) else 0.0
    counts = np.bincount(np.searchsorted(edges, values, side="right"), minlength=len(expect))
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    return float(stats.chi2.sf(chi2, len(expect) - 1))


def tail_interval(q, n, level=1.0e-6):
    """two-sided binomial interval of the count of an event of probability q in n draws"""
    if q <= 0.0:
        return 0, 0
    return int(stats.binom.ppf(level / 2, n, q)), int(stats.binom.isf(level / 2, n, q))


def normal_pvalue(values, bins=64):
    """chi^2 of `values` against the standard normal law over `bins` equiprobable bins"""
    values = np.asarray(values, dtype=np.float64).ravel()
    edges = stats.norm.ppf(np.arange(1, bins) / bins)
    counts = np.bincount(np.searchsorted(edges, values, side="right"), minlength=bins)
    e = len(values) / bins
    return float(stats.chi2.sf(float(((counts - e) ** 2 / e).sum()), bins - 1))
