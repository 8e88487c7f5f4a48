"""The diffraction-spike step of the FFT branch (stamp.diffraction_fft) restated in np.longdouble, independently of
oracle/orc_fft.c, the kernels (k_fft_bbox, k_fft_spike_table, k_fft_spikes, k_fft_spikes_stream, k_fft_spikes_arms) and
imsim_amd/diffraction_fft.py.  Inputs are only what the product uploads -- the ims_spikes_t block, the ims_fft_object_t rows, the
real-space buffer -- and the written description of the operation (include/imsim_hip.h, ims_spikes_t).  There is no
table here, no early exit, no pruning of sums that are known to be zero, no interval of candidate columns:

* stencil S(a, b) at every integer offset (a rows, b columns): the anti-aliased cross max(0, 1 - min(|xr|, |yr|)) with
  (xr, yr) = (cos0 a + sin0 b, -sin0 a + cos0 b), replaced by 1 inside the swept wedge mod(atan2(b, a) - a_lo, pi/2) <= d_alpha,
  times the Lorentzian pixel integral (2 / pi) (atan((r + 1/2) s / R0) - atan((r - 1/2) s / R0)), r = hypot(a, b), over
  max(r d_alpha, 1), doubled at the origin.
* saturated box: the bounding box of the pixels above `threshold` among the pixels INSIDE the stamp; empty when there are none.
* image: out = max(in, 0); inside the stamp and with a non-empty box, the box is set to 0 and
  sum over every box pixel (ry, rx) with |iy - ry|, |ix - rx| <= cutoff of S(iy - ry, ix - rx) / norm max(in[ry, rx], 0)
  is added: the plain dense double sum.  Pixels outside the stamp are only clipped.  `norm` is the uploaded ims_spikes_t.norm.
* rbuf_raw = 1: every value read is fl64(raw fl64(1 / (nfft nfft))), formed here in float64 as the ABI comment promises.

`stencil` and `apply` return, next to the values, a bound and the offsets "near a decision".  EPS = 2^-52, u = EPS / 2; the
kernel works in float64 with correctly rounded + - * / sqrt (u each; asserted below as EPS where it costs nothing).

A stencil value S / norm, absolute:
* m = min(|xr|, |yr|): two products and a sum, each rounded at a size of at most |a| + |b| (|cos0|, |sin0| <= 1): 1.5 u (|a| + |b|)
  ... dm = 2 EPS (|a| + |b|).  1 - m rounds once more (a value <= 1): dval = dm + u; the clip at 0 is 1-Lipschitz.  Inside the
  wedge val = 1 exactly: dval = 0.  Where m - 1 > dm and the offset is outside the wedge and not near a decision the kernel's
  value is an exact zero (its early exit or its clip) and so is the bound.  edge: |m - 1| <= dm -- the kernel may have a tiny
  value where the reference has none, or the reverse; the bound covers it, the table's non-zero set may differ there.
* profile: r = sqrt(a^2 + b^2), the radicand an exact integer, the root rounded (EPS r).  t = (r +- 1/2) scale / r0: the sum, the
  product and the quotient round (3 EPS asserted), r's error enters as EPS r / |r +- 1/2|: et relative, which atan passes on as
  et |t| / (1 + t^2).  Each datan carries the absolute bound tests/test_math_spec.py holds it to (restated in _atan_bound:
  4.5 u atan|t| up to tan(pi/8), 3.7 u up to 1, 5.8 u above) -- for r >= 1 both arguments exceed 1 and this is twice 5.8 u.
  It is an ABSOLUTE term: at r = 200 the two arctangents are within 1e-6 of pi/2, their difference is ~1e-6 and its error
  still ~EPS.  The difference, the rounded constant 2 / pi and the product add 3 u of the value: 2 EPS prof asserted.
  dprof = (2 / pi) (bound(t+) + bound(t-) + et+ |t+| / (1 + t+^2) + et- |t-| / (1 + t-^2)) + 2 EPS prof.
* arc = r d_alpha rounds (u) and carries r's EPS; max(., 1) is 1-Lipschitz: 2 EPS relative of the divisor.  val prof and the
  quotient by the divisor round (EPS together), the doubling at the origin is exact, / norm rounds (EPS): 4 EPS of the value.
  bound = ((dval (prof + dprof) + val dprof) / max(arc, 1) [x 2 at the origin] + 4 EPS S) / norm, times 1 + 2^-20 for the products
  of these first-order terms.

Near a decision: the kernel's dth = datan2(b, a) - a_lo reduced by floor(dth / PI_2) PI_2 differs from the exact one by the bound
test_math_spec.py holds datan2 to (_atan2_bound) plus the subtraction, the quotient, the product with a PI_2 that misses pi/2 by
0.55 u up to three times, and the last subtraction, all at a size below 2 pi: 8 EPS.  An offset whose dth is within that of
d_alpha, or of the wrap at 0 and pi/2, AND whose two candidate values (1 in the wedge, the cross outside) differ is flagged;
the reference evaluates both candidates and widens the offset's bound by their difference (apply: times the source).  Nothing
is left out of a comparison.  On the exact axes of a cross along the axes m = 0, both candidates are 1, nothing is flagged.
The four half-axes (a = 0 or b = 0) are decided exactly where that can be proved: datan2 returns exactly 0, +-PI_2, PI there
(pinned by test_math_spec.py's edge cases), and _axis_exact follows the kernel's three operations on that constant in exact
rational arithmetic; if every intermediate is a float64 (no rounding happened), floor's argument is an integer or further from
one than its rounding, and the result equals the exact dth = -a_lo (0 <= -a_lo <= 1.5 < pi/2), the kernel's decision IS the exact
one and the offset is not flagged.  That holds for a_lo = 0 (axis_exact) and for a dyadic d_alpha with rot = pi/4 (axis_dyadic,
d_alpha = 2^-5, where dth == d_alpha on all four half-axes and the cross there is NOT 1: the one geometry on which `<` for `<=`
in the wedge test changes values); it does not hold for d_alpha = 0.04 at rot = pi/4, whose three inexact half-axes would be
flagged -- 3 cutoff offsets, far over the cap -- which is why axis_swept sits 2e-3 rad off pi/4 (and `diagonal` 3e-3 rad off 0:
at rot = 0 exactly the offsets a = +-b sit on the wedge's upper edge to rounding).
Cap (a condition, not a measurement): at most FLAG_CAP = 1e-3 of a geometry's non-zero offsets may be flagged;
tests/test_spike_ref.py checks it on the reference alone.

A pixel: the sum of its terms' bounds (a term's bound is the stencil bound times the clipped source, which is an input and
exact); the terms are non-negative, each product rounds (u) and the sequential sum of n of them rounds n - 1 times (u of a
partial sum <= the sum): (n_terms + 2) EPS of the sum asserted, n_terms counting the offsets that are not exact zeros; the last
addition to the clipped pixel rounds by u of the result: 2 EPS of the clipped pixel asserted with the term above.  Pixels outside
the stamp, and every pixel of an object with an empty box, have bound 0: they equal the clipped input.

Observed worst error / bound per geometry (every case of tests/spike_cases.py; a ratio above 1 fails; records, not thresholds):

    geometry      oracle (CPU)   MI355X
    near_axis     0.121          0.121
    generic       0.226          0.226
    diagonal      0.210          0.210
    axis_exact    0.173          0.173
    axis_swept    0.144          0.144
    axis_dyadic   0.145          0.145
    negative      0.145          0.145
    wide          0.167          0.167

(The two columns agree because the kernels give the oracle's bits on every case.  The table's values alone, ims_fft_spike_table at
cutoffs 20 and 200 on the MI355X: 0.117 .. 0.170 of the stencil bound.  No offset of any of the eight geometries is flagged.)

Mutations (`mutate=`; tests/test_spike_ref.py::test_teeth): every one of MUTATIONS leaves the bounds of the case named there.
The three that restate mistakes of the table walk model the table as the kernel's comment describes it (of stencil row a the
non-zero entries, b descending; rows longer than 16 entries entered by bisection at the first b <= bhi; batches of four from
there) and take terms away from, or add terms to, the dense sum.
"""
import fractions
import math

import numpy as np

LD = np.longdouble
EPS = LD(2.0) ** -52
U = EPS / 2
PI = 4 * np.arctan(LD(1))
HALF_PI = PI / 2
TAN_PI_8 = 0.41421356237309503
PI_2_F64 = 1.5707963267948966                     # the kernel's PI_2; PI = 2 PI_2 exactly
FLAG_CAP = 1.0e-3
EMPTY_BOX = (0x7fffffff, -1, 0x7fffffff, -1)

# mutation -> (shape, geometry) of the case of tests/spike_cases.py that catches it
MUTATIONS = {
    "batch_last_dropped": ("clip64", "generic"),      # the last entry of a four-batch dropped
    "bisect_late": ("long32", "axis_exact"),          # the bisection starting one entry late
    "b_gt_bhi_used": ("clip64", "generic"),           # entries with b > bhi (source columns left of the box) used
    "box_over_grid": ("edge96", "generic"),           # the box taken over the grid instead of the stamp
    "box_not_zeroed": ("clip64", "near_axis"),
    "source_not_clipped": ("edge96", "diagonal"),     # a negative pixel inside the box spread as it is
    "swap_ab": ("clip64", "generic"),
    "origin_not_doubled": ("long32", "negative"),
    "cutoff_lt": ("clip64", "axis_exact"),            # |a|, |b| < cutoff
    "wedge_lt": ("clip64", "axis_dyadic"),            # dth < d_alpha
    "no_inv_n2": ("batch", "generic"),                # 1 / nfft^2 missing under rbuf_raw
}


class Geometry:
    """the ims_spikes_t block as uploaded: every field a float64 (or int) taken as an exact number"""

    def __init__(self, S):
        self.cos0, self.sin0, self.a_lo, self.d_alpha = float(S.cos0), float(S.sin0), float(S.a_lo), float(S.d_alpha)
        self.scale, self.r0, self.norm = float(S.scale), float(S.r0), float(S.norm)
        self.cutoff, self.threshold, self.enabled = int(S.cutoff), float(S.threshold), int(S.enabled)

    def key(self):
        return (self.cos0, self.sin0, self.a_lo, self.d_alpha, self.scale, self.r0, self.norm, self.cutoff)


def _atan_bound(ax):
    """|datan(x) - atan x| at |x| = ax, absolute (tests/test_math_spec.py::test_atan_bounds)"""
    return np.where(ax <= TAN_PI_8, 4.5 * U * np.arctan(ax), np.where(ax <= 1.0, 3.7 * U, 5.8 * U))


def _atan2_bound(y, x):
    """|datan2(y, x) - atan2(y, x)| (tests/test_math_spec.py::test_atan2_bounds); exact at the origin and on the +x half-axis"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(x == 0, LD(0), np.abs(y / np.where(x == 0, LD(1), x)))
    b = _atan_bound(q) + np.minimum(LD(0.5), np.arctan(q)) * U + np.where(x < 0, 3.11 * U, LD(0))
    return np.where(x == 0, np.where(y == 0, LD(0), 0.56 * U), b)


def _is_f64(fr):
    return fractions.Fraction(float(fr)) == fr


def _axis_exact(th64, a_lo):
    """True if the kernel's dth on the half-axis where datan2 returns th64 is EXACTLY -a_lo = the exact dth (module docstring)"""
    F = fractions.Fraction
    if not 0.0 <= -a_lo <= 1.5:
        return False
    hp = F(PI_2_F64)
    d = F(th64) - F(a_lo)
    if not _is_f64(d):
        return False
    q = d / hp
    k = math.floor(q)
    if q != k and min(q - k, k + 1 - q) <= 4 * F(2) ** -52 * abs(q):
        return False
    p = k * hp
    return _is_f64(p) and _is_f64(d - p) and d - p == F(-a_lo)


class Stencil:
    pass


_STENCILS = {}


def stencil(g, half=None, mutate=None):
    """S (un-normalised), Sn = S / norm, bound (absolute, of the kernel's S / norm), near (flagged offsets), edge, alt (the other
    candidate of a flagged offset, un-normalised) on the (2 half + 1)^2 grid of offsets; [a + half, b + half]"""
    half = g.cutoff if half is None else int(half)
    mut = mutate if mutate in ("swap_ab", "origin_not_doubled", "wedge_lt") else None
    key = (g.key(), half, mut)
    if key in _STENCILS:
        return _STENCILS[key]
    rng = np.arange(-half, half + 1).astype(LD)
    a, b = np.broadcast_arrays(rng[:, None], rng[None, :])
    if mut == "swap_ab":
        a, b = b, a
    c0, s0, a_lo, da, sc, r0, norm = (LD(v) for v in (g.cos0, g.sin0, g.a_lo, g.d_alpha, g.scale, g.r0, g.norm))
    xr, yr = c0 * a + s0 * b, -s0 * a + c0 * b
    m = np.minimum(np.abs(xr), np.abs(yr))
    cross = np.maximum(LD(0), 1 - m)
    on_axis = ((a == 0) | (b == 0)) & ~((a == 0) & (b == 0))
    th = np.where(on_axis, LD(0), np.arctan2(b, a))           # a half-axis is an exact multiple of pi/2 from the +a one
    dth = np.mod(th - a_lo, HALF_PI)
    inw = (dth < da) if mut == "wedge_lt" else (dth <= da)
    tol = _atan2_bound(b, a) + 8 * EPS
    proved = np.zeros(a.shape, dtype=bool)
    for th64, sel in ((0.0, (b == 0) & (a > 0)), (PI_2_F64, (a == 0) & (b > 0)), (2 * PI_2_F64, (b == 0) & (a < 0)),
                      (-PI_2_F64, (a == 0) & (b < 0))):
        if _axis_exact(th64, g.a_lo):
            proved |= sel
    near = ((np.abs(dth - da) <= tol) | (dth <= tol) | (HALF_PI - dth <= tol)) & (cross != 1) & ~proved
    val = np.where(inw, LD(1), cross)
    other = np.where(inw, cross, LD(1))
    r = np.sqrt(a * a + b * b)
    tp, tm = (r + LD(0.5)) * sc / r0, (r - LD(0.5)) * sc / r0
    prof = (2 / PI) * (np.arctan(tp) - np.arctan(tm))
    den = np.maximum(r * da, LD(1))
    f0 = np.where((a == 0) & (b == 0), LD(1) if mut == "origin_not_doubled" else LD(2), LD(1))
    S = val * prof / den * f0
    # bounds
    dm = 2 * EPS * (np.abs(a) + np.abs(b))
    dval = np.where(inw, LD(0), dm + U)
    et_p, et_m = EPS * r / np.abs(r + LD(0.5)) + 3 * EPS, EPS * r / np.abs(r - LD(0.5)) + 3 * EPS
    atp, atm = np.abs(tp), np.abs(tm)
    dprof = (2 / PI) * (_atan_bound(atp) + _atan_bound(atm) + et_p * atp / (1 + tp * tp) + et_m * atm / (1 + tm * tm)) + 2 * EPS * prof
    bound = ((dval * (prof + dprof) + val * dprof) / den * f0 + 4 * EPS * S) / norm * (1 + LD(2.0) ** -20)
    bound = bound + np.where(near, np.abs(val - other) * prof / den * f0 / norm, LD(0))
    sure_zero = (m - 1 > dm) & ~inw & ~near
    bound = np.where(sure_zero, LD(0), bound)
    st = Stencil()
    st.half, st.S, st.Sn, st.bound, st.near = half, S, S / norm, bound, near
    st.edge = (np.abs(m - 1) <= dm) & ~inw
    st.alt = other * prof / den * f0
    st.live = (S != 0) | (bound != 0)                        # the offsets that are not exact zeros for the kernel
    _STENCILS[key] = st
    return st


def stencil_sum(g, half=None):
    """sum of S over the (2 half + 1)^2 grid and the number of its terms (what diffraction_fft.stencil_norm approximates)"""
    st = stencil(g, half)
    return np.sum(st.S), st.S.size


def _box(sat):
    ys, xs = np.nonzero(sat)
    if ys.size == 0:
        return EMPTY_BOX
    return int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())


def _walk_delta(g, st, v, box, inst, mutate):
    """what a mistake of the table walk adds to the dense sum of every target (float64-sized effects: plain Python loops)"""
    c, n = g.cutoff, v.shape[0]
    r0, r1, c0, c1 = box
    rows = {}
    for a in range(-c, c + 1):
        bs = np.nonzero(st.S[a + c] != 0)[0][::-1] - c       # b descending
        rows[a] = (bs, st.Sn[a + c, bs + c])
    delta = np.zeros((n, n), dtype=LD)
    for iy in range(n):
        for ry in range(max(r0, iy - c), min(r1, iy + c) + 1):
            bs, sv = rows[iy - ry]
            if bs.size == 0:
                continue
            for ix in range(n):
                if not inst[iy, ix]:
                    continue
                blo, bhi = ix - c1, ix - c0
                start = int(np.count_nonzero(bs > bhi)) if bs.size > 16 else 0
                if mutate == "bisect_late" and bs.size > 16:
                    lost = (np.arange(bs.size) == start) & (bs >= blo) & (bs <= bhi)
                elif mutate == "batch_last_dropped":
                    lost = ((np.arange(bs.size) - start) % 4 == 3) & (np.arange(bs.size) >= start) & (bs >= blo) & (bs <= bhi)
                else:
                    lost = np.zeros(bs.size, dtype=bool)
                for j in np.nonzero(lost)[0]:
                    delta[iy, ix] -= sv[j] * max(v[ry, ix - bs[j]], 0.0)
                if mutate == "b_gt_bhi_used" and bs.size <= 16:
                    for j in np.nonzero((bs > bhi) & (ix - bs >= 0))[0]:
                        delta[iy, ix] += sv[j] * max(v[ry, ix - bs[j]], 0.0)
    return delta


def apply(S, rows, rbuf, raw=False, mutate=None):
    """the spike step on every object of `rows` (ims_fft_object_t records) reading `rbuf`: (out, bound, boxes), out and bound
    np.longdouble arrays laid out like rbuf, boxes int [n_objects][4] = rowmin, rowmax, colmin, colmax (EMPTY_BOX: none)"""
    assert mutate is None or mutate in MUTATIONS
    g = S if isinstance(S, Geometry) else Geometry(S)
    rbuf = np.asarray(rbuf, dtype=np.float64)
    out, bound, boxes = np.zeros(rbuf.size, dtype=LD), np.zeros(rbuf.size, dtype=LD), []
    c = g.cutoff
    reach = c - 1 if mutate == "cutoff_lt" else c
    st = stencil(g, c, mutate)
    for o in rows:
        n, off = int(o["nfft"]), int(o["r_offset"])
        v = rbuf[off:off + n * n].reshape(n, n)
        if raw and mutate != "no_inv_n2":
            v = v * (np.float64(1.0) / (np.float64(n) * np.float64(n)))            # float64: the product the ABI promises
        iy, ix = np.mgrid[0:n, 0:n]
        px, py = int(o["x0"]) + ix, int(o["y0"]) + iy
        inst = (px >= int(o["stamp_xmin"])) & (px <= int(o["stamp_xmax"])) & (py >= int(o["stamp_ymin"])) & (py <= int(o["stamp_ymax"]))
        sat = (v > g.threshold) & (inst if mutate != "box_over_grid" else True)
        box = _box(sat) if g.enabled else EMPTY_BOX
        boxes.append(box)
        img = np.maximum(v, 0.0).astype(LD)
        res, bnd = img.copy(), np.zeros((n, n), dtype=LD)
        if box[1] >= box[0]:
            r0, r1, c0, c1 = box
            base = img.copy()
            if mutate != "box_not_zeroed":
                base[r0:r1 + 1, c0:c1 + 1] = 0
            acc, accb, nterm = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=np.int64)
            for ry in range(r0, r1 + 1):
                for rx in range(c0, c1 + 1):
                    src = LD(v[ry, rx]) if mutate == "source_not_clipped" else img[ry, rx]
                    if src == 0:
                        continue
                    ylo, yhi, xlo, xhi = max(0, ry - reach), min(n - 1, ry + reach), max(0, rx - reach), min(n - 1, rx + reach)
                    sl = (slice(ylo - ry + c, yhi - ry + c + 1), slice(xlo - rx + c, xhi - rx + c + 1))
                    tg = (slice(ylo, yhi + 1), slice(xlo, xhi + 1))
                    acc[tg] += st.Sn[sl] * src
                    accb[tg] += st.bound[sl] * abs(src)
                    nterm[tg] += st.live[sl]
            if mutate in ("batch_last_dropped", "bisect_late", "b_gt_bhi_used"):
                acc = acc + _walk_delta(g, st, v, box, inst, mutate)
            res = np.where(inst, base + acc, img)
            bnd = np.where(inst, accb + (nterm + 2) * EPS * np.abs(acc) + 2 * EPS * base, LD(0))
        out[off:off + n * n], bound[off:off + n * n] = res.ravel(), bnd.ravel()
    return out, bound, np.array(boxes, dtype=np.int64).reshape(-1, 4)


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the pixels with a bound; pixels with bound 0 must agree exactly (ratio inf otherwise)"""
    err = np.abs(np.asarray(got).astype(LD) - want)
    if np.any((bound == 0) & (err != 0)):
        return float("inf")
    nz = bound > 0
    return float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0
