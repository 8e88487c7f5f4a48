"""The update-free half of the Silicon sensor restated in plain numpy, independently of oracle/ and the kernels: the photon
conversion (absorption length, conversion depth, lateral walk, diffusion, shrink factor, coin) and the initial tree-ring state
of the pixel boundaries.  Written from the field descriptions of ims_sensor_t / ims_photons_t (include/imsim_hip.h) and the
formulas of GalSim's SiliconSensor as imSim uses it; inputs are only the data the product uploads (engine.SensorSetup).  After
the integer words of Philox everything is np.longdouble with libm's logl / cosl / sinl / tanhl / sqrtl.

Every value comes with a bound computed from the case's own numbers, never from what the code under test returns.
eps = 2^-52; S = 2.5e-12, the relative accuracy of the spec's log of a word, and D = 1.7e-11 r, the accuracy of a Gaussian
deviate of radius r (1.5e-11 of the sine / cosine series cut at 2^-36, plus half the log's), are the figures
tests/photon_source_ref.py uses and tests/test_oracle_math.py asserts.

Conversion (photon at x, y with slopes dxdz, dydz and wavelength wl; T = thickness, p = pixel_size):

* f = (wl - wl_min) / step carries two roundings: e_f = 2 eps |f| (+ eps |wl| / step from the subtraction).  The absorption
  length L = v0 + a (v1 - v0) moves by |v1 - v0| e_f and has three roundings at the size of its operands:
  e_L = |v1 - v0| e_f + 4 eps max(|v0|, |v1|).
* si = -L ln u:  e_si = |ln u| e_L + si (S + 2 eps).
* with angles dz = si / sqrt(1 + dxdz^2 + dydz^2) (the root's argument has three roundings, the root halves them, the
  division adds one): e_dz = e_si / norm + 4 eps dz; after the clip dz = T - 1, formed once: e_dz = eps T.  min() is
  continuous, so the bound of the unclipped value holds on either side of the threshold.
* walk: x moves by dxdz dz / p:  e_walk = |dxdz| e_dz / p + 8 eps |dxdz dz / p|  (two roundings of the product and
  quotient, and the sum rounds at their size).
* zconv = T - dz:  e_z = e_dz + eps T.
* sigma = diff_step sqrt(zconv / T) / p.  The root is not Lipschitz at zconv = 0, so its error is taken as the difference of
  the roots at zconv +- e_z:  e_sigma = diff_step / p (sqrt((zconv + e_z) / T) - sqrt(max(zconv - e_z, 0) / T)) + 8 eps sigma
  (the product may form diff_step / (T p) first and the root of zconv T: six roundings).
* kick g sigma with |g| <= r:  e_kick = sigma r D + |g| e_sigma + 8 eps |g sigma|.
* x0, y0:  e_walk + e_kick + 4 eps |x|  (the additions round at the size of their operands; the shares of the walk and the
  kick are in their own terms).
* zfactor = tanh(zconv / 12): slope <= 1 / 12, and the spec's tanh is (1 - e) / (1 + e) with e = exp(-2 z) <= 1 from an
  exponential good to 2 ulp at an argument with relative rounding eps (|argument| <= 2 T / 12): absolute error
  <= eps (8 + 4 zconv / 12).  e_zf = e_z / 12 + eps (8 + 4 zconv / 12).

Decisions that can flip on the last bit -- lost (zconv < 0), clipped (dz > T - 1), the absorption bin (f against an integer,
0 and n - 1) -- are marked ambiguous where the reference's own value is within its bound of the threshold; such photons are left
out, and their share is capped at photon_source_ref.EDGE_SHARE_CAP.  The coin is bit 31 of word 3: exact.

Tree rings (owned point at nominal local position e of owner cell (ci, cj), ring centre c, table step dr, h2 = dr^2 / 6):

* position q = (xmin + ci) - 1/2 + e: two roundings at |q|;  t = q - c: one more at |t|:  e_t = eps (2 |q| + |t|) per axis.
* r = sqrt(tx^2 + ty^2):  e_r = sqrt(2) e_t + 3 eps r.   f = r / dr:  e_f = e_r / dr + eps f.
* the spline a v0 + b v1 + ((a^3 - a) m0 + (b^3 - b) m1) h2 has |d/df| <= |v1 - v0| + 2 (|m0| + |m1|) h2 on its interval
  (|3 a^2 - 1| <= 2) and a dozen roundings at the size of its terms:
  e_s = slope e_f + 16 eps (|v0| + |v1| + (|m0| + |m1|) h2).
* point = e + s t / r:  e_point = e_s + |s| (2 e_t / r + 6 eps) + 2 eps |e|.  (2 e_t / r: the direction t / r of a point close to
  the centre is ill conditioned, and the bound says so.)
* ambiguous: f within e_f of an integer (the interval), of n - 1 (beyond it the shift is zero, a jump unless the table ends on
  zero), or of 0.

Second derivatives of the natural spline: tridiag(1, 4, 1) m = b, b = 6 (y[i - 1] - 2 y[i] + y[i + 1]) / dr^2, has
|inverse|_inf <= 1 / 2, |b| <= 24 Y / dr^2 (Y = max|y|), |m| <= 12 Y / dr^2 and condition number <= 3; a backward-stable f64
solution with a constant of 8 is within 8 * 3 * 12 eps Y / dr^2 = 288 eps Y / dr^2.  The host builds its spline on the nodes it
tabulated, fl(i dr) or a linspace, each within eps r of i dr, while the device reads the table as uniform: the interval lengths
differ relatively by up to eps (n - 1), which moves b by 2 eps (n - 1) |b| and the matrix by eps (n - 1):
(48 + 6 * 12) / 2 = 60 eps (n - 1) Y / dr^2 more.  `spline_m_bound` is the sum.  (The first statement of this bound had only the
first term; the production table of 2667 nodes on linspace(0, 8000) differs from the uniform-grid spline by 880 eps Y / dr^2
near r = 7900, which is the second term at work -- 5e-12 of the table's amplitude in the shift, far inside the point bound's
own terms -- not an error of the host.)

Observed worst error / bound per quantity (every case of tests/sensor_convert_cases.py; a ratio above 1 fails the test):

    quantity     oracle (CPU)   MI355X
    x            -              0.509
    y            -              0.504
    zfactor      -              0.451
    point_x      0.13           0.13
    point_y      0.16           0.16
    tr_table2    0.0113         (host)

(x, y, zfactor: the oracle keeps no converted pool; it is held to the reference through the pixel every photon lands in.
tr_table2: the host's second derivatives against `natural_spline_m`, the four-point table; the production table 0.0055.)
"""
import numpy as np

from photon_source_ref import DEVIATE_ERR, EDGE_SHARE_CAP, EPS, LD, gauss_pair, w01, words

SLOT_SENSOR = 24
LOG_ERR = LD(2.5e-12)
OBJ_FAINT = 1
ZFIT = LD(12)


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


class Sensor:
    """the numbers of an engine.SensorSetup (what the product uploads), nothing derived"""

    def __init__(self, ss):
        m = ss.model
        self.nV = int(m.num_vertices)
        self.pixel_size, self.thickness, self.diff_step = LD(m.pixel_size), LD(m.thickness), LD(m.diff_step)
        self.emptypoly = np.asarray(m.emptypoly, dtype=np.float64).reshape(4 * self.nV + 4, 2)
        wl = np.asarray(ss.abs_wl, dtype=np.float64)
        self.abs_wl_min, self.abs_wl_step = LD(wl[0]), LD(wl[1] - wl[0])          # the two doubles of ims_sensor_t
        self.abs_len = np.asarray(ss.abs_len, dtype=np.float64)
        self.tr_table = None if ss.tr_table is None else np.asarray(ss.tr_table, dtype=np.float64)
        self.tr_table2 = None if ss.tr_table2 is None else np.asarray(ss.tr_table2, dtype=np.float64)
        self.tr_dr = LD(ss.tr_dr)
        self.tr_center = (LD(ss.tr_center[0]), LD(ss.tr_center[1]))
        self.slots = ss.slots


class Converted:
    """per photon, np.longdouble: x0, y0, zconv, zfactor and their bounds e_x, e_y, e_z, e_zf; bool: coin, lost, clipped,
    outside (wavelength beyond the table), ambiguous; int: bin (absorption interval, -1 / n - 1 when held at an end)"""


def convert(sensor, seed, obj_id, k, x, y, dxdz, dydz, wl, has_angles):
    s = sensor
    k = np.atleast_1d(np.asarray(k, dtype=np.int64))
    x, y, dxdz, dydz, wl = (_ld(np.atleast_1d(v)) for v in (x, y, dxdz, dydz, wl))
    T, p = s.thickness, s.pixel_size
    w = words(seed, obj_id, k, SLOT_SENSOR)
    out = Converted()
    out.coin = (w[3] >> np.uint64(31)) & np.uint64(1) == 1
    # absorption length
    n = len(s.abs_len)
    f = (wl - s.abs_wl_min) / s.abs_wl_step
    e_f = EPS * (2 * np.abs(f) + np.abs(wl) / s.abs_wl_step)
    below, above = f <= 0, f >= n - 1
    t = np.clip(np.floor(f).astype(np.int64), 0, n - 2)
    a = f - t
    v0, v1 = _ld(s.abs_len[t]), _ld(s.abs_len[t + 1])
    L = np.where(below, LD(s.abs_len[0]), np.where(above, LD(s.abs_len[-1]), v0 + a * (v1 - v0)))
    e_L = np.abs(v1 - v0) * e_f + 4 * EPS * np.maximum(np.abs(v0), np.abs(v1))
    out.bin = np.where(below, -1, np.where(above, n - 1, t))
    out.outside = below | above
    amb = np.abs(f - np.rint(f)) <= e_f
    # conversion depth
    lnu = np.log(w01(w[2]))
    si = -L * lnu
    e_si = np.abs(lnu) * e_L + si * (LOG_ERR + 2 * EPS)
    out.clipped = np.zeros(len(k), dtype=bool)
    x0, y0 = x.copy(), y.copy()
    e_x, e_y = 4 * EPS * np.abs(x), 4 * EPS * np.abs(y)
    if has_angles:
        norm = np.sqrt(1 + dxdz * dxdz + dydz * dydz)
        dz_free = si / norm
        e_free = e_si / norm + 4 * EPS * dz_free
        out.clipped = dz_free > T - 1
        amb |= np.abs(dz_free - (T - 1)) <= e_free + EPS * T
        dz = np.where(out.clipped, T - 1, dz_free)
        e_dz = np.where(out.clipped, EPS * T, e_free)
        wx, wy = dxdz * dz / p, dydz * dz / p
        x0, y0 = x0 + wx, y0 + wy
        e_x = e_x + np.abs(dxdz) * e_dz / p + 8 * EPS * np.abs(wx)
        e_y = e_y + np.abs(dydz) * e_dz / p + 8 * EPS * np.abs(wy)
    else:
        dz, e_dz = si, e_si
    zconv = T - dz
    e_z = e_dz + EPS * T
    out.lost = zconv < 0
    amb |= np.abs(zconv) <= e_z
    zc = np.where(out.lost, LD(0), zconv)
    if s.diff_step != 0:
        sigma = np.maximum(LD(0), s.diff_step * np.sqrt(zc / T) / p)
        e_sigma = s.diff_step / p * (np.sqrt((zc + e_z) / T) - np.sqrt(np.maximum(zc - e_z, 0) / T)) + 8 * EPS * sigma
        g0, g1, rad = gauss_pair(w[0], w[1])
        for g, (pos, err) in ((g0, (x0, e_x)), (g1, (y0, e_y))):
            pos += sigma * g
            err += sigma * rad * DEVIATE_ERR + np.abs(g) * e_sigma + 8 * EPS * np.abs(g * sigma)
    out.x0, out.y0, out.e_x, out.e_y = x0, y0, e_x, e_y
    out.zconv, out.e_z = zconv, e_z
    out.zfactor = np.tanh(zc / ZFIT)
    out.e_zf = e_z / ZFIT + EPS * (8 + 4 * zc / ZFIT)
    out.ambiguous = amb
    return out


def convert_pool(sensor, seed, objects, pool, has_angles):
    """`convert` over an un-converted photon pool in pool order (object after object, photon phot_first + j).  sensor None, faint
    objects and photons that arrive without flux keep x and y: `kept`.  Returns a Converted whose arrays span the pool."""
    n = len(pool["x"])
    out = Converted()
    for name in ("x0", "y0", "zconv", "zfactor", "e_x", "e_y", "e_z", "e_zf"):
        setattr(out, name, np.zeros(n, dtype=LD))
    for name in ("coin", "lost", "clipped", "outside", "ambiguous"):
        setattr(out, name, np.zeros(n, dtype=bool))
    out.bin = np.full(n, -2)
    out.x0[:], out.y0[:], out.zfactor[:] = _ld(pool["x"]), _ld(pool["y"]), 1
    out.kept = np.ones(n, dtype=bool)
    pos = 0
    for o in objects:
        m = int(o["n_phot"])
        sl = slice(pos, pos + m)
        pos += m
        if sensor is None or int(o["flags"]) & OBJ_FAINT:
            continue
        k = int(o["phot_first"]) + np.arange(m, dtype=np.int64)
        c = convert(sensor, seed, int(o["obj_id"]), k, pool["x"][sl], pool["y"][sl], pool["dxdz"][sl], pool["dydz"][sl],
                    pool["wavelength"][sl], has_angles)
        live = pool["flux"][sl] != 0
        for name in ("x0", "y0", "zconv", "zfactor", "e_x", "e_y", "e_z", "e_zf", "coin", "lost", "clipped", "outside", "ambiguous", "bin"):
            getattr(out, name)[sl] = np.where(live, getattr(c, name), getattr(out, name)[sl])
        out.kept[sl] = ~live
    assert pos == n
    return out


# ---------------- tree rings ----------------
def natural_spline_m(table, dr):
    """second derivatives at the knots of the natural cubic spline through `table` on a uniform grid of step dr: m[0] = m[-1] = 0
    and m[i - 1] + 4 m[i] + m[i + 1] = 6 (y[i - 1] - 2 y[i] + y[i + 1]) / dr^2, solved by elimination in np.longdouble"""
    y = _ld(table)
    n = len(y)
    m = np.zeros(n, dtype=LD)
    if n < 3:
        return m
    rhs = 6 * (y[:-2] - 2 * y[1:-1] + y[2:]) / (LD(dr) * LD(dr))
    c, d = np.zeros(n - 2, dtype=LD), np.zeros(n - 2, dtype=LD)
    c[0], d[0] = LD(1) / 4, rhs[0] / 4
    for i in range(1, n - 2):
        den = 4 - c[i - 1]
        c[i], d[i] = 1 / den, (rhs[i] - d[i - 1]) / den
    m[n - 2] = d[n - 3]
    for i in range(n - 4, -1, -1):
        m[i + 1] = d[i] - c[i] * m[i + 2]
    return m


def spline_m_bound(table, dr):
    return (288 + 60 * (len(table) - 1)) * EPS * np.abs(_ld(table)).max() / (LD(dr) * LD(dr))


def tree_ring_shift(sensor, r, e_r=None):
    """f(r): zero unless 0 < r / dr < n - 1; the natural spline through tr_table with the second derivatives tr_table2, or the
    chord where tr_table2 is absent.  With e_r also returns (bound, ambiguous)."""
    s = sensor
    r = np.asarray(r, dtype=LD)
    if s.tr_table is None:
        z = np.zeros(r.shape, dtype=LD)
        return z if e_r is None else (z, z.copy(), np.zeros(r.shape, dtype=bool))
    n = len(s.tr_table)
    f = r / s.tr_dr
    inside = (f > 0) & (f < n - 1)
    i = np.clip(np.floor(f).astype(np.int64), 0, n - 2)
    b = f - i
    a = 1 - b
    v0, v1 = _ld(s.tr_table[i]), _ld(s.tr_table[i + 1])
    val, curv = a * v0 + b * v1, np.zeros(r.shape, dtype=LD)
    if s.tr_table2 is not None:
        h2 = s.tr_dr * s.tr_dr / 6
        m0, m1 = _ld(s.tr_table2[i]), _ld(s.tr_table2[i + 1])
        val = val + ((a * a * a - a) * m0 + (b * b * b - b) * m1) * h2
        curv = (np.abs(m0) + np.abs(m1)) * h2
    val = np.where(inside, val, LD(0))
    if e_r is None:
        return val
    e_f = e_r / s.tr_dr + EPS * f
    bound = (np.abs(v1 - v0) + 2 * curv) * e_f + 16 * EPS * (np.abs(v0) + np.abs(v1) + curv)
    amb = (np.abs(f - np.rint(f)) <= e_f) & (f < n - 1 + 2 * e_f) & (r > 0)
    return val, np.where(inside, bound, LD(0)), amb


def owned_nominal(sensor):
    """nominal local positions [2 nV + 2][2] of the points an owner cell owns: the lower-left corner, the bottom-row points, the
    lower-right corner, the left-edge points from the bottom up (the layout shapes_ref.polygons documents), read off the
    counter-clockwise polygon emptypoly (whose left edge runs from the top down)"""
    nV, e = sensor.nV, sensor.emptypoly
    return np.concatenate([e[0:nV + 2], e[4 * nV + 3:3 * nV + 3:-1]])


def owned_points(sensor, slot):
    """the initial state of a slot: (points [(ny + 1) (nx + 1)][2 nV + 2][2], bound of the same shape, ambiguous
    [cells][2 nV + 2]), owner cells row-major with x fastest"""
    xmin, ymin, nx, ny = (int(slot[f]) for f in ("xmin", "ymin", "nx", "ny"))
    e = _ld(owned_nominal(sensor))                                   # [npo][2]
    cj, ci = np.mgrid[0:ny + 1, 0:nx + 1]
    qx = (_ld(xmin + ci.ravel()) - LD(0.5))[:, None] + e[None, :, 0]
    qy = (_ld(ymin + cj.ravel()) - LD(0.5))[:, None] + e[None, :, 1]
    tx, ty = qx - sensor.tr_center[0], qy - sensor.tr_center[1]
    e_t = EPS * np.maximum(2 * np.abs(qx) + np.abs(tx), 2 * np.abs(qy) + np.abs(ty))
    r = np.sqrt(tx * tx + ty * ty)
    e_r = np.sqrt(LD(2)) * e_t + 3 * EPS * r
    sh, e_s, amb = tree_ring_shift(sensor, r, e_r)
    rr = np.where(r > 0, r, LD(1))
    pts = np.stack([e[None, :, 0] + np.where(r > 0, sh * tx / rr, 0), e[None, :, 1] + np.where(r > 0, sh * ty / rr, 0)], axis=-1)
    bound = e_s + np.abs(sh) * (2 * e_t / rr + 6 * EPS) + 2 * EPS
    return pts, np.repeat(bound[..., None], 2, axis=-1), amb


# ---------------- the assertions both test files use ----------------
def _ratio(err, bound):
    return np.where(err == 0, LD(0), err / np.where(bound > 0, bound, LD(1e-300)))


def report(what, worst, ratios):
    if ratios is not None:
        for f, v in worst.items():
            ratios[f] = max(ratios.get(f, 0.0), v)
    print(f"{what}: error / bound " + " ".join(f"{f}={v:.3g}" for f, v in worst.items()))
    bad = {f: v for f, v in worst.items() if not v <= 1.0}
    assert not bad, f"{what}: error exceeds the bound: {bad}"


def assert_matches(conv, got, flux_in, what, ratios=None):
    """got: the converted pool {x, y, flux, dxdz} (ims_photons_t.converted); flux_in: the flux of the un-converted pool.
    Unambiguous photons only (share asserted first): coin and lost exactly, x, y, zfactor within the bounds; kept photons keep
    x, y and flux bit for bit."""
    n = len(conv.x0)
    assert conv.ambiguous.sum() <= EDGE_SHARE_CAP * n, f"{what}: {conv.ambiguous.sum()} of {n} photons ambiguous"
    for f in ("x", "y", "flux", "dxdz"):
        assert np.asarray(got[f]).shape == (n,) and np.all(np.isfinite(got[f])), f"{what}: {f}"
    kept = conv.kept
    assert np.array_equal(got["x"][kept], conv.x0[kept].astype(np.float64)) and np.array_equal(got["y"][kept], conv.y0[kept].astype(np.float64))
    assert np.array_equal(got["flux"][kept], flux_in[kept]), f"{what}: flux of photons the sensor does not convert"
    ok = ~kept & ~conv.ambiguous
    lost = got["flux"] == 0
    assert np.array_equal(lost[ok], conv.lost[ok]), f"{what}: {(lost[ok] != conv.lost[ok]).sum()} photons lost on one side only"
    assert np.array_equal(got["flux"][ok & ~lost], flux_in[ok & ~lost]), f"{what}: flux changed"
    live = ok & ~conv.lost
    assert np.array_equal(np.signbit(got["dxdz"][live]), conv.coin[live]), f"{what}: coin"
    worst = {}
    for name, value, refv, bound in (("x", got["x"], conv.x0, conv.e_x), ("y", got["y"], conv.y0, conv.e_y),
                                     ("zfactor", np.abs(got["dxdz"]), conv.zfactor, conv.e_zf)):
        r = _ratio(np.abs(_ld(value) - refv)[live], bound[live])
        worst[name] = float(r.max()) if r.size else 0.0
    report(what, worst, ratios)
    return worst


def assert_points(sensor, slot, boundary, what, ratios=None):
    """boundary: the f64 boundary array of all slots; the slot's unambiguous points against `owned_points`.  Returns the slot's
    points [cells][npo][2] and the number of ambiguous ones (the caller caps their share over the case)"""
    pts, bound, amb = owned_points(sensor, slot)
    npo = 2 * sensor.nV + 2
    cells = pts.shape[0]
    off = int(slot["offset"])
    got = np.asarray(boundary, dtype=np.float64)[off * npo * 2:(off + cells) * npo * 2].reshape(cells, npo, 2)
    assert np.all(np.isfinite(got)), what
    keep = ~amb
    worst = {}
    for ax, name in ((0, "point_x"), (1, "point_y")):
        r = _ratio(np.abs(_ld(got[..., ax]) - pts[..., ax])[keep], bound[..., ax][keep])
        worst[name] = float(r.max()) if r.size else 0.0
    report(what, worst, ratios)
    return got, int(amb.sum())
