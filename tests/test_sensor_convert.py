"""The sensor's photon conversion and initial tree-ring state against an independent reference, on the CPU:
tests/sensor_convert_ref.py (plain numpy, np.longdouble) checks itself, then holds the oracle -- which shares its structure with
the kernels -- to the same cases and assertions the GPU file uses (tests/test_sensor_convert_gpu.py)."""
import numpy as np
import pytest

from helpers import assert_bits_equal
import sensor_convert_cases as cases
import sensor_convert_ref as ref
import shapes_ref
from photon_source_ref import EDGE_SHARE_CAP, EPS, LD

CONVERT, RINGS = cases.CONVERT_NAMES, cases.RING_NAMES
RATIOS = {}


def _toy_setup(table, table2, dr, center=(0.0, 0.0), slots=((1, 1, 4, 3),), model_name="lsst_e2v_50_4", abs_len=cases.ABS_LEN):
    from imsim_amd.engine import SensorSetup, make_slots
    return SensorSetup(model=cases.model(model_name), abs_wl=cases.ABS_WL, abs_len=abs_len, tr_table=table, tr_table2=table2,
                       tr_dr=dr, tr_center=center, slots=make_slots(list(slots)))


# ---------------- the reference alone ----------------
def test_spline_reproduces_a_cubic_with_zero_end_curvature():
    """s = x^3 - 3 x on [0, 1], mirrored about x = 1 on [1, 2]: cubic pieces, C2 at the knot (s' = 0, s'' = 6 there from both
    sides), s''(0) = s''(2) = 0 -- a natural spline, so the natural spline through its samples on a grid that holds the knot is s
    itself: second derivatives 6 x and 6 (2 - x), and its values between the nodes"""
    dr = 0.25
    x = np.arange(9) * dr
    fold = np.where(x <= 1, x, 2 - x)
    y = fold ** 3 - 3 * fold                                     # exact in double
    m = ref.natural_spline_m(y, dr)
    assert np.abs(m - 6 * fold).max() < 64 * EPS
    assert np.all(ref.natural_spline_m(2 * x - 1, dr) == 0)      # a straight line has no curvature
    s = ref.Sensor(_toy_setup(y, m.astype(np.float64), dr))
    assert np.all(ref.tree_ring_shift(s, x[1:8].astype(LD)) == y[1:8])          # interpolates its interior nodes
    xm = (np.arange(1, 64) * LD(2) / 64)
    fm = np.where(xm <= 1, xm, 2 - xm)
    assert np.abs(ref.tree_ring_shift(s, xm) - (fm ** 3 - 3 * fm)).max() < 64 * EPS
    # zero unless 0 < r / dr < n - 1: at the centre, at the last node, beyond it
    assert np.all(ref.tree_ring_shift(s, np.array([0, 2, 2.5, 1e4], dtype=LD)) == 0)
    # without second derivatives: the chord
    lin = ref.Sensor(_toy_setup(y, None, dr))
    assert abs(ref.tree_ring_shift(lin, LD(0.375)) - LD(y[1] + y[2]) / 2) < 4 * EPS


@pytest.mark.parametrize("nV,model_name", [(4, "lsst_e2v_50_4"), (8, "lsst_itl_50_8"), (32, "lsst_e2v_50_32")])
def test_owned_points_of_a_flat_table_are_the_empty_polygon(nV, model_name):
    from imsim_amd import sensor
    s = ref.Sensor(_toy_setup(np.zeros(5), np.zeros(5), 3.0, slots=((-2, 5, 3, 2),), model_name=model_name))
    pts, bound, amb = ref.owned_points(s, s.slots[0])
    e = sensor.empty_polygon(nV)
    owned = np.concatenate([e[:nV + 2], e[4 * nV + 3:3 * nV + 3:-1]])         # LL corner, bottom row, LR corner, left edge upwards
    assert owned.shape == (2 * nV + 2, 2) and np.all(owned[nV + 2:, 0] == 0) and np.all(np.diff(owned[nV + 2:, 1]) > 0)
    assert pts.shape == (4 * 3, 2 * nV + 2, 2) and np.all(pts == owned[None])
    # and the polygons shapes_ref assembles from that layout are the empty polygon, for every pixel
    poly = shapes_ref.polygons(pts.astype(np.float64).ravel(), s.slots[0], nV, e, [0, 2, 1], [0, 1, 0])
    assert np.abs(poly - e[None]).max() < 4 * float(EPS)


def test_convert_behind_a_transparent_sensor():
    """abs_len far above the thickness: every angle-free photon converts beyond the back (lost), every inclined one is clipped to
    zconv = 1 and walks (thickness - 1) slope / pixel_size"""
    s = ref.Sensor(_toy_setup(None, None, 3.0, abs_len=np.full(6, 1e12)))
    s.diff_step = LD(0)
    n = 5000
    k = np.arange(n) + 2 ** 32 - 50
    rng = np.random.default_rng(5)
    x, y = rng.uniform(1, 30, n), rng.uniform(1, 200, n)
    sx, sy, wl = rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), rng.uniform(560, 700, n)
    c = ref.convert(s, cases.SEED, 2 ** 40 + 7, k, x, y, sx, sy, wl, False)
    assert c.lost.all() and not c.clipped.any() and np.all(c.x0 == x) and np.all(c.y0 == y)
    c = ref.convert(s, cases.SEED, 2 ** 40 + 7, k, x, y, sx, sy, wl, True)
    assert c.clipped.all() and not c.lost.any() and np.all(c.zconv == 1)
    assert np.abs(c.x0 - (x + sx.astype(LD) * 99 / 10)).max() < 64 * EPS * 30
    assert np.abs(c.zfactor - np.tanh(LD(1) / 12)).max() < 4 * EPS
    assert 0.45 < c.coin.mean() < 0.55 and c.outside.any() and not c.outside.all()
    # the diffusion kick: sigma = diff_step sqrt(zconv / thickness) / pixel_size, cosine half to x
    s.diff_step = LD(5)
    d = ref.convert(s, cases.SEED, 2 ** 40 + 7, k, x, y, sx, sy, wl, True)
    kx, ky = (d.x0 - c.x0).astype(np.float64), (d.y0 - c.y0).astype(np.float64)
    assert abs(kx.std() - 0.05) < 0.003 and abs(ky.std() - 0.05) < 0.003 and abs(np.corrcoef(kx, ky)[0, 1]) < 0.05


# ---------------- the cases stay under the ambiguity cap (reference only) ----------------
@pytest.mark.parametrize("name", RINGS)
def test_ring_cases_stay_under_the_ambiguity_cap(name):
    case = cases.ring_case(name)
    s = case.ref_sensor()
    amb = total = 0
    for slot in s.slots:
        pts, _, a = ref.owned_points(s, slot)
        amb, total = amb + int(a.sum()), total + a.size
    assert amb <= EDGE_SHARE_CAP * total, f"{case.name}: {amb} of {total} points within the bound of a table interval's end"


# ---------------- the host's second derivatives ----------------
def test_uploaded_second_derivatives_are_the_natural_splines():
    """what the renderer uploads as tr_table2 for every case (and for the production table of R22_S11) against the tridiagonal
    solution in np.longdouble, within sensor_convert_ref.spline_m_bound (conditioning of tridiag(1, 4, 1) and the rounding of the
    host's nodes).  Largest difference seen: 880 eps max|y| / dr^2 on the production table (0.0055 of its bound), 16 eps max|y| /
    dr^2 over the hand-made tables; largest share of a bound 0.0113 (the four-point table)."""
    from imsim_amd import configs
    every = [cases.ring_case(n) for n in RINGS] + [cases.convert_case(n) for n in CONVERT]
    setups = [c.scene.sensor for c in every if c.scene.sensor is not None and c.scene.sensor.tr_table2 is not None]
    setups.append(configs.silicon_setup(64, 64))
    worst = 0.0
    for ss in setups:
        m = ref.natural_spline_m(ss.tr_table, ss.tr_dr)
        assert len(ss.tr_table2) == len(ss.tr_table) == len(m)
        worst = max(worst, float(np.abs(np.asarray(ss.tr_table2).astype(LD) - m).max() / ref.spline_m_bound(ss.tr_table, ss.tr_dr)))
    print(f"tr_table2 against the natural spline: worst difference / bound {worst:.3g}")
    assert worst <= 1.0


# ---------------- the oracle against the reference ----------------
def _check_bounds(bounds, boundary, slot, nV, empty, what):
    """the bounds lines of a slot are exactly the inner and outer rectangles of the polygons of the same boundary array"""
    xmin, ymin, nx, ny, off = shapes_ref.slot_view(slot)
    jj, ii = np.mgrid[0:ny, 0:nx]
    p = shapes_ref.polygons(boundary, slot, nV, empty, ii.ravel(), jj.ravel())
    b = bounds[off * 8:(off + (nx + 1) * (ny + 1)) * 8].reshape(ny + 1, nx + 1, 8)[:ny, :nx].reshape(-1, 8)
    for k, v in enumerate(shapes_ref.inner_bounds(p, nV)):
        assert_bits_equal(b[:, k], v, f"{what}: inner bound {k}")
    assert_bits_equal(b[:, 4], np.minimum(0.0, p[..., 0].min(axis=1)), f"{what}: outer x min")
    assert_bits_equal(b[:, 5], np.maximum(1.0, p[..., 0].max(axis=1)), f"{what}: outer x max")
    assert_bits_equal(b[:, 6], np.minimum(0.0, p[..., 1].min(axis=1)), f"{what}: outer y min")
    assert_bits_equal(b[:, 7], np.maximum(1.0, p[..., 1].max(axis=1)), f"{what}: outer y max")


def check_initial_state(case, boundary, bounds, what, ratios):
    """shared with the GPU file: every slot's points against owned_points, its bounds lines against its own points; returns the
    largest displacement of a point from its nominal place"""
    s = case.ref_sensor()
    ss = case.scene.sensor
    amb = total = 0
    moved = 0.0
    nominal = ref.owned_nominal(s)
    for k, slot in enumerate(s.slots):
        got, a = ref.assert_points(s, slot, boundary, f"{what} slot {k}", ratios)
        amb, total = amb + a, total + got.size // 2
        moved = max(moved, float(np.hypot(*np.moveaxis(got - nominal[None], -1, 0)).max()))
        _check_bounds(bounds, boundary, slot, s.nV, ss.model.emptypoly, f"{what} slot {k}")
    assert amb <= EDGE_SHARE_CAP * total
    assert moved > 0.02, "the rings moved nothing"
    return moved


@pytest.mark.parametrize("name", RINGS)
def test_oracle_initial_state_matches_the_reference(name):
    case = cases.ring_case(name)
    from oracle import orc_loader
    orc = orc_loader.OracleScene(case.scene)                     # (initialises every static slot)
    check_initial_state(case, orc.sensor_array("boundary"), orc.sensor_array("bounds"), case.name, RATIOS)
    n = case.scene.sensor.total_cells()
    assert not orc.sensor_array("delta")[:n].any()
    print("worst so far:", {f: float(f"{v:.3g}") for f, v in RATIOS.items()})


def search_pixels(case, conv, boundary, obj_index, flux):
    """shared with the GPU file: the reference's conversion through shapes_ref.pixel_search over `boundary` -> (pixel index or -1,
    ambiguous) per photon.  Ambiguous: the conversion's own flag, a position within its bound of a pixel's half-integer edge,
    or within the bound (at least 1e-12) of a polygon edge that decided the pixel."""
    sc = case.scene
    n = len(conv.x0)
    x0, y0 = conv.x0.astype(np.float64), conv.y0.astype(np.float64)
    stamps = shapes_ref.stamps_of(case.objects, obj_index)
    amb = conv.ambiguous.copy()
    for v, e in ((conv.x0, conv.e_x), (conv.y0, conv.e_y)):
        h = v + LD(0.5)
        amb |= np.abs(h - np.rint(h)) <= e + 2 * EPS * np.abs(h)
    want = np.full(n, -1, dtype=np.int64)
    ix, iy = np.floor(x0 + 0.5).astype(np.int64), np.floor(y0 + 0.5).astype(np.int64)
    sx0, sx1, sy0, sy1 = stamps
    lost = conv.lost | (flux == 0) | (ix < sx0) | (ix > sx1) | (iy < sy0) | (iy > sy1)
    sil = ~conv.kept
    if sil.any():
        w = np.flatnonzero(sil & ~conv.lost)
        s = case.ref_sensor()
        tol = max(1e-12, float(max(conv.e_x[w].max(), conv.e_y[w].max())) * 1.5) if w.size else 1e-12
        jx, jy, jl, ja = shapes_ref.pixel_search(boundary, s.slots[0], s.nV, sc.sensor.model.emptypoly, x0[w], y0[w],
                                                 conv.zfactor[w].astype(np.float64), conv.coin[w], tuple(v[w] for v in stamps), tol=tol)
        ix[w], iy[w], lost[w] = jx, jy, jl
        amb[w] |= ja
    px, py = ix - sc.xmin, iy - sc.ymin
    on = ~lost & (px >= 0) & (px < sc.nx) & (py >= 0) & (py < sc.ny)
    want[on] = py[on] * sc.nx + px[on]
    return want, amb


def assert_exercised(case, conv):
    """the case holds what it is for"""
    if case.scene.sensor is None:
        assert conv.kept.all()
        return
    live = ~conv.kept
    n = len(case.scene.sensor.abs_len)
    assert conv.kept.any(), "a faint object"
    assert (conv.outside & live & (conv.bin == -1)).any() and (conv.outside & live & (conv.bin == n - 1)).any()
    assert ((conv.bin == 0) & live).any() and ((conv.bin == n - 2) & live).any()
    if case.has_angles:
        assert (conv.clipped & live).sum() > 100 and not conv.lost.any()
    else:
        assert (conv.lost & live).sum() > 100 and not conv.clipped.any()
    assert 0.4 < conv.coin[live].mean() < 0.6


@pytest.mark.parametrize("name", CONVERT)
def test_oracle_pixels_are_the_reference_conversion_and_search(name):
    """the oracle keeps no converted pool: the reference converts the oracle's un-accumulated pool, shapes_ref.pixel_search puts
    every photon into a polygon of the oracle's boundary array, and the oracle's own pixel index must be that pixel"""
    from oracle import orc_loader
    case = cases.convert_case(name)
    orc = orc_loader.OracleScene(case.scene)
    pool = orc.shoot_pool(case.objects)
    orc.apply_ops(pool)
    g = pool.to_host()
    conv = ref.convert_pool(case.ref_sensor(), case.scene.seed, case.objects, g, case.has_angles)
    assert conv.ambiguous.sum() <= EDGE_SHARE_CAP * len(conv.x0), "the case's own inputs put too many photons on a threshold"
    assert_exercised(case, conv)
    pix = orc.accumulate(pool, want_pixel_index=True)
    boundary = orc.sensor_array("boundary") if case.scene.sensor is not None else None
    want, amb = search_pixels(case, conv, boundary, g["obj_index"], g["flux"])
    assert amb.sum() <= EDGE_SHARE_CAP * len(want), f"{case.name}: {amb.sum()} ambiguous photons"
    bad = (pix != want) & ~amb
    assert not bad.any(), (f"{case.name}: {int(bad.sum())} of {len(want)} photons in another pixel than the reference says, first "
                           f"{np.flatnonzero(bad)[:5]}: oracle {pix[bad][:5]} reference {want[bad][:5]}")
    assert (want >= 0).sum() > 0.3 * (~conv.lost).sum()


@pytest.mark.parametrize("name", [CONVERT[0], CONVERT[3]])
def test_oracle_coin_is_bit_31_of_word_3(name):
    """Neighbouring polygons share their points, so on a real state the search finds a pixel for all but a null set of photons
    and the coin never shows in an image.  Here the bounds lines of the oracle's state are overwritten so that no pixel holds
    anything (empty inner and outer rectangles): every photon of an interior pixel is then 'not found' and lands in its nominal
    pixel (coin set) or in the first neighbour the search visits (coin clear)"""
    from oracle import orc_loader
    case = cases.convert_case(name)
    orc = orc_loader.OracleScene(case.scene)
    orc.sensor_array("bounds").reshape(-1, 8)[:] = [1.0, 0.0, 1.0, 0.0, 2.0, -1.0, 2.0, -1.0]
    pool = orc.shoot_pool(case.objects)
    orc.apply_ops(pool)
    g = pool.to_host()
    conv = ref.convert_pool(case.ref_sensor(), case.scene.seed, case.objects, g, case.has_angles)
    pix = orc.accumulate(pool, want_pixel_index=True)
    sc = case.scene
    x0, y0 = conv.x0.astype(np.float64), conv.y0.astype(np.float64)
    ix, iy = np.floor(x0 + 0.5).astype(np.int64), np.floor(y0 + 0.5).astype(np.int64)
    x, y = conv.x0 - ix + LD(0.5), conv.y0 - iy + LD(0.5)
    e = np.maximum(conv.e_x, conv.e_y) * 2 + 8 * EPS
    near = (np.minimum(x, 1 - x) <= e) | (np.minimum(y, 1 - y) <= e) | (np.abs(x - y) <= e) | (np.abs(x - (1 - y)) <= e)
    step = np.where((x > y) & (x > 1 - y), 1, np.where((x > y) & (x < 1 - y), 7, np.where((x < y) & (x > 1 - y), 3, 5)))
    use = (~conv.kept & ~conv.lost & ~conv.ambiguous & ~near
           & (ix > sc.xmin) & (ix < sc.xmin + sc.nx - 1) & (iy > sc.ymin) & (iy < sc.ymin + sc.ny - 1))
    assert near.sum() <= EDGE_SHARE_CAP * len(near) and use.sum() > 2000
    nb = np.where(conv.coin, 0, step)
    want = (iy + shapes_ref.YOFF[nb] - sc.ymin) * sc.nx + (ix + shapes_ref.XOFF[nb] - sc.xmin)
    assert 0.4 < conv.coin[use].mean() < 0.6
    bad = use & (pix != want)
    assert not bad.any(), f"{case.name}: {int(bad.sum())} of {int(use.sum())} photons: the coin is not bit 31 of word 3"
