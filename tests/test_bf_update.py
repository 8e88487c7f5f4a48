"""The brighter-fatter boundary update against an exact, independent scatter (tests/bf_update_ref.py), on the CPU: the reference
checks itself (teeth, linearity, locality, discriminating power of the cases), then holds oracle/orc_silicon.c -- the same gather
as the kernels, line for line -- to the cases and assertions the GPU file uses (tests/test_bf_update_gpu.py).

measured (CPU): worst |oracle - exact| / bound over every case and field: 0.575 (a ratio above 1 fails); the weakest tap of any
case moves its point by 3.1e6 (the dense field) bounds (at least bf_update_ref.FACTOR = 100 is asserted)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bf_update_cases as cases
import bf_update_ref as ref
from helpers import assert_bits_equal

RATIOS = {}


@functools.lru_cache(maxsize=None)
def model(name):
    return ref.Model(name)


def synthetic_points(m, nx, ny):
    """initial points made here: the nominal places of a cell's owned points plus a smooth shift of a few 1e-3 pixel"""
    own_k = {q: k for k, (dci, dcj, q) in enumerate(ref.vertex_map(m.nV)) if (dci, dcj) == (0, 0)}
    nominal = np.array([m.poly[own_k[q]] for q in range(m.npo)])
    c = np.arange((nx + 1) * (ny + 1))[:, None, None]
    q = np.arange(m.npo)[None, :, None]
    ax = np.arange(2)[None, None, :]
    return nominal[None] + 0.003 * np.sin(0.37 * c + 0.11 * q + 1.3 * ax + 0.2)


# ---------------- the comparison both files make ----------------
def assert_lines(stored, lines, what):
    for k, name in enumerate(("inner x0", "inner x1", "inner y0", "inner y1", "outer x min", "outer x max", "outer y min", "outer y max")):
        assert_bits_equal(stored[:, k], lines[:, k], f"{what}: {name}")


def check_update(c, delta, before, boundary, bounds, delta_after, changed, what, ratios):
    """one launch: `before` / `boundary` are the point arrays of all regions before and after it, `delta` the charge it consumed.
    Points of the launch's slots within the bound of the reference applied to `before` (bit for bit where no charge reaches);
    every other region bit for bit; `changed` (None: not kept) the reference's flags on every owner cell; every pixel's bounds
    line the rectangles of the points in `boundary`; no charge left.  Returns {slot: bf_update_ref.Result}."""
    m = model(c.model)
    sl = cases.slots(c)
    out = {}
    before, boundary = np.asarray(before, dtype=np.float64), np.asarray(boundary, dtype=np.float64)
    for s, slot in enumerate(sl):
        if not c.first_slot <= s < c.first_slot + c.n_slots:
            assert_bits_equal(ref.slot_points(boundary, slot, m.npo).ravel(), ref.slot_points(before, slot, m.npo).ravel(),
                              f"{what}: region {s} is not in the launch")
            continue
        res = ref.update(m, c.qdist, slot["nx"], slot["ny"], ref.slot_points(before, slot, m.npo), ref.slot_cells(delta, slot))
        ref.check_points(res, ref.slot_points(boundary, slot, m.npo), f"{what} slot {s}", ratios)
        if changed is not None:
            got = ref.slot_cells(changed, slot) != 0
            assert np.array_equal(got, res.changed), f"{what} slot {s}: changed flags differ at cells {np.flatnonzero(got != res.changed)[:8]}"
        assert_lines(ref.stored_lines(bounds, slot), ref.bounds_lines(boundary, slot, m.nV, m.poly), f"{what} slot {s}")
        assert not ref.slot_cells(delta_after, slot).any(), f"{what} slot {s}: delta charge left"
        out[s] = res
    return out


# ---------------- the oracle, fed by a sensor block assembled here ----------------
class OracleState:
    def __init__(self, c):
        from imsim_amd import _abi
        from imsim_amd._abi import BFSLOT_DTYPE
        from oracle import orc_loader
        m = model(c.model)
        self.lib, self.keep = orc_loader.load(), []
        S = _abi.Sensor()
        S.kind, S.num_vertices, S.nx, S.ny, S.qdist = _abi.IMS_SENSOR_SILICON, m.nV, m.nx, m.ny, c.qdist
        S.num_elec, S.pixel_size, S.thickness, S.diff_step = m.num_elec, m.raw["pix"], m.raw["thick"], m.raw["diff_step"]
        S.n_abs, S.abs_wl_min, S.abs_wl_step = 2, 300.0, 800.0
        S.abs_len = self.ptr([1.0, 1.0])
        S.n_tr, S.tr_dr, S.tr_cx, S.tr_cy = len(cases.TR_TABLE), cases.TR_DR, cases.TR_CENTER[0], cases.TR_CENTER[1]
        S.tr_table, S.distortions, S.emptypoly = self.ptr(cases.TR_TABLE), self.ptr(m.table), self.ptr(m.poly)
        off, total = cases.offsets(c)
        slots = np.zeros(len(c.regions), dtype=BFSLOT_DTYPE)
        for k, (x, y, nx, ny) in enumerate(c.regions):
            slots[k] = (x, y, nx, ny, off[k])
        self.keep.append(slots)
        S.n_bf_slots, S.bf_slots = len(slots), slots.ctypes.data
        self.boundary, self.bounds, self.delta = np.zeros(total * m.npo * 2), np.zeros(total * 8), np.zeros(total)
        S.bf_boundary, S.bf_bounds, S.bf_delta = self.boundary.ctypes.data, self.bounds.ctypes.data, self.delta.ctypes.data
        S.pristine_margin = -1.0
        self.S = S
        self.lib.orc_sensor_init_boundaries(C.addressof(S), 0, len(slots))

    def ptr(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.keep.append(a)
        return a.ctypes.data

    def update(self, first_slot, n_slots):
        self.lib.orc_sensor_update_distortions(C.addressof(self.S), first_slot, n_slots)


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """every field of a case through the oracle, one after the other on the same state -> [{slot: Result}] per field"""
    c = cases.case(name)
    o = OracleState(c)
    m = model(c.model)
    corner = o.boundary.reshape(-1, m.npo, 2)[:, 0]                 # the lower-left corners: nominally (0, 0)
    assert 1e-4 < np.abs(corner).max() < 0.05, "the initial points carry a tree-ring shift"
    out = []
    for k, field in enumerate(c.fields):
        before = o.boundary.copy()
        delta = cases.delta_of(c, field)
        o.delta[:] = delta
        o.update(c.first_slot, c.n_slots)
        out.append(check_update(c, delta, before, o.boundary, o.bounds, o.delta, None, f"{name} field {k}", RATIOS))
    return out


@pytest.mark.parametrize("name", cases.NAMES)
def test_oracle_update_matches_the_reference(name):
    """points within (T + 2) 2^-53 S of the exact sum, untouched points bit for bit, delta cleared, bounds lines exact.
    measured: worst error / bound 0.575"""
    results = oracle_case(name)
    assert len(results) == len(cases.case(name).fields) and all(r for r in results)
    assert any(res.T.any() for r in results for res in r.values())
    print("worst so far:", {f: float(f"{v:.3g}") for f, v in RATIOS.items()})


@pytest.mark.parametrize("name", cases.NAMES)
def test_cases_have_discriminating_power(name):
    """on the reference alone: every tap with a non-zero table entry moves its point by more than FACTOR bounds, so a kernel that
    takes one tap of one form from the wrong place cannot pass"""
    worst = np.inf
    for k, r in enumerate(oracle_case(name)):
        for s, res in r.items():
            ratio, where = ref.weakest_tap(res)
            worst = min(worst, ratio)
            if (name, k) not in cases.EXCEPTIONS:
                assert ratio > ref.FACTOR, f"{name} field {k} slot {s}: a tap moves (cell, point, axis) {where} by {ratio:.3g} bounds only"
    print(f"{name}: the weakest tap moves its point by {worst:.3g} bounds")


def test_case_catalogue_holds_what_it_is_for():
    c = cases.case("sparse_50x40_itl4")
    res = oracle_case(c.name)[0][0]
    ch = res.changed.reshape(41, 51)
    n = sum(len(v) for v in c.fields[0].values())
    assert 0.02 * 2000 <= n <= 0.05 * 2000
    assert not ch[:, 48:].any() and not ch[12:16, :16].any() and ch[:12, :16].any(), "a tile and a wavefront's rows without charge in reach"
    assert ch[16:, :32].any() and not ch.all()
    assert cases.tiles(cases.case("impulses_33x47_e2v4")) == 9 and cases.tiles(cases.case("three_regions_e2v4")) == 7
    assert all(cases.tiles(cases.case(n)) <= 64 for n in cases.NAMES if n != "many_regions_itl4")
    assert 65 <= cases.tiles(cases.case("many_regions_itl4")) <= 128
    dense = oracle_case("dense_20x36_e2v4")[0][0]
    assert dense.changed.all() and dense.T.max() == 56
    assert [model(cases.case(n).model).nV for n in cases.GENERIC] == [32, 4, 8] and [cases.case(n).qdist for n in cases.GENERIC] == [3, 2, 4]
    assert {model(cases.case(n).model).nV for n in cases.Q3_FAST} == {4, 8}
    # the pair of opposite sign: a point between the two pixels moves by far less than either contribution
    pair = oracle_case("fractional_and_opposite_24x20_e2v8")[1][0]
    moved = np.abs(pair.new - pair.p0)
    each = pair.S - np.abs(pair.p0)
    assert ((pair.T == 2)[..., None] & (moved < 1e-3 * each) & (each > 1e-7)).any()


# ---------------- the reference alone ----------------
def _impulse(m, q=3, nx=20, ny=20, at=((9, 9, 1003.0),)):
    p0 = synthetic_points(m, nx, ny)
    d = np.zeros((ny + 1, nx + 1))
    for i, j, e in at:
        d[j, i] = e
    return p0, d, ref.update(m, q, nx, ny, p0, d)


def test_vertex_map_and_reference_on_one_impulse():
    """by hand: the charged pixel's own bottom row moves by the centre entry's bottom vertices, its top row -- stored with the pixel
    above -- by that pixel's entry, and both ends of the reach by the rule of the far rim"""
    m = model("lsst_e2v_50_4")
    nV, cx = m.nV, 4
    p0, d, res = _impulse(m)
    w = 1003.0 / m.num_elec
    c = lambda i, j: j * 21 + i
    np.testing.assert_allclose(res.new[c(9, 9), :nV + 2] - p0[c(9, 9), :nV + 2], m.table[cx, cx, :nV + 2] * w, rtol=1e-9, atol=1e-16)
    np.testing.assert_allclose(res.new[c(9, 10), :nV + 2] - p0[c(9, 10), :nV + 2], m.table[cx, cx + 1, :nV + 2] * w, rtol=1e-9, atol=1e-16)
    # the far rim: the top row of the last reached pixel (9, 12) is stored with (9, 13) and moves by (9, 13)'s entry
    np.testing.assert_allclose(res.new[c(9, 13), :nV + 2] - p0[c(9, 13), :nV + 2], m.table[cx, cx + 4, :nV + 2] * w, rtol=1e-9, atol=1e-16)
    assert np.all(res.T[c(9, 13), :nV + 2] == 1) and np.all(res.T[c(9, 13), nV + 2:] == 0) and np.all(res.T[c(9, 14)] == 0)
    assert np.all(res.T[c(13, 9), nV + 2:] == 1) and np.all(res.T[c(13, 9), :nV + 2] == 0) and np.all(res.T[c(13, 13)] == 0)
    assert ref.check_points(res, res.new, "the reference's own output") <= 1.0 / 3.0           # its one rounding: half an ulp of a value below S, over (1 + 2) 2^-53 S


def test_teeth():
    """the reference rejects numpy-made corruptions of its own exact output"""
    m = model("lsst_e2v_50_4")
    nV, cx, q = m.nV, 4, 3
    p0, d, res = _impulse(m, at=((9, 9, 1003.0), (12, 12, 1409.0)))
    w, w2 = 1003.0 / m.num_elec, 1409.0 / m.num_elec
    c = lambda i, j: j * 21 + i
    own_k = {qq: k for k, (dci, dcj, qq) in enumerate(ref.vertex_map(nV)) if (dci, dcj) == (0, 0)}

    def rejected(bad, what):
        with pytest.raises(AssertionError):
            ref.check_points(res, bad, what)

    # a tap taken from the neighbouring column: cell (11, 5) sees only the first charge, at (di, dj) = (2, -4) ... use (2, -3)
    cell = c(11, 6)
    assert res.T[cell, 2] == 1
    bad = res.new.copy()
    bad[cell, 2] = p0[cell, 2] + m.table[cx + 3, cx - 3, 2] * w
    assert np.any(m.table[cx + 3, cx - 3, 2] != m.table[cx + 2, cx - 3, 2])
    rejected(bad, "neighbouring column")
    # the extra column applied to bottom-row points: cell (13, 6) is the extra column of the first charge alone
    cell = c(13, 6)
    assert np.all(res.T[cell, :nV + 2] == 0) and np.all(res.T[cell, nV + 2:] == 1)
    bad = res.new.copy()
    bad[cell, :nV + 2] += m.table[cx + 4, cx - 3, :nV + 2] * w
    rejected(bad, "extra column on the bottom row")
    # the left edge's vertex order reversed
    cell = c(10, 8)
    bad = res.new.copy()
    bad[cell, nV + 2:] = p0[cell, nV + 2:] + (res.new[cell, nV + 2:] - p0[cell, nV + 2:])[::-1]
    rejected(bad, "left edge reversed")
    # one far tap dropped: cell (9, 9) is at (-3, -3) of the second charge
    cell = c(9, 9)
    assert res.T[cell, 1] == 2 and np.all(m.table[cx - 3, cx - 3, own_k[1]] != 0)
    bad = res.new.copy()
    bad[cell, 1] -= m.table[cx - 3, cx - 3, own_k[1]] * w2
    rejected(bad, "far tap dropped")
    # and by less than the largest corruption above: half a bound passes, two bounds do not
    bad = res.new.copy()
    bad[cell, 1] += 0.4 * ref.bound_of(res)[cell, 1]
    ref.check_points(res, bad, "inside the bound")
    bad[cell, 1] += 2.0 * ref.bound_of(res)[cell, 1]
    rejected(bad, "two bounds off")
    # a bounds line left stale for a pixel whose right neighbour's cell moved while its own did not: column 5, left of the reach
    slot = dict(xmin=1, ymin=1, nx=20, ny=20, offset=0)
    old, new = ref.bounds_lines(p0.ravel(), slot, nV, m.poly), ref.bounds_lines(res.new.ravel(), slot, nV, m.poly)
    assert_lines(new, new, "the reference's own lines")
    rows = [j for j in range(6, 13) if not res.T[c(5, j)].any() and res.T[c(6, j)].any() and not res.T[c(5, j + 1)].any()
            and not np.array_equal(old[j * 20 + 5], new[j * 20 + 5])]
    assert rows, "a right neighbour's left edge decides a rectangle of some pixel of the column"
    for j in rows:
        stale = new.copy()
        stale[j * 20 + 5] = old[j * 20 + 5]
        with pytest.raises(AssertionError):
            assert_lines(stale, new, "stale line")


def test_linearity_and_locality():
    m = model("lsst_itl_50_8")
    rng = np.random.default_rng(3)
    nx, ny, q = 22, 19, 3
    p0 = synthetic_points(m, nx, ny)
    A, B = np.zeros((ny + 1, nx + 1)), np.zeros((ny + 1, nx + 1))
    for k in range(16):
        (A if k % 2 else B)[rng.integers(0, ny), rng.integers(0, nx)] = 900.0 + 41 * k
    B[A != 0] = 0
    both = ref.update(m, q, nx, ny, p0, A + B)
    first = ref.update(m, q, nx, ny, p0, A)
    second = ref.update(m, q, nx, ny, first.new, B)
    assert np.array_equal(both.T, first.T + second.T)
    assert np.all(np.abs(second.new - both.new) <= ref.bound_of(first) + ref.bound_of(second))
    assert np.abs(both.new - p0).max() > 1e-5
    # an impulse moves no point farther than the model's reach from it, and flags the corners of the reached pixels
    for qd, name in ((2, "lsst_e2v_50_4"), (3, "lsst_e2v_50_4"), (4, "lsst_itl_50_8")):
        mm = model(name)
        p0, d, res = _impulse(mm, q=qd, at=((9, 10, 1117.0),))
        moved = (res.new != p0).any(axis=(1, 2)).reshape(21, 21)
        reach = np.zeros((21, 21), dtype=bool)
        reach[10 - qd:10 + qd + 2, 9 - qd:9 + qd + 2] = True
        assert np.array_equal(res.changed.reshape(21, 21), reach)
        corner = np.zeros((21, 21), dtype=bool)
        corner[10 + qd + 1, 9 + qd + 1] = True                     # the far corner cell holds no edge of a reached pixel
        assert np.array_equal(moved, reach & ~corner), qd
        assert res.T.max() == 1


def test_reach_beyond_the_stamp_is_refused():
    with pytest.raises(AssertionError):
        ref.visits(model("lsst_e2v_50_4"), 5)
