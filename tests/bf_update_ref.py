"""Silicon's updatePixelDistortions (the move of the pixel boundaries between two brighter-fatter rounds) and the bounds lines
behind it, restated as an exact scatter over pixel polygons in plain Python / numpy.  It shares no code with the kernels
(k_update_distortions, k_update_distortions_q3 in its three table forms, k_refresh_changed) or with oracle/orc_silicon.c, which are
gathers over owner cells: the sensor-model files are read by the reader of tests/test_independent_fill.py, and the vertex ->
(owner cell, owned point) map is read off shapes_ref.polygons, which the shape tests hold against the device.

The rule ("distortion[dx, dy, vertex] q / NumElect" for the pixels around a charged one, "boundary points
are stored in shared horizontal / vertical arrays (each edge owned once)"; nothing under tests/golden/ records a boundary state,
so no golden decides it -- it is the recalled layout of GalSim's Silicon):

* The plane is a lattice of pixel polygons of 4 nV + 4 vertices.  Every edge is stored once, with the polygon whose BOTTOM row
  (both corners included) or LEFT edge (corners excluded) it is: a horizontal edge with the pixel above it, a vertical edge with
  the pixel to its right.  The lower-right corner of a pixel and the lower-left corner of its right neighbour are the same place
  but two stored points, one in each bottom row.  A slot of nx x ny pixels stores the (nx + 1) x (ny + 1) lattice cells that hold
  an edge of one of its pixels; the table belongs to the lattice, not to the slot, so the cells i == nx and j == ny move like any
  other (their polygons merely are no pixels of the slot, and can hold no charge).
* A charged pixel (si, sj) with w = charge / num_elec (the one quantity taken as the correctly rounded double) reaches the
  polygons (pi, pj) with |pi - si| <= qdist and |pj - sj| <= qdist, and moves every vertex k of each of them ONCE, by
  table[pi - si, pj - sj, k] w of the polygon that STORES the vertex.  A vertex of a reached polygon that is stored with a
  neighbour (its right edge, its top row) is therefore moved by the neighbour's entry for the same place -- by the neighbour's own
  visit when the neighbour is reached too, and otherwise (the far rim of the reach: this is the "extra row and column") on the
  visit of the reached polygon.  Where the storing neighbour lies beyond the tabulated stamp (qdist = 4 with the 9 x 9 files)
  there is no such entry, and the vertex moves by the reached polygon's own entry.
* `changed` of a cell: a charged pixel reaches one of the four polygons around the cell's lattice corner.

Arithmetic: doubles are dyadic rationals, so every table entry, weight and point becomes a Python integer at a common power-of-two
scale; products and sums are exact, and a point is rounded to double once, at the end (Fraction -> float is correctly rounded).

Tolerance, derived: the kernels and the oracle add at most T FMAs in a fixed order onto p0.  Each FMA rounds once, relatively by
2^-53, a partial sum that never exceeds S = |p0| + sum |d_k w_k| (1 + T 2^-53); the reference's own rounding is one more
half-ulp.  So |got - exact| <= (T + 2) 2^-53 S per coordinate, asserted in exact integer arithmetic with no slack factor; a point
with T == 0 must come back bit for bit, the sign of a zero included.

Observed worst |got - exact| / bound over every case of tests/bf_update_cases.py (a ratio above 1 fails the test):

    run                                   points
    oracle (CPU)                          0.575
    MI355X, every form                    0.575
"""
import os
from fractions import Fraction

import numpy as np

import shapes_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 100                     # discriminating power: every tap moves its point by more than FACTOR bounds


class Model:
    """the tabulated displacements [nx][ny][4 nV + 4][2] (pixel units, per num_elec electrons in the stamp's centre pixel), read
    by the reader tests/test_independent_fill.py wrote for itself"""

    def __init__(self, name):
        from test_independent_fill import _read_model
        m = _read_model(os.path.join(ROOT, "imsim_amd", "data", "sensor_models", name))
        self.name, self.nV, self.nx, self.ny = name, m["nV"], m["nx"], m["ny"]
        self.table, self.num_elec, self.poly, self.raw = m["table"], m["num_elec"], m["poly"], m
        self.npo, self.nv = 2 * self.nV + 2, 4 * self.nV + 4


def vertex_map(nV):
    """[(dci, dcj, q)] per polygon vertex k: the vertex is owned point q of lattice cell (i + dci, j + dcj).  Read off
    shapes_ref.polygons by handing it a boundary array that holds its own indices."""
    npo = 2 * nV + 2
    slot = dict(xmin=0, ymin=0, nx=1, ny=1, offset=0)
    marks = 4.0 * np.arange(4 * npo)                                      # (multiples of 4: the unit shift of a neighbour shows)
    poly = shapes_ref.polygons(np.repeat(marks, 2), slot, nV, None, [0], [0])[0]
    out = []
    for x, y in poly:
        idx = int(min(x, y)) // 4
        cell, q = divmod(idx, npo)
        dcj, dci = divmod(cell, 2)
        assert (x - 4 * idx, y - 4 * idx) == (dci, dcj), "a neighbour's point is shifted by the neighbour's offset"
        out.append((dci, dcj, q))
    assert len(out) == 4 * nV + 4
    own = sorted(q for dci, dcj, q in out if (dci, dcj) == (0, 0))
    assert own == list(range(npo)), "a polygon holds each of its cell's owned points once"
    return out


def _scale(a):
    """smallest E with a 2^E integer for every double of a"""
    e = 0
    for v in np.asarray(a, dtype=np.float64).ravel().tolist():
        e = max(e, v.as_integer_ratio()[1].bit_length() - 1)
    return e


def _ints(a, e):
    """the doubles of a times 2^e as Python integers (exact; object array of a's shape)"""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.size, dtype=object)
    for k, v in enumerate(a.ravel().tolist()):
        n, d = v.as_integer_ratio()
        out[k] = n * ((1 << e) // d)
    return out.reshape(a.shape)


def visits(model, qdist):
    """what the visit of the polygon at (dx, dy) from a charged pixel moves: [(dx, dy, dci, dcj, q [n], tx [n], ty [n], k [n])] --
    owned points q of cell (pi + dci, pj + dcj) by table[tx, ty, k] (stamp indices)"""
    vm = vertex_map(model.nV)
    own_k = {q: k for k, (dci, dcj, q) in enumerate(vm) if (dci, dcj) == (0, 0)}
    cx, cy = (model.nx - 1) // 2, (model.ny - 1) // 2
    assert qdist <= min(cx, cy), "the reach lies inside the tabulated stamp"
    out = []
    for dy in range(-qdist, qdist + 1):
        for dx in range(-qdist, qdist + 1):
            groups = {}
            for k, (dci, dcj, q) in enumerate(vm):
                src = (dx + cx, dy + cy, k)
                if (dci, dcj) != (0, 0):
                    ox, oy = dx + dci, dy + dcj                           # the polygon that stores this vertex
                    if abs(ox) <= qdist and abs(oy) <= qdist:
                        continue                                         # reached itself: it moves the vertex on its own visit
                    if 0 <= ox + cx < model.nx and 0 <= oy + cy < model.ny:
                        src = (ox + cx, oy + cy, own_k[q])
                groups.setdefault((dci, dcj), []).append((q,) + src)
            for (dci, dcj), rows in groups.items():
                q, tx, ty, k = (np.array(c) for c in zip(*rows))
                out.append((dx, dy, dci, dcj, q, tx, ty, k))
    return out


class Result:
    """new [cells][npo][2] f64: the exactly rounded points; T [cells][npo]: charged taps that reach the point; S [cells][npo][2]:
    |p0| + sum |d w| (rounded, for reports); changed [cells] bool; exact: the sums and S as integers at scale 2^-K; min_tap: the
    smallest non-zero |d w| that reached the coordinate (integer at the same scale; None where there is none)"""


def update(model, qdist, nx, ny, points, delta):
    """one slot of nx x ny pixels: points [(ny + 1)(nx + 1)][npo][2] and delta [(ny + 1)(nx + 1)] as stored (row-major, x fastest)"""
    npo = model.npo
    cells = (nx + 1) * (ny + 1)
    p0 = np.asarray(points, dtype=np.float64).reshape(cells, npo, 2)
    delta = np.asarray(delta, dtype=np.float64).reshape(ny + 1, nx + 1)
    sj, si = np.nonzero(delta[:ny, :nx])                                  # charge sits in pixels; +0 and -0 are no charge
    w = delta[sj, si] / model.num_elec
    e_t, e_w = _scale(model.table), _scale(w)
    K = max(e_t + e_w, _scale(p0))
    tab = _ints(model.table, e_t)
    wi = _ints(w, e_w) * (1 << (K - e_t - e_w)) if len(w) else []
    acc = _ints(p0, K)
    S = np.abs(acc)
    T = np.zeros((cells, npo), dtype=np.int64)
    big = 1 << 4000
    min_tap = np.full((cells, npo, 2), big, dtype=object)
    changed = np.zeros((ny + 1, nx + 1), dtype=bool)
    vis = visits(model, qdist)
    for a in range(len(w)):
        i0, j0, wa = int(si[a]), int(sj[a]), wi[a]
        changed[max(j0 - qdist, 0):j0 + qdist + 2, max(i0 - qdist, 0):i0 + qdist + 2] = True     # corners of the reached polygons
        for dx, dy, dci, dcj, q, tx, ty, k in vis:
            ci, cj = i0 + dx + dci, j0 + dy + dcj
            if not (0 <= ci <= nx and 0 <= cj <= ny):
                continue
            c = cj * (nx + 1) + ci
            d = tab[tx, ty, k] * wa
            ad = np.abs(d)
            acc[c, q] += d
            S[c, q] += ad
            T[c, q] += 1
            min_tap[c, q] = np.minimum(min_tap[c, q], np.where(ad == 0, big, ad))
    out = Result()
    out.K, out.exact, out.S_exact, out.T, out.p0 = K, acc, S, T, p0
    out.changed = changed.ravel()
    new = p0.copy()
    Sf = np.abs(p0)
    den = 1 << K
    for c, q in zip(*np.nonzero(T)):
        for ax in (0, 1):
            new[c, q, ax] = float(Fraction(acc[c, q, ax], den))
            Sf[c, q, ax] = float(Fraction(S[c, q, ax], den))
    out.new, out.S = new, Sf
    out.min_tap = np.where(min_tap == big, None, min_tap)
    return out


def bound_of(res):
    """(T + 2) 2^-53 S per coordinate, as doubles (reports; the assertion is made on the integers)"""
    return (res.T[..., None] + 2) * 2.0 ** -53 * res.S


def check_points(res, got, what, ratios=None):
    """got [cells][npo][2]: points with T == 0 bit for bit p0, the others within (T + 2) 2^-53 S of the exact sum; returns and
    records the worst error / bound"""
    got = np.ascontiguousarray(got, dtype=np.float64).reshape(res.p0.shape)
    assert np.all(np.isfinite(got)), what
    still = res.T == 0
    same = got.view(np.int64) == np.ascontiguousarray(res.p0).view(np.int64)
    bad = still[..., None] & ~same
    assert not bad.any(), (f"{what}: {int(bad.sum())} coordinates that no charge reaches changed, first (cell, point, axis) "
                           f"{np.argwhere(bad)[:4].tolist()}: {got[bad][:4]} was {res.p0[bad][:4]}")
    worst, where = Fraction(0), None
    den = 1 << res.K
    for c, q in zip(*np.nonzero(res.T)):
        for ax in (0, 1):
            err = abs(Fraction(float(got[c, q, ax])) - Fraction(res.exact[c, q, ax], den))
            if err == 0:
                continue
            r = err * (1 << 53) * den / ((int(res.T[c, q]) + 2) * res.S_exact[c, q, ax])
            if r > worst:
                worst, where = r, (int(c), int(q), ax)
    w = float(worst)
    if ratios is not None:
        ratios["points"] = max(ratios.get("points", 0.0), w)
    print(f"{what}: worst error / bound {w:.3g}" + (f" at (cell, point, axis) {where}" if where else ""))
    assert worst <= 1, (f"{what}: (cell, point, axis) {where}: got {got[where]!r}, exact {res.new[where]!r}, was {res.p0[where]!r}, "
                        f"T {int(res.T[where[:2]])}, error / bound {w:.4g}")
    return w


def weakest_tap(res):
    """discriminating power: the smallest (non-zero tap) / bound over the coordinates a tap reaches, with its place"""
    worst, where = None, None
    den53 = 1 << 53
    for c, q in zip(*np.nonzero(res.T)):
        for ax in (0, 1):
            m = res.min_tap[c, q, ax]
            if m is None:
                continue
            r = Fraction(m * den53, (int(res.T[c, q]) + 2) * res.S_exact[c, q, ax])
            if worst is None or r < worst:
                worst, where = r, (int(c), int(q), ax)
    return (float(worst) if worst is not None else np.inf), where


def bounds_lines(boundary, slot, nV, emptypoly):
    """[ny nx][8] per pixel of the slot, from whatever points `boundary` (the array of all slots) holds: the inner rectangle of
    shapes_ref.inner_bounds (x0, x1, y0, y1) and the outer one (plain min / max of the vertices with the unit square)"""
    _, _, nx, ny, _ = shapes_ref.slot_view(slot)
    jj, ii = np.mgrid[0:ny, 0:nx]
    p = shapes_ref.polygons(boundary, slot, nV, emptypoly, ii.ravel(), jj.ravel())
    x0, x1, y0, y1 = shapes_ref.inner_bounds(p, nV)
    return np.stack([x0, x1, y0, y1, np.minimum(0.0, p[..., 0].min(axis=1)), np.maximum(1.0, p[..., 0].max(axis=1)),
                     np.minimum(0.0, p[..., 1].min(axis=1)), np.maximum(1.0, p[..., 1].max(axis=1))], axis=1)


def stored_lines(bounds, slot):
    """the [ny nx][8] lines of a slot's pixels out of the bounds array of all slots (one line per owner cell)"""
    _, _, nx, ny, off = shapes_ref.slot_view(slot)
    b = np.asarray(bounds, dtype=np.float64)[off * 8:(off + (nx + 1) * (ny + 1)) * 8]
    return b.reshape(ny + 1, nx + 1, 8)[:ny, :nx].reshape(-1, 8)


def slot_points(boundary, slot, npo):
    _, _, nx, ny, off = shapes_ref.slot_view(slot)
    cells = (nx + 1) * (ny + 1)
    return np.asarray(boundary, dtype=np.float64)[off * npo * 2:(off + cells) * npo * 2].reshape(cells, npo, 2)


def slot_cells(a, slot):
    _, _, nx, ny, off = shapes_ref.slot_view(slot)
    return np.asarray(a)[off:off + (nx + 1) * (ny + 1)]
