"""tests/opd_ref.py on its own (no GPU): closed forms, the frame check of the perturbed path, the basis, the flagged-share
conditions of every case of tests/opd_cases.py, the sensitivity of the comparison (mutations), and the rule of
opd.solve_normal for singular normal equations."""
import math

import numpy as np
import pytest

from imsim_amd import opd
import opd_cases
import opd_ref
from opd_ref import LD, EPS


def _one_mirror(nx, fields=((0.0, 0.0),), jmax=28, **kw):
    tel = opd_cases.one_mirror(**kw)
    return tel, opd_ref.compute(opd_cases.descriptor(tel), fields, 620.0, nx, tel.pupil_outer, "postel", tel.sphere_radius, "chief",
                                tel.eps, jmax)


def test_paraboloid_is_stigmatic_on_axis():
    res = opd_cases.reference(opd_cases.BY_NAME["one_mirror_nx17"])
    F = res.fields[0]
    fin = np.isfinite(F.opd)
    assert fin.sum() > 200
    assert np.all(np.abs(F.opd[fin]) <= F.bound[fin])          # zero, to the bound the GPU is held to
    assert F.bound[fin].max() < 1e-4


@pytest.mark.parametrize("dz", [1e-4, -1e-4])
def test_defocus_is_pure_z4(dz):
    """the coefficient of tests/test_opd_gpu.py::test_defocus_is_pure_z4"""
    _, res = _one_mirror(65, det_z=10.0 + dz)
    zk = res.fits[0].zk.astype(np.float64)
    expect = dz * 0.5 ** 2 * (1 - 0.2 ** 2) / (4 * math.sqrt(3) * 10.0 ** 2) * 1e9
    assert abs(zk[3] / expect - 1) < 5e-3 and np.sign(zk[3]) == np.sign(dz)
    assert np.abs(zk[4:]).max() <= 1e-2 * abs(zk[3])


def test_spherical_mirror_third_order():
    tel, res = _one_mirror(65, conic=0.0)
    m = res.fields[0].opd.astype(np.float64)
    X, Y, _ = opd_ref.grid(65, tel.pupil_outer)
    h = np.sqrt(X * X + Y * Y).astype(np.float64).reshape(65, 65)
    w = h ** 4 / (4 * 20.0 ** 3) * 1e9
    f = np.isfinite(m)
    resid = (m[f] - m[f].mean()) - (w[f] - w[f].mean())
    assert np.abs(resid).max() / np.ptp(w[f]) < 0.01
    assert (m[f & (h > 0.45)] > 0).all()                       # edge rays travel the shorter path


def test_rigid_tilt_equals_the_counter_rotated_field():
    """The whole one-mirror telescope turned about the stop centre, traced through surface frames (origin and rotation), gives
    each ray the hit and the path of the untilted telescope traced with the ray counter-rotated: lengths and positions are kept
    in telescope coordinates, whatever frame the surfaces sit in."""
    T = opd_ref.Tel(opd_cases.descriptor(opd_cases.one_mirror()))
    a, b = LD(2 * opd_cases.ARCMIN), LD(-1 * opd_cases.ARCMIN)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]], dtype=LD)
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]], dtype=LD)
    G = Rx @ Ry
    centre = np.array([0, 0, T.stop_z], dtype=LD)
    X, Y, _ = opd_ref.grid(9, 0.5)
    pos = np.stack([X, Y, np.full(len(X), T.stop_z)], axis=1)
    d = np.tile(opd_ref.field_direction(0.1 * opd_cases.DEG, 0.05 * opd_cases.DEG, "postel")[None, :], (len(X), 1))
    tilted = opd_ref.trace(T.rigidly_moved(G, centre), pos, d, LD(620.0))
    plain = opd_ref.trace(T, centre[None, :] + (pos - centre[None, :]) @ G, d @ G, LD(620.0))      # rows times G: G^T a
    ok = (tilted.status == 0) & (plain.status == 0)
    assert ok.sum() > 40 and np.array_equal(tilted.status, plain.status)
    back = centre[None, :] + (plain.hit - centre[None, :]) @ G.T
    assert np.all(np.abs(tilted.hit - back)[ok].max(axis=1) <= (tilted.hit_bound + plain.hit_bound)[ok])
    diff = (tilted.path - plain.path)[ok]                       # the two phase origins differ: one constant for all rays
    assert np.all(np.abs(diff - diff[0]) <= (tilted.bound + plain.bound)[ok] + (tilted.bound + plain.bound)[ok][0])
    # the check has teeth: with the hit left in the surface's frame the paths disagree by far more
    bad = opd_ref.trace(T.rigidly_moved(G, centre), pos, d, LD(620.0), mutate="local_frame")
    dbad = (bad.path - plain.path)[ok]
    assert np.abs(dbad - dbad[0]).max() > 1e3 * (tilted.bound + plain.bound)[ok].max()


@pytest.mark.parametrize("eps", [0.0, 0.612])
def test_basis_is_orthonormal_on_the_annulus(eps):
    """mean of Z_j Z_k over the annulus = delta_jk: Gauss-Legendre in r (exact for these polynomials), uniform azimuth grid"""
    gx, gw = np.polynomial.legendre.leggauss(40)
    r = eps + (1 - eps) * (gx + 1) / 2
    wr = gw * (1 - eps) / 2
    nt = 64
    th = 2 * np.pi * np.arange(nt) / nt
    R, T = np.meshgrid(r, th)
    W = (np.meshgrid(wr, th)[0] * R * (2 * np.pi / nt) / (np.pi * (1 - eps * eps))).ravel()
    Z, _ = opd_ref.Basis(66, eps)(opd_ref.lds((R * np.cos(T)).ravel()), opd_ref.lds((R * np.sin(T)).ravel()), 1.0)
    G = (Z * opd_ref.lds(W)[:, None]).T @ Z
    assert float(np.abs(G - np.eye(66)).max()) < 1e-12          # (the quadrature nodes are binary64)
    assert opd_ref.noll_sequence(11) == [(0, 0), (1, 1), (1, -1), (2, 0), (2, -2), (2, 2), (3, -1), (3, 1), (3, -3), (3, 3), (4, 0)]
    assert [opd_ref.noll_sequence(66)[j - 1] for j in (22, 37, 55, 56, 65, 66)] == [(6, 0), (8, 0), (9, -9), (10, 0), (10, -10),
                                                                                   (10, 10)]


def test_long_double_least_squares():
    rng = np.random.default_rng(11)
    A = opd_ref.lds(rng.standard_normal((40, 7)))
    z = opd_ref.lds(rng.standard_normal(7))
    got, sv = opd_ref.lstsq_min_norm(A, A @ z)
    assert float(np.abs(got - z).max()) < 1e-16
    assert np.allclose(np.sort(sv.astype(np.float64)), np.sort(np.linalg.svd(A.astype(np.float64), compute_uv=False)), rtol=1e-12)
    B = A[:4]                                                   # fewer rows than columns: the minimum-norm solution
    got, _ = opd_ref.lstsq_min_norm(B, B @ z)
    want = np.linalg.pinv(B.astype(np.float64)) @ (B @ z).astype(np.float64)
    assert np.abs(got.astype(np.float64) - want).max() < 1e-12


@pytest.mark.parametrize("case", opd_cases.CASES, ids=[c["name"] for c in opd_cases.CASES])
def test_flagged_share_and_rank_margins(case):
    """On the reference alone: no ray near a decision in any case (every case compares Zernike sums, several take the mean
    reference), the grids hold what the cases file says, and no singular value of A sits near the cut."""
    res = opd_cases.reference(case)
    share = opd_ref.flagged_share(res)
    assert share <= opd_ref.FLAG_CAP
    assert share == 0.0
    for fld, F, ft in zip(case["fields"], res.fields, res.fits):
        n_fin = int(np.isfinite(F.opd).sum())
        assert np.all(F.bound[np.isfinite(F.opd)] > 0) and np.all(F.bound[np.isfinite(F.opd)] < 5e-3)
        if fld == opd_cases.OUT:
            assert n_fin == 0 and np.all(F.status != 0) and not np.any(ft.zk) and not np.any(ft.ata) and ft.zk_bound == 0
            continue
        assert n_fin > 0.3 * case["nx"] ** 2
        sv = (ft.sv / ft.sv.max()).astype(np.float64)
        assert not np.any((sv > 1e-9) & (sv < 1e-2))
        assert ft.rank == min(n_fin, case["jmax"])
    if case["name"] == "rubin_nx5_rank_deficient":
        assert res.fits[0].rank < case["jmax"]


# mutation -> the case that catches it, and the quantity it shows in
TEETH = {"no_phase": ("one_mirror_nx17", "map"), "n_after": ("rubin_nx16_zemax", "map"), "local_frame": ("m2_nx15_mean", "map"),
         "s_sign": ("one_mirror_nx17", "map"), "no_sqrt2": ("rubin_nx15_gnomonic_mean", "zk"),
         "swap_projection": ("rubin_nx16_zemax", "map")}


@pytest.mark.parametrize("mutate", opd_ref.MUTATIONS)
def test_teeth(mutate):
    """a reference that is wrong in one of these ways differs from the right one by more than the bound the GPU is held to"""
    name, what = TEETH[mutate]
    case = opd_cases.BY_NAME[name]
    good, bad = opd_cases.reference(case), opd_cases.reference(case, mutate)
    worst = 0.0
    for F, B, ft, bt in zip(good.fields, bad.fields, good.fits, bad.fits):
        if what == "map":
            both = np.isfinite(F.opd) & np.isfinite(B.opd)
            if not np.array_equal(np.isfinite(F.opd), np.isfinite(B.opd)):
                worst = math.inf
            elif both.any():
                worst = max(worst, opd_ref.ratio(B.opd[both], F.opd[both], F.bound[both]))
        else:
            worst = max(worst, opd_ref.ratio(bt.zk, ft.zk, ft.zk_bound), opd_ref.ratio(bt.ata, ft.ata, ft.d_ata))
    print(f"{mutate} on {name}: {worst:.3g} bounds")
    assert worst > 1.0


def test_solve_normal_rule():
    """opd.solve_normal: zeros for the empty system, the minimum-norm solution for a rank-deficient one, the plain solution
    (within the binary64 solve's error) for a regular one; it never raises"""
    assert np.array_equal(opd.solve_normal(np.zeros((28, 28)), np.zeros(28)), np.zeros(28))
    ft = opd_cases.reference(opd_cases.BY_NAME["rubin_nx5_rank_deficient"]).fits[0]
    ata, atw = ft.ata.astype(np.float64), ft.atw.astype(np.float64)
    assert np.linalg.matrix_rank(ata) == ft.rank < len(atw)       # (np.linalg.solve raises on it, or returns garbage)
    got = opd.solve_normal(ata, atw)
    assert opd_ref.ratio(got, ft.zk, ft.zk_bound) <= 1.0
    ft = opd_cases.reference(opd_cases.BY_NAME["rubin_nx17_four_mean"]).fits[3]
    ata, atw = ft.ata.astype(np.float64), ft.atw.astype(np.float64)
    got = opd.solve_normal(ata, atw)
    assert opd_ref.ratio(got, ft.zk, ft.zk_bound) <= 1.0
    assert opd_ref.ratio(got, opd_ref.lds(np.linalg.solve(ata, atw)), ft.zk_bound) <= 1.0
