"""The oracle's operator chain against the independent reference of tests/photon_ops_ref.py on the planted pools of
tests/photon_ops_cases.py; the reference's own anchors; and the teeth of the comparison (the reference with one thing
miswritten must leave the bounds by a wide margin)."""
import math

import numpy as np
import pytest

import photon_ops_cases as cases
import photon_ops_ref as ref
from photon_ops_ref import LD

CASES = cases.plain_cases() + cases.rubin_cases(False)              # (the oracle is coaxial: the perturbed telescope runs on the device)
RATIOS = {}
_REF = {}


def reference(case):
    if case.name not in _REF:
        _REF[case.name] = case.reference()
    return _REF[case.name]


def oracle_pool(case):
    from imsim_amd.engine import segment_prefix
    from oracle import orc_loader
    orc = orc_loader.OracleScene(case.scene)
    objects = case.objects
    offs = np.concatenate([[0], np.cumsum(objects["n_phot"])]).astype(np.int64)
    pool = orc_loader.HostPool(offs[-1])
    pool.objects, pool.prefix, pool.offs = objects, segment_prefix(objects["n_phot"], case.scene.seg_size), offs
    for f in ref.FIELDS:
        pool.a[f][:pool.n] = case.pool[f]
    pool.obj_index[:pool.n] = case.obj_index()
    orc.apply_ops(pool)
    return pool.to_host()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_matches_the_reference(case):
    res = reference(case)
    assert ref.flagged_share(res) <= ref.FLAG_CAP, f"{case.name}: the planted inputs put {ref.flagged_share(res):.2e} of the photons near a decision"
    got = oracle_pool(case)
    ref.assert_matches(res, got, case.name, ratios=RATIOS)
    same = lambda f: got[f].tobytes() == case.pool[f].tobytes()
    if case.name == "focus_zero":
        assert same("x") and same("y")
    if case.name.startswith("dcr_"):
        still = np.repeat(case.objects["dcr_tanz"] == 0.0, case.objects["n_phot"])
        assert still.any() and np.array_equal(got["x"][still], case.pool["x"][still]) and np.array_equal(got["y"][still], case.pool["y"][still])
    if case.name.startswith("refraction_"):
        zero = (case.pool["dxdz"] == 0.0) & (case.pool["dydz"] == 0.0)
        assert zero.sum() > 100 and not got["dxdz"][zero].any() and not got["dydz"][zero].any()
    if case.name == "chain_faint":
        assert all(same(f) for f in ref.FIELDS if f != "flux") and not same("flux")
    if case.name == "ratio_t1_faint":
        assert all(same(f) for f in ref.FIELDS if f != "flux")
    if case.rubin and res.status.max() >= 0 and not case.name.startswith("chain"):      # (the chain draws its own pupil)
        assert (res.status == 2).sum() >= 2 and (res.status == 1).sum() >= 100, np.bincount(res.status[res.status >= 0])
    print("worst so far:", {f: float(f"{v:.3g}") for f, v in RATIOS.items()})


PERTURBED = cases.rubin_cases(True)


@pytest.mark.parametrize("case", PERTURBED, ids=[c.name for c in PERTURBED])
def test_perturbed_cases_on_the_reference_alone(case):
    """the oracle traces no perturbed telescope: here the reference's frames and figures run, the planted inputs keep the flagged
    share under the cap, and the statuses the issue asks for occur; the comparison itself is tests/test_photon_ops_ref_gpu.py"""
    res = reference(case)
    assert ref.flagged_share(res) <= ref.FLAG_CAP, f"{case.name}: {ref.flagged_share(res):.2e} of the photons near a decision"
    assert all(np.all(np.isfinite(res.fields[f].astype(np.float64))) and np.all(res.bounds[f] >= 0) for f in ref.FIELDS)
    if res.status.max() >= 0 and not case.name.startswith("chain"):
        assert (res.status == 2).sum() >= 2 and (res.status == 1).sum() >= 100, np.bincount(res.status[res.status >= 0])
    # the perturbation is visible: the coaxial twin of the case lands the traced photons elsewhere
    twin = reference(cases.by_name(case.name[:-len("_pert")]))
    ok = (res.status == 0) & (twin.status == 0)
    if ok.any():
        assert float(np.median(np.hypot(res.fields["x"] - twin.fields["x"], res.fields["y"] - twin.fields["y"])[ok])) > 0.1


# ---------------- the reference's own anchors ----------------
def test_edlen_anchor():
    """760 mmHg, 15 C, dry: the pressure / temperature factor is 1 (0.99999946 by hand), and (n - 1) 1e6 at 500 nm is 278.964:
    64.328 + 29498.1 / (146 - 4) + 255.4 / (41 - 4) = 64.328 + 207.7331 + 6.9027 = 278.9638"""
    P = 760.0 / 7.50061683
    factor = 760.0 * (1 + (1.049 - 0.0157 * 15.0) * 1e-6 * 760.0) / (720.883 * (1 + 0.003661 * 15.0))
    assert abs(factor - 0.99999946) < 1e-8
    n6 = float(ref.air_n_minus_one(np.array([LD(500)]), P, 288.15, 0.0)[0]) * 1e6
    assert abs(n6 - 278.964 * factor) < 5e-4
    # water vapour lowers the index: 10 mmHg at 500 nm by (0.0624 - 0.00068 * 4) * 10 / 1.054915 = 0.5657
    wet = float(ref.air_n_minus_one(np.array([LD(500)]), P, 288.15, 10.0 / 7.50061683)[0]) * 1e6
    assert abs((n6 - wet) - 0.5657) < 1e-3


@pytest.mark.parametrize("deg", [0.0, 5.0, 17.0, 30.0, 31.0])
def test_snell_anchor(deg):
    """n sin(theta') = sin(theta): 30 degrees into n = 3.9 comes out at asin(0.5 / 3.9) = asin(0.128205) = 7.3659 degrees"""
    th = math.radians(deg)
    a, b = ref.snell_slopes(np.array([LD(math.tan(th) * 0.6)]), np.array([LD(math.tan(th) * 0.8)]), LD("3.9"))
    out = math.atan(math.hypot(float(a[0]), float(b[0])))
    assert abs(3.9 * math.sin(out) - math.sin(th)) < 1e-15
    if deg == 30.0:
        assert abs(math.degrees(out) - 7.3659) < 1e-4
    if deg:
        assert abs(float(b[0]) / float(a[0]) - 0.8 / 0.6) < 1e-15            # the azimuth is kept


def test_wcs_round_trip_is_the_identity():
    for offaxis in (False, True):
        O = ref.Optics(cases.optics_block(offaxis))
        rng = np.random.default_rng(3)
        x, y = ref.lds(rng.uniform(-50.0, 4150.0, 500)), ref.lds(rng.uniform(-50.0, 4150.0, 500))
        thx, thy = O.xy_to_field(x, y)
        X, Y = O.field_to_xy(thx, thy)
        # the spec inverts the rotation by its transpose, and the uploaded f64 rows are orthonormal to 2^-52 only: 8 EPS rad in pixels
        tol = float(8 * ref.EPS / LD(O.img.cdmax) * 2)
        assert tol < 5e-9 and float(np.abs(X - x).max()) < tol and float(np.abs(Y - y).max()) < tol
        assert (math.degrees(float(np.hypot(thx, thy).max())) > 1.5) == offaxis


def test_dcr_derived_constants_of_the_site():
    """the config's site values: the air index the suite used to hold only to a range"""
    (air_p, _), (air_w, _), (r0, _) = ref.dcr_derived([620.0, 69.328, 293.15, 1.067, 1.0])
    assert 1e-4 < float(r0) < 4e-4 and float(air_p) > 0 and float(air_w) > 0
    nm1 = float(ref.air_n_minus_one(LD(620), 69.328, 293.15, 1.067))
    assert abs(float(r0) - (nm1 - 1.5 * nm1 * nm1 + 2.0 * nm1 ** 3)) < 1e-14     # (n^2 - 1) / (2 n^2) = d - 3/2 d^2 + 2 d^3 - ...


# ---------------- teeth ----------------
@pytest.mark.parametrize("mutation", sorted(ref.MUTATIONS))
def test_teeth(mutation):
    """the reference with one thing miswritten moves at least one field of at least 1 % of the photons by more than 100 bounds"""
    case = cases.by_name(ref.MUTATIONS[mutation])
    good, bad = reference(case), case.reference(mutate=mutation)
    share = {}
    for f in ref.FIELDS:
        bd = np.where(good.bounds[f] > 0, good.bounds[f], LD(1e-300))
        moved = np.abs(bad.fields[f] - good.fields[f]) > 100 * bd
        share[f] = float(moved.mean())
    print(mutation, case.name, {f: round(v, 4) for f, v in share.items() if v})
    assert max(share.values()) >= 0.01, (mutation, share)
