"""ims_psf_moments / psf_map.compute on the GPU: the sums against the photon pool of the same rows summed in np.longdouble,
closed forms, determinism, points that lose every photon, the optical phase screen against its numpy restatement, and
output.psf_map through the config driver.

The bound of the first test (used again by the optical-screen test)
-------------------------------------------------------------------
Reference: T = sum_i tau_i over the photons of the pool, tau_i the exact term (w, w dx, w dy, w dx^2, w dx dy, w dy^2 with
dx = x - x0 of the pool's f64 values), formed and added in np.longdouble.  Kernel: S = the f64 sum of t_i.  With u = 2^-53:

* a term.  dx = fl(x - x0) carries one rounding (none in stage 1, whose rows have x0 = 0: the pool's 0 + x is x); w dx and
  (w dx) dx are one rounding each (the library is built without contraction), so a second-moment term holds dx twice and two
  products: |t_i - tau_i| <= gamma_4 |tau_i|.
* the sum.  A term reaches the result through at most D additions: 6 levels of the xor butterfly over the 64 lanes and 3 additions
  over the 4 wavefronts in the segment's workgroup; then ceil(n_seg / 256) additions in the combining thread (the first onto 0),
  6 butterfly levels and 3 more.  For any fixed summation tree |fl(sum) - sum t_i| <= gamma_D sum |t_i| (Higham, Accuracy and
  Stability of Numerical Algorithms, 2nd ed., section 4.2), D = 18 + ceil(n_seg / 256), n_seg = ceil(n / 256).
* the reference's own error: n longdouble additions and the products, below (n + 4) 2^-64 sum |tau_i|.

  |S - T| <= (gamma_{D + 4} + (n + 4) 2^-64) sum |tau_i| + the smallest subnormal,   gamma_k = k u / (1 - k u).

The counts are integers and must be equal."""
import math
import os

import numpy as np
import pytest

import optical_screen_numpy as OSN
import photon_source_cases as cases
from imsim_amd import _abi, config, configs, fits_io, psf_map

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
U = 2.0 ** -53
COUNTS = (1, 63, 64, 65, 257, 1000, 2 ** 16 + 1)          # 2^16 + 1: 257 segments, two per thread of the combining workgroup
BASE_HIGH = 2 ** 32 + 12345                                # a photon base index above 2^32
WORST = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def bound(n, abs_sum):
    n_seg = -(-int(n) // 256)
    k = 18 + -(-n_seg // 256) + 4
    return (k * U / (1.0 - k * U) + (n + 4) * 2.0 ** -64) * float(abs_sum) + 5e-324


def reference_sums(x, y, w, x0, y0):
    """(T [6], sum |tau| [6], used, dropped) of one point's pool photons, in np.longdouble"""
    x, y, w = x.astype(LD), y.astype(LD), w.astype(LD)
    dx, dy = x - LD(x0), y - LD(y0)
    terms = [w, w * dx, w * dy, w * dx * dx, w * dx * dy, w * dy * dy]
    return ([t.sum() for t in terms], [np.abs(t).sum() for t in terms], int((w != 0).sum()), int((w == 0).sum()))


def check_against_pool(run, pool, rows, what):
    sums, counts = run.raw()
    offs = np.concatenate([[0], np.cumsum(rows["n_phot"])])
    worst = 0.0
    for i, o in enumerate(rows):
        sl = slice(offs[i], offs[i + 1])
        T, A, used, dropped = reference_sums(pool["x"][sl], pool["y"][sl], pool["flux"][sl], o["x0"], o["y0"])
        assert (counts[i, 0], counts[i, 1]) == (used, dropped), (what, i)
        for q in range(6):
            err, b = abs(float(LD(sums[i, q]) - T[q])), bound(o["n_phot"], A[q])
            worst = max(worst, err / b)
            assert err <= b, (what, i, q, err, b)
    WORST[what] = max(WORST.get(what, 0.0), worst)
    print(f"{what}: worst error / bound {worst:.3g} over {len(rows)} points")
    return worst


def table(n_points):
    """photon counts and bases of a table: every count of COUNTS, the long one twice at most; every fourth row above 2^32"""
    i = np.arange(n_points)
    n = np.array([COUNTS[k % 6] for k in i])
    if n_points > 1:
        n[[6, n_points - 5]] = COUNTS[6]
    first = np.where(i % 4 == 1, BASE_HIGH + 1000 * i, 37 * i)
    return n, first


def stage1_scene():
    """Kolmogorov (chromatic) + Gaussian, no operators: photon_source_cases.production_case's PSF"""
    r2, cdf = configs.standard_tables()
    return cases._scene([(cases.RAD, 2, 0.7, -0.3, 620.0), (cases.G, 0, 0.2, 1.0, 650.0)], r2, cdf, cases.sed_tables(3))


def stage1_rows(n_points, n_phot=None, first=None):
    o = cases.rows(n_points)                        # sheared jac, rotated winv of 5 pixels per arcsec, ids and bases beyond 32 bits
    o["x0"], o["y0"] = 0.0, 0.0                     # the pool's x is then the kick itself, bit for bit
    o["sed_table"] = [(0, -1, 1)[k % 3] for k in range(n_points)]
    n, f = table(n_points)
    o["n_phot"], o["phot_first"] = (n if n_phot is None else n_phot), (f if first is None else first)
    return o


def stage2_scene():
    return configs.scene_c3(nx=64, ny=64, sensor=False)       # Kolmogorov + Gaussian, imSim's default operator chain


def stage2_rows(scene, n_points, n_phot=None, first=None):
    i = np.arange(n_points)
    xy = np.stack([3.25 + (37 * i) % 59, 2.5 + (23 * i) % 61], axis=1)
    n, f = table(n_points)
    o = psf_map.point_rows(scene, xy, n if n_phot is None else n_phot, "ops")
    o["phot_first"] = f if first is None else first
    o["obj_id"] = [cases.OBJ_IDS[k % 4] + 16 * (k // 4) for k in i]
    return o


@pytest.fixture(scope="module")
def renderers(torch_cuda):
    out = {}
    for stage, make in (("psf", stage1_scene), ("ops", stage2_scene)):
        sc = make()
        out[stage] = (sc, psf_map.renderer_for(sc))
    return out


def run_and_pool(r, rows, stage):
    run = psf_map.Prepared(r, rows, stage)
    run()
    pool = r.shoot_ops_photons(rows, converted=False)
    r.synchronize()
    return run, pool.to_host()


@pytest.mark.parametrize("stage", ["psf", "ops"])
def test_same_photons_exact_sums(renderers, stage):
    """One point with each photon count, one point based above 2^32, and a table of 130 points: the kernel's six sums against the
    unconverted pool of ims_shoot_ops_photons for the same rows and seed within the bound of the module docstring, the counts
    equal.  Worst error / bound measured on the MI355X: 0.141 in stage psf, 0.111 in stage ops."""
    sc, r = renderers[stage]
    make = stage1_rows if stage == "psf" else (lambda *a, **k: stage2_rows(sc, *a, **k))
    for n in COUNTS:
        rows = make(1, n_phot=[n], first=[0])
        run, pool = run_and_pool(r, rows, stage)
        check_against_pool(run, pool, rows, stage)
    rows = make(1, n_phot=[1000], first=[BASE_HIGH])
    low = make(1, n_phot=[1000], first=[12345])
    run, pool = run_and_pool(r, rows, stage)
    check_against_pool(run, pool, rows, stage)
    run_low = psf_map.Prepared(r, low, stage)
    run_low()
    assert run_low.raw()[0].tobytes() != run.raw()[0].tobytes(), "the high half of the photon index reaches the counters"
    rows = make(130)
    assert (rows["phot_first"] > 2 ** 32).sum() > 30 and set(rows["n_phot"]) == set(COUNTS)
    run, pool = run_and_pool(r, rows, stage)
    check_against_pool(run, pool, rows, stage)
    sums, counts = run.raw()
    if stage == "ops":
        assert counts[:, 1].sum() > 0 and np.all(counts.sum(axis=1) == rows["n_phot"])      # the annulus does lose photons
    else:
        assert np.all(counts[:, 0] == rows["n_phot"]) and np.all(counts[:, 1] == 0)
    print("worst error / bound so far:", WORST)


@pytest.mark.parametrize("name", ["gaussian", "double_gaussian"])
def test_closed_forms(torch_cuda, name):
    """Single components at n = 2^20, offsets in arcsec.  Tolerances: five standard errors with the sampling variances of a
    Gaussian of the same sigma -- 2 sigma^4 / N for Ixx and Iyy, sigma^4 / N for Ixy, sigma^2 / N per centroid axis (for the
    double Gaussian, whose fourth moment is larger, that is less than five of its own standard errors: the stricter reading).
    The photons of this seed were checked on the CPU with tests/photon_source_ref.py before the test was written: the largest
    deviation is 0.29 of the tolerance (Ixx of the double Gaussian)."""
    n = 1 << 20
    if name == "gaussian":
        fwhm = 0.7
        psf, var = [(_abi.IMS_PSF_GAUSSIAN, 0, fwhm / 2.3548200450309493, 0.0, 1.0)], (fwhm / 2.3548200450309493) ** 2
    else:
        comp, _, _ = config.double_gaussian_psf(0.8)
        s1, s2, f1 = comp[2], comp[5], comp[6]
        psf, var = [comp], f1 * s1 * s1 + (1.0 - f1) * s2 * s2
    m = psf_map.compute(psf, np.zeros((1, 2)), n, stage="psf", wavelength=620.0, seed=398414)[0]
    tol2, tolxy, tolc = 5.0 * math.sqrt(2.0 * var * var / n), 5.0 * math.sqrt(var * var / n), 5.0 * math.sqrt(var / n)
    print(name, {k: float(m[k]) for k in ("xbar", "ybar", "Ixx", "Iyy", "Ixy", "sigma", "fwhm")}, "expected variance", var)
    assert m["n_used"] == n and m["n_dropped"] == 0 and m["flux"] == n
    assert abs(m["Ixx"] - var) <= tol2 and abs(m["Iyy"] - var) <= tol2 and abs(m["Ixy"]) <= tolxy
    assert abs(m["xbar"]) <= tolc and abs(m["ybar"]) <= tolc
    assert m["fwhm"] == 2.3548200450309493 * m["sigma"]


@pytest.mark.parametrize("stage", ["psf", "ops"])
def test_determinism_and_row_order(renderers, stage):
    """two calls give identical bytes; the reversed table gives the reversed rows, bit for bit"""
    sc, r = renderers[stage]
    rows = stage1_rows(130) if stage == "psf" else stage2_rows(sc, 130)
    a = psf_map.compute(sc, rows, stage=stage, renderer=r)
    b = psf_map.compute(sc, rows, stage=stage, renderer=r)
    c = psf_map.compute(sc, rows[::-1].copy(), stage=stage, renderer=r)
    assert a["n_used"].sum() > 100_000
    assert a.tobytes() == b.tobytes()
    assert c[::-1].tobytes() == a.tobytes()
    alone = psf_map.compute(sc, rows[6:7].copy(), stage=stage, renderer=r)        # a multi-workgroup point on its own
    assert alone.tobytes() == a[6:7].tobytes()


def test_all_photons_lost(renderers):
    """A stage-2 point 6e4 pixels (3.3 degrees) off the CCD, where every ray is vignetted or lost (tried on the CPU oracle):
    n_used 0, n_dropped n, NaN moments, no exception; its neighbours in the launch are what they are without it."""
    sc, r = renderers["ops"]
    xy = np.array([[20.5, 30.25], [6.0e4, 32.0], [40.0, 12.5]])
    rows = psf_map.point_rows(sc, xy, 1000, "ops")
    m = psf_map.compute(sc, rows, stage="ops", renderer=r)
    assert (m["n_used"][1], m["n_dropped"][1], m["flux"][1]) == (0, 1000, 0.0)
    for f in ("xbar", "ybar", "Ixx", "Iyy", "Ixy", "sigma", "e1", "e2", "fwhm"):
        assert np.isnan(m[f][1]), f
    r.synchronize()                                   # (raises on a device-side error)
    others = psf_map.compute(sc, rows[[0, 2]].copy(), stage="ops", renderer=r)
    assert m[[0, 2]].tobytes() == others.tobytes()
    assert np.all(m["n_used"][[0, 2]] > 900) and np.all(np.isfinite(m["sigma"][[0, 2]]))


ON = dict(doOpt=True, data_dir=os.path.join(HERE, "golden"), optical_deviations=np.zeros(50), optical_nominal=False)
EPS_OBSC = 0.61


@pytest.mark.parametrize("terms,expect", [({(2, 1): 2.0}, None), ({(0, 0): 4.0, (2, 1): 2.0}, "flip")],
                         ids=["astigmatism", "astigmatism+defocus"])
def test_optical_screen_moments_follow_the_restatement(torch_cuda, terms, expect):
    """doOpt with the state set to a single astigmatism term a_6 = c thx (and, second case, a constant defocus beside it, without
    which an astigmatic kick (k u, -k v) has equal moments on both axes), the atmosphere switched off, two field points at
    thx = +- 1 degree.  The restatement (tests/optical_screen_numpy.py) gives every photon's gradient from the pupil position
    the pool records, bit for bit; p0 and the identity winv make the kick.  The kernel's sums match the restatement's
    within the bound of the module docstring, (e1, e2) follow in sign and value, and with the defocus e1 flips with thx."""
    from imsim_amd.engine import Renderer
    sc = configs.scene_c3b(nx=64, ny=64, sensor=False, screen_size=102.4, screen_scale=0.1, optical=ON)
    for (j, t), val in terms.items():
        sc.atm.opt.field_matrix[j, t] = val
    sc.psf, sc.ops = [sc.atm.optical_component()], []
    rows = psf_map.point_rows(sc, np.array([[10.0, 20.0], [50.0, 40.0]]), 20_000, "psf", wavelength=620.0)
    rows["atm_tan_x"], rows["atm_tan_y"] = np.radians([1.0, -1.0]), 0.0
    rows["x0"], rows["y0"] = 0.0, 0.0
    r = psf_map.renderer_for(sc)
    run, pool = run_and_pool(r, rows, "psf")
    S = sc.atm.opt.screen_struct()
    p0 = float(sc.psf[0][2])
    sums, counts = run.raw()
    m = run.result()
    e_ref = []
    for i in range(2):
        sl = slice(20_000 * i, 20_000 * (i + 1))
        _, gu, gv = OSN.evaluate(S, np.full(20_000, rows["atm_tan_x"][i]), np.zeros(20_000), pool["pupil_u"][sl], pool["pupil_v"][sl])
        ku, kv = p0 * gu, p0 * gv
        x, y = 1.0 * ku + 0.0 * kv, 0.0 * ku + 1.0 * kv                       # winv (dx, dy) of the identity, as the kernel forms it
        assert np.array_equal(x, pool["x"][sl]) and np.array_equal(y, pool["y"][sl])
        T, A, used, dropped = reference_sums(x, y, np.ones(20_000), 0.0, 0.0)
        assert (counts[i, 0], counts[i, 1]) == (used, dropped) == (20_000, 0)
        for q in range(6):
            assert abs(float(LD(sums[i, q]) - T[q])) <= bound(20_000, A[q]), (i, q)
        xb, yb = T[1] / T[0], T[2] / T[0]
        ixx, ixy, iyy = T[3] / T[0] - xb * xb, T[4] / T[0] - xb * yb, T[5] / T[0] - yb * yb
        e1, e2 = float((ixx - iyy) / (ixx + iyy)), float(2 * ixy / (ixx + iyy))
        e_ref.append((e1, e2))
        print(f"point {i}: e1 {m['e1'][i]:+.6f} (restatement {e1:+.6f})  e2 {m['e2'][i]:+.6f} ({e2:+.6f})  sigma {m['sigma'][i]:.5f} arcsec")
        assert np.sign(m["e1"][i]) == np.sign(e1) and np.sign(m["e2"][i]) == np.sign(e2)
        assert abs(m["e1"][i] - e1) < 1e-9 and abs(m["e2"][i] - e2) < 1e-9
        assert m["sigma"][i] > 0.01
    if expect == "flip":
        # kick (A u, B v), A = g4 d + g6 a6, B = g4 d - g6 a6: e1 = (A^2 - B^2) / (A^2 + B^2), opposite at +thx and -thx
        from imsim_amd import optical_system
        g4, g6 = 4.0 * math.sqrt(3.0) / (1.0 - EPS_OBSC ** 2), 2.0 * math.sqrt(6.0) / math.sqrt(1.0 + EPS_OBSC ** 2 + EPS_OBSC ** 4)
        a6 = 2.0 * 1.0 * optical_system.THETA_REMAP
        A_, B_ = g4 * 4.0 + g6 * a6, g4 * 4.0 - g6 * a6
        e_pred = (A_ * A_ - B_ * B_) / (A_ * A_ + B_ * B_)
        assert e_pred > 0.2 and m["e1"][0] > 0.5 * e_pred and m["e1"][1] < -0.5 * e_pred
        assert abs(m["e2"][0]) < 0.05 and abs(m["e2"][1]) < 0.05              # the long axis lies along u, then along v


def test_config_end_to_end(torch_cuda, tmp_path, monkeypatch):
    """A one-CCD visit with output.psf_map (nx 2, 1000 photons): the file is listed, its cube's planes are compute() on the same
    points of the same scene, the header names them; an LSST_Flat lists the key as ignored."""
    seen = []
    real = psf_map.compute

    def spy(scene, points, n_photons=None, **kw):
        seen.append((scene, np.array(points), n_photons, kw))
        return real(scene, points, n_photons, **kw)
    monkeypatch.setattr(psf_map, "compute", spy)
    o = {"input.instance_catalog.file_name": os.path.join(HERE, "golden", "example_instcat_subset.txt"),
         "image.nobjects": 3, "stamp.draw_method": "phot", "output.dir": str(tmp_path),
         "output.psf_map": {"file_name": "psf_map.fits", "nx": 2, "n_photons": 1000, "stage": "ops"}}
    res = config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")], overrides=o)
    fn = str(tmp_path / "psf_map.fits")
    assert fn in res.files and not any("psf_map" in s for s in res.ignored)
    hdus = fits_io.read_fits(fn)
    assert len(hdus) == 1 and len(seen) == 1
    h, data = hdus[0]
    scene, pts, n_photons, kw = seen[0]
    assert data.shape == (len(psf_map.PLANES), 2, 2) and len(pts) == 4 and n_photons == 1000 and kw["stage"] == "ops"
    assert pts.tolist() == psf_map.grid_points(scene.nx, scene.ny, 2).tolist()
    again = real(scene, pts, 1000, **kw)
    for k, (name, _) in enumerate(psf_map.PLANES):
        assert h[f"PLANE{k + 1}"] == name
        assert data[k].tobytes() == np.asarray(again[name], dtype=np.float64).reshape(2, 2).tobytes(), name
    assert (h["STAGE"], h["NPHOT"], h["DET_NAME"], h["UNITS"]) == ("ops", 1000, res.det_names[0], "pixel") and h["WAVELEN"] > 300.0
    assert np.all(data[1] + data[2] == 1000) and np.all(data[1] > 900) and np.all(np.isfinite(data))
    flat = config.Process({"image": {"type": "LSST_Flat", "random_seed": 1234, "xsize": 64, "ysize": 48, "counts_per_pixel": 100,
                                     "max_counts_per_iter": 100},
                           "output": {"psf_map": {"file_name": str(tmp_path / "never.fits")}}})
    assert "output.psf_map" in flat.ignored and not os.path.exists(str(tmp_path / "never.fits"))
