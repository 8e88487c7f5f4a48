"""Adaptive moments on the host (no GPU): the numpy restatement (tests/adaptive_moments_ref.py) reaches the fixed points known
in closed form, its status paths and those of psf_map.adaptive_from_state / adaptive_start, the argument checks of
ims_psf_adaptive, and the new keys of output.psf_map.

Tolerances of the fixed-point tests: five standard errors, the standard error measured on the sample itself -- it is split
into 16 disjoint groups, the reference runs on each, and the scatter of the 16 estimates (ddof 1) divided by sqrt(16) = 4 is the
standard error of the estimate from the whole sample."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import adaptive_moments_ref as ref
from imsim_amd import _abi, config, psf_map
from imsim_amd.lsst_image import GalSimConfigError

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
N = 200_000
FIELDS = ("xbar", "ybar", "Mxx", "Mxy", "Myy", "sigma", "rho4")


def estimate_with_errors(x, y, tol=1e-9):
    """(estimate from the whole sample, its standard error by the 16-group scatter), dicts over FIELDS"""
    w = np.ones(len(x))
    full = ref.iterate(x, y, w, tol=tol)
    assert full["status"] == ref.CONVERGED and full["n_used"] == len(x)
    groups = [ref.iterate(x[g::16], y[g::16], w[g::16], tol=tol) for g in range(16)]
    assert all(g["status"] == ref.CONVERGED for g in groups)
    se = {f: float(np.std([float(g[f]) for g in groups], ddof=1)) / 4.0 for f in FIELDS}
    return {f: float(full[f]) for f in FIELDS}, se


def test_reference_converges_to_an_elliptical_gaussians_covariance():
    """2e5 points of a Gaussian with axes 1 and 0.6 (axis ratio 0.6) rotated by 30 degrees: the matching weight of a Gaussian
    is the Gaussian itself, so M is its covariance, the centre 0 and rho4 = 2, each within 5 standard errors."""
    rng = np.random.default_rng(20021)
    a, b, th = 1.0, 0.6, math.radians(30.0)
    p, q = a * rng.standard_normal(N), b * rng.standard_normal(N)
    c, s = math.cos(th), math.sin(th)
    x, y = c * p - s * q, s * p + c * q
    cov = dict(Mxx=c * c * a * a + s * s * b * b, Myy=s * s * a * a + c * c * b * b, Mxy=c * s * (a * a - b * b), xbar=0.0, ybar=0.0,
               sigma=math.sqrt(a * b), rho4=2.0)
    est, se = estimate_with_errors(x, y)
    for f in FIELDS:
        print(f"{f}: {est[f]:+.6f} expected {cov[f]:+.6f}, deviation / standard error {(est[f] - cov[f]) / se[f]:+.2f}")
    for f in FIELDS:
        assert abs(est[f] - cov[f]) <= 5.0 * se[f], f
    assert abs(est["Mxy"]) > 20.0 * se["Mxy"]                      # the rotation is seen, not lost in the noise


def test_reference_converges_to_the_mixtures_root_below_the_unweighted_sigma():
    """2e5 points of the two-Gaussian mixture of DoubleGaussian (fwhm 0.8): M = m I with m the root of the fixed-point equation
    (adaptive_moments_ref.mixture_root, by bisection), within 5 standard errors; and the unweighted sigma, which the wide
    component inflates, is above the adaptive one -- what the feature is for."""
    comp, _, _ = config.double_gaussian_psf(0.8)
    s1, s2, f1 = comp[2], comp[5], comp[6]
    m = float(ref.mixture_root([s1 * s1, s2 * s2], [f1, 1.0 - f1]))
    assert s1 * s1 < m < f1 * s1 * s1 + (1.0 - f1) * s2 * s2
    rng = np.random.default_rng(20022)
    sig = np.where(rng.random(N) < f1, s1, s2)
    x, y = sig * rng.standard_normal(N), sig * rng.standard_normal(N)
    est, se = estimate_with_errors(x, y)
    want = dict(Mxx=m, Myy=m, Mxy=0.0, xbar=0.0, ybar=0.0, sigma=math.sqrt(m))
    for f in want:
        print(f"{f}: {est[f]:+.6f} expected {want[f]:+.6f}, deviation / standard error {(est[f] - want[f]) / se[f]:+.2f}")
    for f in want:
        assert abs(est[f] - want[f]) <= 5.0 * se[f], f
    assert est["rho4"] > 2.0 + 5.0 * se["rho4"]                     # heavier than a Gaussian under its own weight
    ixx, iyy, ixy = np.var(x), np.var(y), np.mean(x * y) - x.mean() * y.mean()
    unweighted = (ixx * iyy - ixy * ixy) ** 0.25
    print(f"unweighted sigma {unweighted:.5f}, adaptive sigma {est['sigma']:.5f}")
    assert unweighted > est["sigma"] + 5.0 * se["sigma"]


def _arrays(res):
    """the device's three arrays for one row, from a result of the reference"""
    state = [[float(res[k]) for k in ("xbar", "ybar", "Mxx", "Mxy", "Myy")]]
    return state, [[res["status"], res["iter"]]], [[float(res["rho4"]), float(res["flux"]), res["n_used"], res["n_dropped"]]]


def test_status_paths():
    """no photon: status 3 and NaN; one photon: status 2 (its unweighted trace is zero); max_iter = 1 from a start three times too
    wide: status 1 after one update -- in the reference, and reported alike by adaptive_from_state."""
    rng = np.random.default_rng(20023)
    x, y = 0.3 * rng.standard_normal(5000), 0.3 * rng.standard_normal(5000)
    none = ref.iterate(x[:7], y[:7], np.zeros(7))
    assert (none["status"], none["iter"], none["n_used"], none["n_dropped"], float(none["flux"])) == (ref.EMPTY, 0, 0, 7, 0.0)
    row = psf_map.adaptive_from_state(*_arrays(none))[0]
    assert row.dtype == psf_map.ADAPTIVE_DTYPE and (row["status"], row["n_used"], row["n_dropped"], row["flux"]) == (3, 0, 7, 0.0)
    for f in ("xbar", "ybar", "Mxx", "Myy", "Mxy", "sigma", "e1", "e2", "rho4", "fwhm"):
        assert np.isnan(none[f]) and np.isnan(row[f]), f
    assert ref.iterate(np.zeros(0), np.zeros(0), np.zeros(0))["status"] == ref.EMPTY
    one = ref.iterate(x[:1], y[:1], np.ones(1))
    assert (one["status"], one["iter"], one["n_used"]) == (ref.FAILED, 0, 1)
    row = psf_map.adaptive_from_state(*_arrays(one))[0]
    assert (row["status"], row["iter"], row["n_used"], row["xbar"], row["ybar"]) == (2, 0, 1, x[0], y[0])
    wide = ref.iterate(x, y, np.ones(5000), start=(0.0, 0.0, 0.81, 0.0, 0.81), max_iter=1)
    assert (wide["status"], wide["iter"]) == (ref.RUNNING, 1) and 0.5 < float(wide["Mxx"]) < 0.81
    row = psf_map.adaptive_from_state(*_arrays(wide))[0]
    assert (row["status"], row["iter"], row["n_used"], row["flux"]) == (1, 1, 5000, 5000.0)
    assert row["sigma"] == math.sqrt(math.sqrt(row["Mxx"] * row["Myy"] - row["Mxy"] ** 2)) and row["fwhm"] == 2.3548200450309493 * row["sigma"]
    assert row["e1"] == (row["Mxx"] - row["Myy"]) / (row["Mxx"] + row["Myy"]) and row["e2"] == 2.0 * row["Mxy"] / (row["Mxx"] + row["Myy"])
    assert row["rho4"] == float(wide["rho4"])
    done = ref.iterate(x, y, np.ones(5000), start=(0.0, 0.0, 0.81, 0.0, 0.81))
    assert done["status"] == ref.CONVERGED and 1 < done["iter"] < 40 and abs(float(done["sigma"]) - 0.3) < 0.02
    # a weight that has lost the profile (all photons 40 sigma away: every g underflows to 0) fails and keeps its state
    lost = ref.iterate(x + 100.0, y, np.ones(5000), start=(0.0, 0.0, 1e-4, 0.0, 1e-4))
    assert (lost["status"], lost["iter"], float(lost["Mxx"])) == (ref.FAILED, 0, 1e-4)
    assert len(psf_map.adaptive_from_state(np.zeros((0, 5)), np.zeros((0, 2)), np.zeros((0, 4)))) == 0


def test_adaptive_start():
    """the start of the rows from their unweighted moments: centroid and half the trace; no photon -> 3; a single photon -> 2, or
    guess_sigma's square when one is given; guesses override"""
    sums = [[4.0, 0.0, 2.0, 2.0, 0.0, 2.0], [0.0] * 6, [1.0, 0.5, -0.25, 0.25, -0.125, 0.0625]]
    m = psf_map.moments_from_sums(sums, [[3, 1], [0, 7], [1, 0]])
    state, status = psf_map.adaptive_start(m)
    assert status.tolist() == [1, 3, 2] and status.dtype == np.int32
    assert state[0].tolist() == [0.0, 0.5, 0.5 * (0.5 + 0.25), 0.0, 0.5 * (0.5 + 0.25)] and np.all(np.isnan(state[1]))
    assert state[2].tolist() == [0.5, -0.25, 0.0, 0.0, 0.0]
    state, status = psf_map.adaptive_start(m, guess_sigma=0.5)
    assert status.tolist() == [1, 3, 1] and state[2].tolist() == [0.5, -0.25, 0.25, 0.0, 0.25] and state[0, 2] == 0.25
    state, status = psf_map.adaptive_start(m, guess_centre=[1.0, 2.0], guess_sigma=[0.5, 1.0, 2.0])
    assert state[0].tolist() == [1.0, 2.0, 0.25, 0.0, 0.25] and state[2].tolist() == [1.0, 2.0, 4.0, 0.0, 4.0] and status.tolist() == [1, 3, 1]
    state, _ = psf_map.adaptive_start(m, guess_centre=[[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    assert state[2, :2].tolist() == [5.0, 6.0] and state[0, 2] == 0.375
    with pytest.raises(ValueError, match="guess_sigma"):
        psf_map.adaptive_start(m, guess_sigma=0.0)


def test_entry_point_is_exported_and_checks_its_arguments():
    """ims_psf_adaptive is declared in the header, listed in _abi.EXPORTS and exported by the library, which loads without a
    GPU; every argument check returns -1 with its message before anything is launched."""
    assert "ims_psf_adaptive" in _abi.EXPORTS
    with open(os.path.join(HERE, "..", "include", "imsim_hip.h")) as f:
        header = f.read()
    assert "ims_psf_adaptive(const ims_render_params_t* params, int32_t stage, int32_t n_rounds, double tol" in header
    assert "#define IMS_ABI_VERSION 22" in header
    lib = _abi.load()
    assert lib.ims_abi_version() == 22
    f = lib.ims_psf_adaptive
    assert f(None, 1, 1, 1e-6, None, None, None, None, None) == -1 and b"NULL" in lib.ims_last_error()
    P = _abi.RenderParams()
    P.seg_size = 256
    assert f(C.byref(P), 3, 1, 1e-6, None, None, None, None, None) == -1 and b"stage" in lib.ims_last_error()
    assert f(C.byref(P), 1, 0, 1e-6, None, None, None, None, None) == -1 and b"n_rounds" in lib.ims_last_error()
    for tol in (0.0, -1e-6, math.inf, math.nan):
        assert f(C.byref(P), 2, 1, tol, None, None, None, None, None) == -1 and b"tol" in lib.ims_last_error()
    assert f(C.byref(P), 1, 1, 1e-6, None, None, None, None, None) == 0                       # no points: nothing to do
    rows = (C.c_double * 32)()
    pre = (C.c_int64 * 2)(0, 1)
    P.n_objects, P.objects, P.seg_prefix, P.n_segments = 1, C.cast(rows, C.c_void_p), C.cast(pre, C.c_void_p), 1
    state, status, aux = (C.c_double * 5)(), (C.c_int32 * 2)(), (C.c_double * 4)()
    for args in ((None, status, aux), (state, None, aux), (state, status, None)):
        assert f(C.byref(P), 2, 1, 1e-6, None, *args, None) == -1 and b"state / status / aux" in lib.ims_last_error()
    assert f(C.byref(P), 2, 1, 1e-6, None, state, status, aux, None) == -1 and b"partial" in lib.ims_last_error()
    part = (C.c_double * 10)()
    P.n_objects = 2 ** 31
    assert f(C.byref(P), 1, 1, 1e-6, part, state, status, aux, None) == -1 and b"too many points" in lib.ims_last_error()
    P.n_objects, P.n_segments = 1, 2 ** 31 - 8
    assert f(C.byref(P), 1, 1, 1e-6, part, state, status, aux, None) == -1 and b"too many segments" in lib.ims_last_error()
    P.n_segments, P.seg_size = 1, 128
    assert f(C.byref(P), 1, 1, 1e-6, part, state, status, aux, None) == -1 and b"seg_size" in lib.ims_last_error()


def _ev():
    return config.Evaluator({})


def test_parse_config_reads_the_new_keys():
    base = dict(nx=8, n_photons=100000, stage="psf")
    assert psf_map.parse_config({"file_name": "m.fits"}, _ev()) == base
    assert psf_map.parse_config({"file_name": "m.fits", "moments": "unweighted"}, _ev()) == base
    assert psf_map.parse_config({"file_name": "m.fits", "moments": "adaptive"}, _ev()) == \
        dict(base, moments="adaptive", guess_sigma=None, tolerance=1e-6, max_iter=100)
    kw = psf_map.parse_config({"file_name": "m.fits", "nx": 3, "n_photons": 2000, "stage": "ops", "moments": "adaptive",
                               "guess_sigma": 0.3, "tolerance": 1e-8, "max_iter": 40}, _ev())
    assert kw == dict(nx=3, n_photons=2000, stage="ops", moments="adaptive", guess_sigma=0.3, tolerance=1e-8, max_iter=40)


@pytest.mark.parametrize("extra,match", [
    ({"moments": "hsm"}, "moments must be one of"),
    ({"guess_sigma": 0.3}, "guess_sigma is given without moments: adaptive"),
    ({"tolerance": 1e-6}, "tolerance is given without moments: adaptive"),
    ({"moments": "unweighted", "max_iter": 10}, "max_iter is given without moments: adaptive"),
    ({"moments": "adaptive", "tolerance": 0.0}, "tolerance must be positive"),
    ({"moments": "adaptive", "tolerance": -1e-6}, "tolerance must be positive"),
    ({"moments": "adaptive", "max_iter": 0}, "max_iter must be at least 1"),
    ({"moments": "adaptive", "guess_sigma": -0.1}, "guess_sigma must be positive"),
])
def test_parse_config_errors(extra, match):
    with pytest.raises(GalSimConfigError, match=match):
        psf_map.parse_config(dict({"file_name": "m.fits"}, **extra), _ev())


def test_config_errors_come_before_any_gpu_work():
    """the driver parses output.psf_map before it renders anything: a bad key raises without a GPU"""
    o = {"input.instance_catalog.file_name": os.path.join(HERE, "golden", "example_instcat_subset.txt"), "image.nobjects": 3,
         "stamp.draw_method": "phot", "output.psf_map": {"file_name": "m.fits", "moments": "adaptive", "max_iter": 0}}
    with pytest.raises(GalSimConfigError, match="max_iter must be at least 1"):
        config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")], overrides=o)
    o["output.psf_map"] = {"file_name": "m.fits", "tolerance": 1e-6}
    with pytest.raises(GalSimConfigError, match="without moments: adaptive"):
        config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")], overrides=o)


def test_header_and_cube_of_the_adaptive_planes():
    assert [name[2:] for name, _ in psf_map.ADAPTIVE_PLANES] == list(psf_map.ADAPTIVE_DTYPE.names[:12])
    plain = psf_map.make_header("R22_S11", "psf", 622.2, 5, 4096, 4000, 2)
    h = psf_map.make_header("R22_S11", "psf", 622.2, 5, 4096, 4000, 2, adaptive=(1e-7, 60))
    assert {k: v for k, v in h.items() if k in plain} == plain and list(h)[:len(plain)] == list(plain)
    assert [h[f"PLANE{13 + k}"][0] for k in range(12)] == [name for name, _ in psf_map.ADAPTIVE_PLANES]
    assert h["TOL"][0] == 1e-7 and h["MAXITER"][0] == 60 and "TOL" not in plain and "PLANE13" not in plain
    rows = np.zeros(4, dtype=psf_map.ADAPTIVE_DTYPE)
    rows["status"], rows["Mxy"] = [0, 1, 2, 3], [0.5, 0.25, 0.0, np.nan]
    cube = psf_map.adaptive_cube(rows, 2)
    assert cube.shape == (12, 2, 2) and cube.dtype == np.float64
    assert cube[0].tolist() == [[0.0, 1.0], [2.0, 3.0]] and cube[6, 0].tolist() == [0.5, 0.25] and np.isnan(cube[6, 1, 1])
