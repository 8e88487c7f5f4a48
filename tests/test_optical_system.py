"""The optical state of a visit on the host (imsim_amd/optical_system.py): the reference's own unit tests restated
(tests/test_optical_zernikes.py), the random stream, the field fit against an independent one, the monomial expansion of the
annular Zernikes, and the config rules of input.atm_psf.doOpt.  None of it needs a GPU."""
import os

import numpy as np
import pytest

import optical_screen_numpy as R
from imsim_amd import _abi, config, optical_system as osys
from imsim_amd.lsst_image import GalSimConfigError

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden")
EPS = 0.61


# ---------------- the reference's tests/test_optical_zernikes.py ----------------
def test_mock_deviations_shape_and_seeding():
    a, b, c = osys.mock_deviations(3, DATA), osys.mock_deviations(3, DATA), osys.mock_deviations(4, DATA)
    assert a.shape == (50,)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_mock_deviations_average_to_zero():
    """The reference's test_average, literally: seed 125, one draw thrown away, 1 999 further draws of the same stream into 2 000
    columns (the last stays zero), every |row mean| < 0.03.  That bound holds for this seed (largest mean 0.0257) and NOT in
    general: five degrees of freedom have standard deviations of 1.08 .. 2.68, so the standard error of a 2 000-draw mean is
    0.024 .. 0.06 for them (RandomState(0) gives a largest mean of 0.12).  What holds for any seed is asserted beside it:
    every row's mean within 4 standard errors, 4 std / sqrt(2000), for one long stream and for 2 000 separately seeded calls."""
    std = osys.aos_std(DATA)
    rs = np.random.RandomState(125)
    assert np.array_equal(rs.normal(0.0, std), osys.mock_deviations(125, DATA))     # mock_deviations(125) seeds the stream
    hist = np.zeros((50, 2000))
    for i in range(1999):
        hist[:, i] = rs.normal(0.0, std)                                             # mock_deviations('persist')
    print("largest |mean|, seed 125:", np.abs(hist.mean(axis=1)).max())
    assert np.all(np.abs(hist.mean(axis=1)) < 0.03)
    rs = np.random.RandomState(0)
    mean = np.mean([rs.normal(0.0, std) for _ in range(2000)], axis=0)
    assert np.all(np.abs(mean) < 4.0 * std / np.sqrt(2000.0) + 1e-300)
    draws = np.array([osys.mock_deviations(s, DATA) for s in range(2000)])
    assert np.all(np.abs(draws.mean(axis=0)) < 4.0 * std / np.sqrt(2000.0) + 1e-300)


def test_zero_deviations_and_nineteen_coefficients():
    oz = osys.OpticalZernikes(np.zeros(50), data_dir=DATA)
    assert np.all(oz.deviation_coeff == 0.0)
    assert np.array_equal(oz.sampling_coeff, oz.nominal_coeff)
    assert oz.cartesian_coeff(0.3, -0.2).shape == (19,) and oz.polar_coeff(0.5, 1.0).shape == (19,)
    assert oz.cartesian_coeff(np.zeros(7), np.ones(7)).shape == (19, 7)
    assert np.all(osys.OpticalZernikes(np.zeros(50), data_dir=DATA, nominal=False).field_matrix == 0.0)


def test_polar_and_cartesian_sampling_points_agree():
    x, y = osys.cartesian_coords()
    r, t = osys.polar_coords()
    assert len(x) == 35
    np.testing.assert_allclose(r * np.cos(t), x, atol=1e-15)
    np.testing.assert_allclose(r * np.sin(t), y, atol=1e-15)
    oz = osys.visit_optical_state(7, DATA)
    np.testing.assert_allclose(oz.polar_coeff(r, t), oz.cartesian_coeff(x, y), atol=1e-13)


# ---------------- the stream ----------------
@pytest.mark.parametrize("seed", [0, 12345, 2 ** 31 - 1])
def test_mock_deviations_are_the_reference_stream(seed):
    std = np.std(np.genfromtxt(os.path.join(DATA, "optics_data", "aos_sim_results.txt.gz"), skip_header=1), axis=1)
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        want = np.random.normal(0, std)
    finally:
        np.random.set_state(state)
    assert np.array_equal(osys.mock_deviations(seed, DATA), want)


def test_visit_state_is_seeded_apart_from_the_atmosphere():
    a, b = osys.visit_optical_state(5, DATA), osys.visit_optical_state(5, DATA)
    assert np.array_equal(a.deviations, b.deviations) and not np.array_equal(a.deviations, osys.visit_optical_state(6, DATA).deviations)
    mock_seed = int(np.random.default_rng(5 + osys.OPTICAL_SEED_OFFSET).random() * 2 ** 31)
    assert np.array_equal(a.deviations, 3.0 * osys.mock_deviations(mock_seed, DATA))
    assert osys.OPTICAL_SEED_OFFSET != 271828


# ---------------- the fit over the field ----------------
def test_field_fit_against_an_independent_least_squares():
    """The 19 fits against numpy.linalg.lstsq on a basis of the textbook Noll Zernikes (optical_screen_numpy.circular_zernike:
    the factorial formula of the radial polynomials, evaluated in polar coordinates at the 35 points in degrees, unscaled).
    Singular values of that 35 x 15 basis: 265.8, 224.6, 174.4, 83.6, 83.4, 47.1, 39.8, 37.6, 15.9, 7.32, 5.42, 5.30, 4.23,
    4.20, 3.99 -- condition number 67 (the points reach 1.7 "radii" of the unit disk the polynomials are scaled for), so two
    backward-stable solutions agree to about 67 * 2^-52 * a few, ~1e-13 of the largest coefficient: the 1e-10 asked for
    has three decades of margin and is kept."""
    oz = osys.visit_optical_state(99, DATA)
    x, y = osys.cartesian_coords()
    basis = np.stack([R.circular_zernike(j, x, y) for j in range(1, 16)], axis=1)          # [35, 15]
    sv = np.linalg.svd(basis, compute_uv=False)
    print("singular values", np.array2string(sv, precision=3))
    assert 60.0 < sv[0] / sv[-1] < 75.0
    coef = np.stack([np.linalg.lstsq(basis, c, rcond=None)[0] for c in oz.sampling_coeff])
    scale = np.abs(coef).max()
    assert np.abs(coef - oz.fit_coeff).max() <= 1e-10 * scale
    # the fitted values at the sampling points and their residual are those of the independent fit
    fit = oz.cartesian_coeff(x, y)
    assert np.abs(fit - coef @ basis.T).max() <= 1e-10 * scale
    res_own, res_ind = fit - oz.sampling_coeff, coef @ basis.T - oz.sampling_coeff
    assert abs(np.linalg.norm(res_own) - np.linalg.norm(res_ind)) <= 1e-10 * scale
    # and between the sampling points: the monomial matrix the device gets evaluates the same polynomials
    rng = np.random.default_rng(3)
    px, py = rng.uniform(-1.5, 1.5, 200), rng.uniform(-1.5, 1.5, 200)
    direct = coef @ np.stack([R.circular_zernike(j, px, py) for j in range(1, 16)])
    assert np.abs(oz.cartesian_coeff(px, py) - direct).max() <= 1e-10 * np.abs(direct).max() * 40


# ---------------- the annular Zernikes as monomials ----------------
def _annular_direct(x, y):
    """annular Z4 .. Z22 (eps 0.61) from radial polynomials formed in the test's own code (optical_screen_numpy.annular_zernike:
    Gram-Schmidt by quadrature), nothing of the product's opd tables or expansion"""
    return np.stack([R.annular_zernike(j, x, y, EPS) for j in range(4, 23)])


def test_independent_annular_zernikes_are_mahajans():
    """the test-side construction against the closed forms of Mahajan (1981) for Z4, Z6 and Z11"""
    rng = np.random.default_rng(2)
    r, t = np.sqrt(rng.uniform(EPS ** 2, 1.0, 500)), rng.uniform(0.0, 2.0 * np.pi, 500)
    x, y, e2 = r * np.cos(t), r * np.sin(t), EPS ** 2
    np.testing.assert_allclose(R.annular_zernike(4, x, y, EPS), np.sqrt(3) * (2 * r * r - 1 - e2) / (1 - e2), rtol=0, atol=1e-12)
    np.testing.assert_allclose(R.annular_zernike(6, x, y, EPS), np.sqrt(6) * r * r * np.cos(2 * t) / np.sqrt(1 + e2 + e2 * e2),
                               rtol=0, atol=1e-12)
    np.testing.assert_allclose(R.annular_zernike(11, x, y, EPS),
                               np.sqrt(5) * (6 * r ** 4 - 6 * (1 + e2) * r * r + 1 + 4 * e2 + e2 * e2) / (1 - e2) ** 2, rtol=0, atol=1e-11)


def test_pupil_monomials_against_direct_annular_zernikes():
    """19 x 28 expansion against the independent direct evaluation on 1 000 points of the annulus.  Achieved: values agree to
    ~1e-13 absolute, i.e. ~1e-16 of the largest monomial coefficient (880: the polynomials of degree 6 cancel to values of a few
    units, which costs three digits and explains the absolute figure).  Central-difference gradients with h = 1e-6: the
    truncation term, h^2 / 6 times a third derivative, is ~1e-10 of the gradient scale at most (third derivatives of these
    polynomials reach a few hundred times the gradients), the rounding term eps |f| / h ~ 1e-10 against gradients of order 10:
    the bound is 1e-8 of the largest gradient."""
    pm = osys.pupil_matrix()
    assert pm.shape == (19, 28)
    rng = np.random.default_rng(1)
    r, t = np.sqrt(rng.uniform(EPS ** 2, 1.0, 1000)), rng.uniform(0.0, 2.0 * np.pi, 1000)
    x, y = r * np.cos(t), r * np.sin(t)
    val = pm @ osys.monomial_values(6, x, y)
    ref = _annular_direct(x, y)
    big = np.abs(pm).max()
    print("largest monomial coefficient", big, "max |value difference|", np.abs(val - ref).max())
    assert np.abs(val - ref).max() <= 1e-12 * big
    # gradients: the restatement's coefficient derivation (p w, q w) evaluated exactly as the device does, per Zernike
    a = np.eye(19)
    gx, gy = R.gradient_coefficients(pm, a)
    dx = gx @ osys.monomial_values(5, x, y)
    dy = gy @ osys.monomial_values(5, x, y)
    h = 1e-6
    fdx = (_annular_direct(x + h, y) - _annular_direct(x - h, y)) / (2 * h)
    fdy = (_annular_direct(x, y + h) - _annular_direct(x, y - h)) / (2 * h)
    gbig = max(np.abs(dx).max(), np.abs(dy).max())
    print("max gradient difference / largest gradient", max(np.abs(dx - fdx).max(), np.abs(dy - fdy).max()) / gbig)
    assert np.abs(dx - fdx).max() <= 1e-8 * gbig and np.abs(dy - fdy).max() <= 1e-8 * gbig


def test_pupil_monomials_are_orthonormal_over_the_annulus():
    """Gauss-Legendre in rho^2 (exact for these polynomials with 8 nodes) times the trapezoid rule in angle (exact for
    trigonometric polynomials below the number of nodes): the Gram matrix of Z4 .. Z22 is the identity to 1e-12."""
    pm = osys.pupil_matrix()
    node, wt = np.polynomial.legendre.leggauss(12)
    s = 0.5 * (1.0 - EPS ** 2) * node + 0.5 * (1.0 + EPS ** 2)             # rho^2, uniform weight: the area measure
    ang = 2.0 * np.pi * np.arange(32) / 32
    rho = np.sqrt(s)[:, None]
    x, y = (rho * np.cos(ang)[None, :]).ravel(), (rho * np.sin(ang)[None, :]).ravel()
    w = (0.5 * wt[:, None] * np.ones(32)[None, :] / 32).ravel()
    val = pm @ osys.monomial_values(6, x, y)
    gram = (val * w) @ val.T
    print("max |gram - 1|", np.abs(gram - np.eye(19)).max())
    assert np.abs(gram - np.eye(19)).max() < 1e-12


def test_screen_struct_layout():
    S = osys.visit_optical_state(1, DATA).screen_struct()
    assert S.inv_r == 1.0 / 4.18 and S.grad_scale == 500.0 * (1.0 / 4.18) and S.remap == 1.708 / 2.04
    f, p = R.screen_arrays(S)
    assert f.shape == (19, 15) and p.shape == (19, 28) and np.array_equal(p, osys.pupil_matrix())
    assert [osys.row(4, q) for q in range(5)] == [0, 5, 9, 12, 14] and osys.row(6, 6) == 27 and osys.row(5, 5) == 20
    import ctypes
    assert ctypes.sizeof(_abi.AtmosphereOptical) == ctypes.sizeof(_abi.Atmosphere) + ctypes.sizeof(_abi.OpticalScreen)
    assert _abi.AtmosphereOptical.opt.offset == ctypes.sizeof(_abi.Atmosphere)


# ---------------- config ----------------
def _res():
    return config.ProcessResult()


def test_doopt_config_rules(tmp_path):
    ev = config.Evaluator(config.load_config({}))
    phot = {"draw_method": "phot", "fft_sb_thresh": 2.0e5}
    assert config.parse_atm_psf_options(None, phot, ev, DATA, _res()) is False
    assert config.parse_atm_psf_options({"doOpt": False}, {"draw_method": "auto", "fft_sb_thresh": 2.0e5}, ev, DATA, _res()) is False
    assert config.parse_atm_psf_options({"doOpt": True}, phot, ev, DATA, _res()) is True
    assert config.parse_atm_psf_options({"doOpt": True}, {"draw_method": "auto"}, ev, DATA, _res()) is True     # no FFT branch without a threshold
    with pytest.raises(GalSimConfigError, match="draw_method: phot"):
        config.parse_atm_psf_options({"doOpt": True}, {"draw_method": "auto", "fft_sb_thresh": 2.0e5}, ev, DATA, _res())
    with pytest.raises(GalSimConfigError, match="draw_method: phot"):
        config.parse_atm_psf_options({"doOpt": True}, {"fft_sb_thresh": 2.0e5}, ev, DATA, _res())
    with pytest.raises(GalSimConfigError, match="draw_method: phot"):
        config.parse_atm_psf_options({"doOpt": True}, {"draw_method": "fft"}, ev, DATA, _res())       # every object by FFT, threshold or not
    # LSST_PhotonPoolingImage sends objects above fft_sb_thresh to the FFT branch whatever draw_method says: only its absence helps
    pool = "LSST_PhotonPoolingImage"
    with pytest.raises(GalSimConfigError, match="Remove stamp.fft_sb_thresh"):
        config.parse_atm_psf_options({"doOpt": True}, phot, ev, DATA, _res(), pool)
    with pytest.raises(GalSimConfigError, match="Remove stamp.fft_sb_thresh"):
        config.parse_atm_psf_options({"doOpt": True}, {"draw_method": "auto", "fft_sb_thresh": 2.0e5}, ev, DATA, _res(), pool)
    assert config.parse_atm_psf_options({"doOpt": True}, {"draw_method": "phot"}, ev, DATA, _res(), pool) is True
    assert config.parse_atm_psf_options({"doOpt": True}, {"fft_sb_thresh": 0.0}, ev, DATA, _res(), pool) is True
    assert config.parse_atm_psf_options({"doOpt": False}, phot, ev, DATA, _res(), pool) is False
    # the optical screen is one more of the at most four components of a launch
    atm_item, gauss = {"type": "AtmosphericPSF"}, {"type": "Gaussian", "fwhm": 0.3}
    ok = {"type": "Convolve", "items": [atm_item, gauss]}
    assert config.parse_atm_psf_options({"doOpt": True}, phot, ev, DATA, _res(), "LSST_Image", ok) is True
    with pytest.raises(GalSimConfigError, match="5 components"):
        config.parse_atm_psf_options({"doOpt": True}, phot, ev, DATA, _res(), "LSST_Image", {"type": "Convolve", "items": [atm_item, gauss, gauss]})
    assert config.parse_atm_psf_options({"doOpt": True, "_no2k": True}, phot, ev, DATA, _res(), "LSST_Image",
                                        {"type": "Convolve", "items": [atm_item, gauss, gauss]}) is True
    # a data directory that lacks one of the tables: the error names the file
    d = tmp_path / "optics_data"
    d.mkdir()
    for name in (osys.AOS_FILE, osys.NOMINAL_FILE):
        os.symlink(os.path.join(DATA, "optics_data", name + ".gz"), d / (name + ".gz"))
    with pytest.raises(GalSimConfigError, match="sensitivity_matrix.txt"):
        config.parse_atm_psf_options({"doOpt": True}, phot, ev, str(tmp_path), _res())
    res = _res()
    config.parse_atm_psf_options({"save_file": "atm.pkl", "nproc": 4}, phot, ev, DATA, res)
    assert len(res.ignored) == 1 and "save_file" in res.ignored[0] and "nproc" not in res.ignored[0]


def test_process_refuses_doopt_before_any_gpu_work(tmp_path):
    """config.Process itself: with the FFT branch in reach and with a table missing, a GalSimConfigError before anything is rendered"""
    def run(extra, data_dir):
        o = {"input.instance_catalog.file_name": os.path.join(HERE, "golden", "example_instcat_subset.txt"),
             "output.dir": str(tmp_path), "psf.items.0": {"type": "AtmosphericPSF"},
             "input.atm_psf": {"airmass": 1.1, "rawSeeing": 0.7, "band": "r", "boresight": "unused", "doOpt": True}}
        o.update(extra)
        return config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")],
                              overrides=o, data_dir=data_dir)
    with pytest.raises(GalSimConfigError, match="doOpt"):
        run({}, None)                                                  # the template's draw_method auto + fft_sb_thresh
    with pytest.raises(GalSimConfigError, match="aos_sim_results.txt"):
        run({"stamp.draw_method": "phot"}, None)                       # the packaged data directory holds no optics_data
    # photon pooling: draw_method phot does not keep bright objects off the FFT branch, so the same config is refused there ...
    pooling = {"image.type": "LSST_PhotonPoolingImage", "stamp.type": "LSST_Photons", "input.checkpoint": "", "stamp.draw_method": "phot"}
    with pytest.raises(GalSimConfigError, match="Remove stamp.fft_sb_thresh"):
        run(pooling, None)
    # ... and passes this check without the threshold (it then stops at the missing table of the packaged data directory)
    with pytest.raises(GalSimConfigError, match="aos_sim_results.txt"):
        run(dict(pooling, **{"stamp.fft_sb_thresh": 0.0}), None)


def test_atmospheric_psf_signature():
    import inspect
    from imsim_amd import atm_psf
    p = inspect.signature(atm_psf.AtmosphericPSF.__init__).parameters
    assert p["doOpt"].default is False and p["data_dir"].default is None
    assert p["optical_deviations"].default is None and p["optical_nominal"].default is True
    with pytest.raises(osys.OpticsDataError, match="optics_data"):
        osys.visit_optical_state(1, str(HERE))


def test_optical_screen_before_the_phase_screens_is_refused():
    """the library's argument check (before any HIP call): the phase screens' deviates are addressed by their place among the
    other components in the kernels and by their list index in the pre-pass, which agree only in the order of getPSF"""
    import ctypes
    lib = _abi.load()
    P = _abi.RenderParams()
    P.seg_size, P.n_psf = 256, 2
    dummy = (ctypes.c_double * 8)()
    P.atm = ctypes.addressof(dummy)                  # never dereferenced by the check
    for k, kind in enumerate((_abi.IMS_PSF_OPTICAL_SCREEN, _abi.IMS_PSF_SCREENS)):
        P.psf[k].kind, P.psf[k].p0 = kind, 1.0
    assert lib.ims_shoot_accumulate(ctypes.byref(P), None) == -1
    assert b"must come after" in lib.ims_last_error()
    P.psf[0].kind, P.psf[1].kind = _abi.IMS_PSF_OPTICAL_SCREEN, _abi.IMS_PSF_OPTICAL_SCREEN
    assert lib.ims_shoot_accumulate(ctypes.byref(P), None) == -1 and b"more than one" in lib.ims_last_error()
