"""FITS-stamp objects on the FFT branch behind `stamp.fft_stamps`, host side: the transform of the quintic interpolant against the
quadrature of engine.quintic_kernel, the FFT-or-photons decision with the switch on and off, LSST_ImageBuilder.prepare's split, the
side arrays of the stamp pass, the config key, the argument checks of the entry point -- and the closed forms of
tests/stamp_closed_forms.py held against each other.  The kernel is held to them in tests/test_fft_stamps_gpu.py."""
import ctypes as C
import math

import numpy as np
import pytest

from imsim_amd import _abi, catalog, config, configs, fft_draw, lsst_image
from imsim_amd.engine import quintic_kernel
from imsim_amd.lsst_image import GalSimConfigError
import fft_closed_forms as cf
import stamp_closed_forms as sc
from test_fft_closed_forms import ROUNDING

FWHM = 0.7                    # arcsec, Gaussian PSF
THRESH = 1.0e5                # fft_sb_thresh
PSF_AREA = 2.0 * math.pi * (FWHM / 2.3548200450309493) ** 2        # 1 / peak of the unit-flux Gaussian [arcsec^2]
KPSF = [(_abi.IMS_KPSF_GAUSSIAN, 0, FWHM / 2.3548200450309493)]
I = catalog.KIND_IMAGE


def test_quintic_hat_is_the_transform_of_the_quintic_kernel():
    """Qhat against the Gauss-Legendre quadrature of engine.quintic_kernel(x) cos(2 pi u x), piece by piece over [-3, 3], 32 nodes per
    piece, for u in 0 .. 4: the pieces are quintics times a cosine of at most 4 periods per piece, which 32 nodes integrate to the
    rounding of the sum (some 1e-14: six pieces of up to 32 terms of size 1)."""
    worst = 0.0
    for u in np.linspace(0.0, 4.0, 161):
        got = float(sc.quintic_hat(u))
        want = sc.gauss_legendre_hat(quintic_kernel, float(u))
        worst = max(worst, abs(got - want))
    print(f"Qhat against the quadrature of engine.quintic_kernel, u in 0 .. 4: {worst:.3e}")
    assert worst <= 3.0e-14
    # the closed forms' own restatement of the kernel is the product's, to the rounding of the double evaluation: its polynomials
    # carry terms of up to 55 x 27 / 24 = 62 before their factors (x - 2), (x - 3) of at most 1 bring the value below 1
    x = np.linspace(-3.5, 3.5, 1401)
    assert float(np.abs(sc.quintic_kernel(x).astype(np.float64) - quintic_kernel(x)).max()) <= 62.0 * sc.EPS
    # reproduction of constants: 1 at 0, 0 at every other integer
    assert float(sc.quintic_hat(0.0)) == 1.0
    for j in range(1, 6):
        assert abs(float(sc.quintic_hat(float(j)))) <= 1.0e-30, j
    assert float(np.abs(sc.quintic_hat(np.linspace(0.0, 8.0, 8001))).max()) <= 1.0 + 1.0e-15       # factor_bound's premise
    assert float(sc.nearest_hat(0.0)) == 1.0 and abs(float(sc.nearest_hat(0.5)) - 2.0 / math.pi) < 1e-18


def _cat(kind, flux, scale=0.2, x=None, y=None, **kw):
    n = len(flux)
    c = dict(x=np.full(n, 128.3) if x is None else np.asarray(x, dtype=np.float64),
             y=np.full(n, 120.6) if y is None else np.asarray(y, dtype=np.float64), mag=np.zeros(n),
             nominal_flux=np.asarray(flux, dtype=np.float64), kind=np.asarray(kind, dtype=np.int32), hlr=np.full(n, 0.3),
             q=np.ones(n), pa=np.zeros(n), obj_id=np.arange(n, dtype=np.int64) + 5, n_knots=np.zeros(n), box_length=np.zeros(n),
             box_width=np.zeros(n), image_index=np.zeros(n, dtype=np.int64),
             image_scale=np.broadcast_to(np.asarray(scale, dtype=np.float64), (n,)).copy(), image_extent=np.full(n, 8.0))
    c.update(kw)
    return c


def _builder():
    b = lsst_image.LSST_ImageBuilder()
    b.setup({"det_name": "R22_S11", "xsize": 256, "ysize": 256})
    return b


def test_the_default_keeps_stamps_with_the_photons():
    """nothing moves while the switch is off, whether it is left out or given as False -- image_peaks or not"""
    kind = np.array([catalog.KIND_KNOTS, I, catalog.KIND_STREAK])
    flux = np.full(3, 1.0e12)
    for kw in ({}, {"fft_stamps": False}, {"fft_stamps": False, "image_peaks": np.full(3, 5.0)}, {"image_peaks": np.full(3, 5.0)}):
        sb = fft_draw.max_surface_brightness(flux, kind, np.full(3, 0.3), FWHM, box_area=np.array([0.0, 0.0, 1.5]), **kw)
        assert sb[0] == 0.0 and sb[1] == 0.0 and sb[2] > THRESH
        assert list(fft_draw.use_fft(flux, kind, np.full(3, 0.3), FWHM, THRESH, box_area=np.array([0.0, 0.0, 1.5]), **kw)) == [False, False, True]
    for kw in ({}, {"fft_stamps": False}, {"fft_stamps": False, "image_sizes": [(5, 5)]}):
        assert list(fft_draw.has_kspace_form(np.array([0, 1, 2, 3, 4, 5]), **kw)) == [True, True, True, False, True, False]


def test_with_the_switch_the_decision_flips_at_the_pixel_peak():
    """the estimate of Convolve(InterpolatedImage, PSF): F / (1 / psf peak + p^2 |det J| / max w) / 2 x 0.04"""
    img = np.array([[1.0, 3.0, -2.0], [0.0, 4.0, 2.0]])                # max w = 4 / 10
    p, mu = 0.25, 1.3
    peaks = fft_draw.image_peaks_per_flux([img], np.zeros(3, dtype=np.int64), np.array([p, p, 0.0]))
    np.testing.assert_allclose(peaks, [0.4 / p ** 2, 0.4 / p ** 2, 0.0], rtol=1e-15)
    inv = PSF_AREA + p * p * mu / 0.4
    flip = THRESH * inv * 2.0 / 0.04                                   # the flux at which the estimate IS the threshold
    assert flip > 1.0e6
    kind = np.array([I, I, 0])
    flux = np.array([flip * (1.0 + 1e-9), flip * (1.0 - 1e-9), 1.0e9])
    kw = dict(fft_stamps=True, image_peaks=peaks, jac_det=np.full(3, mu))
    sb = fft_draw.max_surface_brightness(flux, kind, np.full(3, 0.3), FWHM, **kw)
    np.testing.assert_allclose(sb[:2], flux[:2] / inv / 2.0 * 0.04, rtol=1e-13)
    assert list(fft_draw.use_fft(flux, kind, np.full(3, 0.3), FWHM, THRESH, **kw)) == [True, False, True]
    assert not fft_draw.use_fft(flux, kind, np.full(3, 0.3), FWHM, 0.0, **kw).any()                  # no threshold: never
    # without the peaks there is no estimate: photon-shot, as with the switch off
    assert fft_draw.max_surface_brightness(flux, kind, np.full(3, 0.3), FWHM, fft_stamps=True)[0] == 0.0
    assert list(fft_draw.has_kspace_form(np.array([0, 1, 2, 3, 4, 5]), fft_stamps=True)) == [True, True, True, False, True, True]
    # aliases to fold: the stamp's spectrum is no common factor of the folded sum
    assert list(fft_draw.has_kspace_form(np.array([0, 1, 2, 3, 4, 5]), fft_stamps=True, n_alias=1)) == [True, True, True, False, True, False]
    # knots and stamps are switched apart
    assert list(fft_draw.has_kspace_form(np.array([3, 5]), fft_knots=True)) == [True, False]
    assert list(fft_draw.has_kspace_form(np.array([3, 5]), fft_stamps=True)) == [False, True]


def test_a_stamp_larger_than_its_grid_stays_with_the_photons():
    """(w + 6) p against the grid of the stamp size: 64 pixels x 0.2" = 12.8"; a 58 x 10 stamp of 0.2" is 64 x 0.2 = 12.8" long with the
    interpolant's support -- it just fits; of 0.21" it does not; turned by 45 degrees its box spans (64 + 16) p / sqrt 2 = 11.3" and
    fits again."""
    img = np.ones((10, 58))
    cat = _cat([I, I, I, 0], [1.0e9] * 4, scale=[0.2, 0.21, 0.2, 0.2], pa=np.array([0.0, 0.0, 45.0, 0.0]))
    objects, _ = catalog.build_object_table(cat, np.full(4, 1000), stamp_size=np.array([64, 64, 64, 64]))
    ok = fft_draw.has_kspace_form(cat["kind"], objects, fft_stamps=True, image_sizes=[(58, 10)])
    assert list(ok) == [True, False, True, True]
    assert list(fft_draw.has_kspace_form(cat["kind"], objects)) == [False, False, False, True]
    with pytest.raises(ValueError, match="image_sizes"):
        fft_draw.has_kspace_form(cat["kind"], objects, fft_stamps=True)
    assert np.asarray(img).shape == (10, 58)


def _prepare(cat, scene, kpsf=KPSF, fwhm=FWHM, sizes=(64, 32, 32, 32), **kw):
    make = lambda c, p: catalog.build_object_table(c, p, stamp_size=np.array(sizes))
    return _builder().prepare(scene, cat, np.full(len(cat["x"]), 1000), make, fft_sb_thresh=THRESH, kpsf=kpsf, fwhm_total=fwhm, **kw)


def test_prepare_sends_the_bright_stamp_down_the_fft_branch():
    img0, img1 = np.ones((4, 6)), np.array([[1.0, 0.0], [-1.0, 3.0]])
    cat = _cat([I, 0, I, I], [1.0e9, 5.0e6, 2.0e5, 3.0e9], image_index=np.array([1, 0, 0, 0]))
    scene = configs.scene_c2(nx=256, ny=256)
    scene.image_profiles = [img0, img1]
    off = _prepare(cat, scene)
    off2 = _prepare(cat, scene, fft_stamps=False)
    modes = lambda job: list(lsst_image.fill_truth({}, job, np.zeros(job.n_kept))["mode"])
    assert modes(off) == modes(off2) == ["phot", "fft", "phot", "phot"] and off.fft_images is None and off2.fft_images is None
    assert off.fft_rows.tobytes() == off2.fft_rows.tobytes() and off.objects.tobytes() == off2.objects.tobytes()
    job = _prepare(cat, scene, fft_stamps=True)
    truth = lsst_image.fill_truth({}, job, np.zeros(job.n_kept))
    assert list(truth["mode"]) == ["fft", "fft", "phot", "fft"]
    assert list(truth["fft_flux"]) == [1.0e9, 5.0e6, 0.0, 3.0e9] and list(truth["phot_flux"]) == [0.0, 0.0, 1000.0, 0.0]
    # the rows: sorted by grid; a stamp object is filled as a point with the stamp's pixel scale, its image travels beside the rows
    assert list(job.fft_index) == [1, 3, 0] and list(job.fft_rows["nfft"]) == [32, 32, 64] and list(job.fft_rows["prof_ktable"]) == [-1] * 3
    assert job.fft_images.dtype == np.int32 and list(job.fft_images) == [-1, 0, 1]
    assert list(job.fft_rows["prof_scale"][1:]) == [0.2, 0.2] and job.fft_knots is None
    # a PSF whose aliases the fill folds (sigma 0.12": n_alias 1) keeps the stamps with the photons, the star not
    sharp = [(_abi.IMS_KPSF_GAUSSIAN, 0, 0.12)]
    job = _prepare(cat, scene, kpsf=sharp, fwhm=0.12 * 2.3548200450309493, fft_stamps=True)
    assert modes(job) == ["phot", "fft", "phot", "phot"] and job.fft_images is None
    # draw_method phot: nothing; fft: everything with a k-space form, the faint stamp too
    job = _prepare(cat, scene, fft_stamps=True, draw_method="phot")
    assert job.n_fft == 0 and job.fft_images is None
    job = _prepare(cat, scene, fft_stamps=True, draw_method="fft")
    assert job.n_fft == 4 and sorted(job.fft_images) == [-1, 0, 0, 1]


def test_side_arrays_follow_the_order_of_the_fft_rows():
    img0 = np.array([[1.0, -2.0, 3.0], [0.0, 4.0, 2.0]])
    img1 = np.array([[5.0]])
    size, offset, ab, w = fft_draw.image_pixel_lists([img0, img1])
    assert size.dtype == np.int32 and offset.dtype == np.int64 and ab.dtype == np.int32 and w.dtype == np.float64
    assert size.tolist() == [[3, 2], [1, 1]] and offset.tolist() == [0, 4, 5]
    assert ab.tolist() == [[0, 0], [2, 0], [1, 1], [2, 1], [0, 0]]               # (column, row), row-major, positive pixels only
    np.testing.assert_array_equal(w, [0.1, 0.3, 0.4, 0.2, 1.0])
    a, b, wt = sc.stamp_pixels(img0)
    assert a.tolist() == [0, 2, 1, 2] and b.tolist() == [0, 0, 1, 1] and np.array_equal(wt, w[:4])
    with pytest.raises(ValueError, match="no positive pixel"):
        fft_draw.image_pixel_lists([np.array([[0.0, -1.0]])])
    cat = _cat([I, 0, I, I], [1.0e9, 5.0e6, 2.0e9, 3.0e9], image_index=np.array([1, 0, 0, 1]))
    objects, _ = catalog.build_object_table(cat, np.full(4, 1000), stamp_size=np.array([128, 64, 32, 64]))
    before = objects.copy()
    rows, order = fft_draw.build_fft_objects(objects, cat["nominal_flux"], fft_draw.profile_ktable_ids(None, objects["prof_table"]))
    assert list(order) == [2, 1, 3, 0] and list(rows["prof_ktable"]) == [-1] * 4
    row_image = fft_draw.image_side_arrays(objects, order)
    assert objects.tobytes() == before.tobytes()
    assert row_image.dtype == np.int32 and list(row_image) == [0, -1, 1, 1]


def test_the_config_key_is_a_boolean():
    ev = config.Evaluator(config.load_config({}))
    assert config.parse_fft_stamps({}, ev) is False
    assert config.parse_fft_stamps({"fft_stamps": True}, ev) is True and config.parse_fft_stamps({"fft_stamps": False}, ev) is False
    for bad in (1, 0, "yes", "true", 2.0e5, None, [True]):
        with pytest.raises(GalSimConfigError, match="stamp.fft_stamps"):
            config.parse_fft_stamps({"fft_stamps": bad}, ev)


def test_the_entry_point_checks_its_arguments_before_any_launch():
    lib = _abi.load()
    assert lib.ims_abi_version() == 22
    assert "ims_fft_image_factor" in _abi.EXPORTS
    f = lib.ims_fft_image_factor
    assert f(None, None, None, 0, 0, None, 0, None, None, None, None, 1, None, None) == 0             # no row with a stamp: nothing to do
    assert f(None, None, None, 1, 32, None, 1, None, None, None, None, 1, None, None) == -1 and b"NULL" in lib.ims_last_error()
    P = _abi.FftParams()
    one = (C.c_double * 8)()
    p = C.cast(one, C.c_void_p)
    P.n_alias = 1
    assert f(C.byref(P), p, p, 1, 32, p, 1, p, p, p, p, 1, p, None) < 0 and b"n_alias" in lib.ims_last_error()
    P.n_alias = 0
    assert f(C.byref(P), p, p, 1, 33, p, 1, p, p, p, p, 1, p, None) == -1 and b"max_nfft" in lib.ims_last_error()
    assert f(C.byref(P), p, p, 1, 32, p, 0, p, p, p, p, 1, p, None) == -1 and b"n_images" in lib.ims_last_error()
    assert f(C.byref(P), p, p, 1, 32, p, 1, p, p, p, p, 2, p, None) == -1 and b"interpolant" in lib.ims_last_error()


# ---------------------------------------------------------------------------------------------
# the closed forms against each other
# ---------------------------------------------------------------------------------------------
SIGMAS_PSF = (0.25, 0.5)      # arcsec.  0.25": exp(-0.5 (0.25 pi / 0.2)^2) = 4.5e-4 at Nyquist -- alias_order 1, the aliases left out dominate
                              # the tolerance; 0.5": alias_order 0, the tolerance is the rounding's


def centre_pixel_stamp():
    img = np.full((5, 5), -1.0)
    img[1, 3] = 0.0
    img[2, 2] = 7.0
    return img


def image_tolerance(sigma, nfft, cx, cy, img, p):
    """per unit flux: the Gaussian-PSF point case's tolerance (tests/test_fft_closed_forms.py, as tests/test_fft_knots_gpu.py takes it:
    the bound on the aliases left out -- the interpolant's factor is at most 1 in modulus, so the Gaussian's bound holds -- plus
    ROUNDING) plus the periodic wrap of the tails"""
    return cf.omitted_alias_bound(sigma, nfft, 0, sc.PIXEL_SCALE) + ROUNDING + sc.wrap_bound(nfft, cx, cy, img, p, sigma, sc.PIXEL_SCALE)


def test_closed_forms_agree_on_the_host():
    """the numpy restatement of the branch (base band only) against the pixel integrals, per unit flux, for the stamp of the GPU test:
    a 5 x 5 stamp whose only positive pixel is the centre one, p = 0.2", Gaussian PSF of 0.25" (and of 0.5"), J' the identity, grid
    64."""
    nfft, cx, cy, p = 64, 31.4, 32.7, 0.2
    img = centre_pixel_stamp()
    assert fft_draw.kpsf_alias_order([(_abi.IMS_KPSF_GAUSSIAN, 0, 0.25)]) == 1 and fft_draw.kpsf_alias_order([(_abi.IMS_KPSF_GAUSSIAN, 0, 0.5)]) == 0
    for sigma in SIGMAS_PSF:
        got = sc.numpy_pipeline(nfft, cx, cy, img, p, sc.JACS[0], sigma, sc.PIXEL_SCALE, 1.0)
        want = sc.image_ref(nfft, cx, cy, img, p, sigma, sc.PIXEL_SCALE, 1.0)
        err = float(np.abs(got - want.astype(np.float64)).max())
        tol = image_tolerance(sigma, nfft, cx, cy, img, p)
        print(f"sigma {sigma}: numpy restatement against the pixel integrals {err:.3e} per unit flux, allowed {tol:.3e}; peak {float(want.max()):.3e}")
        assert err <= tol
        assert abs(float(want.sum()) - 1.0) < 1.0e-12
        # and it is not the point's image (the kernel has no second moment, so the difference is small, but far above the tolerance)
        diff = float(np.abs(want.astype(np.float64) - cf.erf_image(nfft, cx, cy, sigma / sc.PIXEL_SCALE, 1.0)).max())
        print(f"sigma {sigma}: differs from the point's image by {diff:.3e}")
        assert diff > 10.0 * tol
    # F_ref: one pixel at the stamp's centre is Qhat Qhat alone; F(0) = 1
    re, im = sc.F_ref(img, p, sc.JACS[0], 32, 0.2)
    assert float(np.abs(im).max()) == 0.0 and re[0, 0] == 1.0
    assert abs(float(re[3, 5]) - float(sc.quintic_hat(5 / 32.0) * sc.quintic_hat(3 / 32.0))) <= 4.0 * sc.EPS
    # a 1 x 2 stamp of equal pixels: cos(kx p / 2) Qhat Qhat
    re, im = sc.F_ref(np.ones((1, 2)), p, sc.JACS[0], 32, 0.2)
    dk = 2.0 * math.pi / (32 * 0.2)
    assert float(np.abs(im).max()) <= 4.0 * sc.EPS
    assert abs(float(re[29, 5]) - math.cos(5 * dk * 0.1) * float(sc.quintic_hat(5 / 32.0) * sc.quintic_hat(-3 / 32.0))) <= 4.0 * sc.EPS
    # the premise of factor_bound for every stamp of the GPU test: inside half the smallest grid
    for name, stamp, scale in sc.factor_stamps():
        for jac in sc.JACS:
            assert sc.extent(stamp, scale, jac) <= 0.5 * 32 * sc.PIXEL_SCALE, name


# the FFT-against-photons case of the GPU test: what enters its chi-square, settled on the host
PHOTON_CASE = dict(nfft=64, cx=31.6, cy=32.3, p=0.3, jac=(1.0, 0.3, -0.15, 0.9), sigma=0.3, flux=2.0e6, floor=25.0)


def photon_case_stamp():
    return np.random.default_rng(8).uniform(0.2, 3.0, size=(8, 8))


def test_the_expectation_of_the_photon_case_fills_its_footprint():
    """pixels whose expectation is at least 25 e-: at least a quarter of the stamp's footprint (here: several times the footprint,
    the PSF spreads 2e6 e- far), so the cut of the chi-square cannot hide a misplaced stamp.  Nearest interpolant: photons of unit
    flux, to which Pearson's chi-square applies (the quintic's photons carry +-1.58)."""
    c = PHOTON_CASE
    img = photon_case_stamp()
    want = sc.numpy_pipeline(c["nfft"], c["cx"], c["cy"], img, c["p"], c["jac"], c["sigma"], sc.PIXEL_SCALE, c["flux"], "nearest")
    n_in = int((want >= c["floor"]).sum())
    foot = sc.footprint_pixels(img, c["p"], c["jac"], sc.PIXEL_SCALE)
    print(f"{n_in} pixels of at least {c['floor']} e-, footprint {foot:.1f} pixels")
    assert n_in >= 0.25 * foot and n_in >= 100
    assert abs(want.sum() - c["flux"]) < 1e-6 * c["flux"]
    assert sc.extent(img, c["p"], c["jac"]) + 3 * c["p"] + 8 * c["sigma"] < 0.5 * c["nfft"] * sc.PIXEL_SCALE
