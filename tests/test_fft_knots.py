"""RandomKnots on the FFT branch behind `stamp.fft_knots`, host side: the FFT-or-photons decision with the switch on and off,
LSST_ImageBuilder.prepare's split, the side arrays of the knots pass, the config key, the argument checks of the two entry points --
and the closed forms of tests/knots_closed_forms.py held against each other.  The kernels are held to them in
tests/test_fft_knots_gpu.py."""
import ctypes as C
import math

import numpy as np
import pytest

from imsim_amd import _abi, catalog, config, configs, fft_draw, lsst_image
from imsim_amd.lsst_image import GalSimConfigError
import fft_closed_forms as cf
import knots_closed_forms as kc
from test_fft_closed_forms import ROUNDING

FWHM = 0.7                    # arcsec, Gaussian PSF
THRESH = 1.0e5                # fft_sb_thresh
PSF_AREA = 2.0 * math.pi * (FWHM / 2.3548200450309493) ** 2        # 1 / peak of the unit-flux Gaussian [arcsec^2]


def _cat(kind, flux, n_knots=10.0, x=None, y=None):
    n = len(flux)
    return dict(x=np.full(n, 128.3) if x is None else np.asarray(x, dtype=np.float64),
                y=np.full(n, 120.6) if y is None else np.asarray(y, dtype=np.float64), mag=np.zeros(n),
                nominal_flux=np.asarray(flux, dtype=np.float64), kind=np.asarray(kind, dtype=np.int32), hlr=np.full(n, 0.3),
                q=np.ones(n), pa=np.zeros(n), obj_id=np.arange(n, dtype=np.int64) + 5,
                n_knots=np.broadcast_to(np.asarray(n_knots, dtype=np.float64), (n,)).copy(), box_length=np.zeros(n), box_width=np.zeros(n),
                image_index=np.zeros(n, dtype=np.int64), image_scale=np.full(n, 0.2), image_extent=np.full(n, 8.0))


def _builder():
    b = lsst_image.LSST_ImageBuilder()
    b.setup({"det_name": "R22_S11", "xsize": 256, "ysize": 256})
    return b


def test_the_default_keeps_knots_with_the_photons():
    """the literals of tests/test_fft_streak.py: nothing moves while the switch is off, whether it is left out or given as False"""
    kind = np.array([catalog.KIND_KNOTS, catalog.KIND_IMAGE, catalog.KIND_STREAK])
    flux = np.full(3, 1.0e12)
    for kw in ({}, {"fft_knots": False}):
        sb = fft_draw.max_surface_brightness(flux, kind, np.full(3, 0.3), FWHM, box_area=np.array([0.0, 0.0, 1.5]), **kw)
        assert sb[0] == 0.0 and sb[1] == 0.0 and sb[2] > THRESH
        assert list(fft_draw.use_fft(flux, kind, np.full(3, 0.3), FWHM, THRESH, box_area=np.array([0.0, 0.0, 1.5]), **kw)) == [False, False, True]
        assert list(fft_draw.has_kspace_form(np.array([0, 1, 2, 3, 4, 5]), **kw)) == [True, True, True, False, True, False]


def test_with_the_switch_a_bright_knots_object_takes_the_fft_branch():
    """GalSim's estimate for Convolve(RandomKnots, PSF): the deltas add nothing, so it is the point source's -- F / psf area / 2 x 0.04"""
    kind = np.array([catalog.KIND_KNOTS, 0, catalog.KIND_IMAGE, catalog.KIND_KNOTS])
    flux = np.array([1.0e9, 1.0e9, 1.0e9, 9.0e5])
    sb = fft_draw.max_surface_brightness(flux, kind, np.full(4, 0.3), FWHM, fft_knots=True)
    assert sb[0] == sb[1] and sb[2] == 0.0
    np.testing.assert_allclose(sb[0], 1.0e9 / PSF_AREA / 2.0 * 0.04, rtol=1e-12)
    assert list(fft_draw.use_fft(flux, kind, np.full(4, 0.3), FWHM, THRESH, fft_knots=True)) == [True, True, False, False]
    assert not fft_draw.use_fft(flux, kind, np.full(4, 0.3), FWHM, 0.0, fft_knots=True).any()          # no threshold: never
    assert list(fft_draw.has_kspace_form(np.array([0, 1, 2, 3, 4, 5]), fft_knots=True)) == [True, True, True, True, True, False]
    # aliases to fold: the structure factor is no common factor of the folded sum
    assert list(fft_draw.has_kspace_form(np.array([0, 1, 2, 3, 4, 5]), fft_knots=True, n_alias=1)) == [True, True, True, False, True, False]


def test_prepare_sends_the_bright_knots_object_down_the_fft_branch():
    K = catalog.KIND_KNOTS
    cat = _cat([K, 0, K, 1], [1.0e9, 5.0e6, 2.0e5, 3.0e3], n_knots=[12.0, 0.0, 7.0, 0.0])
    scene = configs.scene_c2(nx=256, ny=256)
    kpsf = [(_abi.IMS_KPSF_GAUSSIAN, 0, FWHM / 2.3548200450309493)]
    phot = np.array([1000, 1000, 1000, 1000])
    make = lambda c, p: catalog.build_object_table(c, p, stamp_size=np.array([64, 32, 32, 32]))
    b = _builder()
    off = b.prepare(scene, cat, phot, make, fft_sb_thresh=THRESH, kpsf=kpsf, fwhm_total=FWHM)
    assert list(lsst_image.fill_truth({}, off, np.zeros(off.n_kept))["mode"]) == ["phot", "fft", "phot", "phot"] and off.fft_knots is None
    job = b.prepare(scene, cat, phot, make, fft_sb_thresh=THRESH, kpsf=kpsf, fwhm_total=FWHM, fft_knots=True)
    truth = lsst_image.fill_truth({}, job, np.zeros(job.n_kept))
    assert list(truth["mode"]) == ["fft", "fft", "phot", "phot"]
    assert list(truth["fft_flux"]) == [1.0e9, 5.0e6, 0.0, 0.0] and list(truth["phot_flux"]) == [0.0, 0.0, 1000.0, 1000.0]
    # the rows: sorted by grid (the star's 32 first); the knots object is filled as a point, its knots travel beside the rows
    assert list(job.fft_index) == [1, 0] and list(job.fft_rows["nfft"]) == [32, 64] and list(job.fft_rows["prof_ktable"]) == [-1, -1]
    n_knots, sigma, offset = job.fft_knots
    assert n_knots.dtype == np.int32 and sigma.dtype == np.float64 and offset.dtype == np.int64
    assert list(n_knots) == [0, 12] and list(offset) == [0, 0] and sigma[0] == 0.0 and sigma[1] == 0.3 / 1.1774100225154747
    assert job.fft_rows["obj_id"][1] == 5
    # a PSF whose aliases the fill folds (sigma 0.12": n_alias 1) keeps the knots with the photons, the star not
    sharp = [(_abi.IMS_KPSF_GAUSSIAN, 0, 0.12)]
    assert fft_draw.kpsf_alias_order(sharp) == 1 and fft_draw.kpsf_alias_order(kpsf) == 0 and fft_draw.kpsf_alias_order(None) == 0
    job = b.prepare(scene, cat, phot, make, fft_sb_thresh=THRESH, kpsf=sharp, fwhm_total=0.12 * 2.3548200450309493, fft_knots=True)
    assert list(lsst_image.fill_truth({}, job, np.zeros(job.n_kept))["mode"]) == ["phot", "fft", "phot", "phot"] and job.fft_knots is None
    # draw_method phot: nothing; fft: everything with a k-space form, the faint knots object too
    job = b.prepare(scene, cat, phot, make, fft_sb_thresh=THRESH, kpsf=kpsf, fwhm_total=FWHM, fft_knots=True, draw_method="phot")
    assert job.n_fft == 0 and job.fft_knots is None
    job = b.prepare(scene, cat, phot, make, fft_sb_thresh=THRESH, kpsf=kpsf, fwhm_total=FWHM, fft_knots=True, draw_method="fft")
    assert job.n_fft == 4 and sorted(job.fft_knots[0]) == [0, 0, 7, 12]


def test_side_arrays_follow_the_order_of_the_fft_rows():
    K = catalog.KIND_KNOTS
    cat = _cat([K, 0, K, K], [1.0e9, 5.0e6, 2.0e9, 3.0e9], n_knots=[12.0, 0.0, 7.0, 257.0])
    cat["hlr"] = np.array([0.3, 0.0, 0.5, 0.7])
    objects, _ = catalog.build_object_table(cat, np.full(4, 1000), stamp_size=np.array([128, 64, 32, 64]))
    before = objects.copy()
    rows, order = fft_draw.build_fft_objects(objects, cat["nominal_flux"], fft_draw.profile_ktable_ids(None, objects["prof_table"]))
    assert list(order) == [2, 1, 3, 0] and list(rows["prof_ktable"]) == [-1] * 4
    n_knots, sigma, offset = fft_draw.knot_side_arrays(objects, order)
    assert objects.tobytes() == before.tobytes()
    assert list(n_knots) == [7, 0, 257, 12] and list(offset) == [0, 7, 7, 264]
    np.testing.assert_array_equal(sigma, np.array([0.5, 0.0, 0.7, 0.3]) / 1.1774100225154747)
    np.testing.assert_array_equal(rows["obj_id"], objects["obj_id"][order])


def test_the_config_key_is_a_boolean():
    ev = config.Evaluator(config.load_config({}))
    assert config.parse_fft_knots({}, ev) is False
    assert config.parse_fft_knots({"fft_knots": True}, ev) is True and config.parse_fft_knots({"fft_knots": False}, ev) is False
    for bad in (1, 0, "yes", "true", 2.0e5, None, [True]):
        with pytest.raises(GalSimConfigError, match="stamp.fft_knots"):
            config.parse_fft_knots({"fft_knots": bad}, ev)


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _abi.load()
    assert lib.ims_abi_version() == 22
    assert lib.ims_fft_knots_factor(None, None, None, 0, 0, None, None, None, None, None) == 0         # no row with knots: nothing to do
    assert lib.ims_fft_knots_factor(None, None, None, 1, 32, None, None, None, None, None) == -1 and b"NULL" in lib.ims_last_error()
    P = _abi.FftParams()
    one = (C.c_double * 8)()
    p = C.cast(one, C.c_void_p)
    P.n_alias = 1
    assert lib.ims_fft_knots_factor(C.byref(P), p, p, 1, 32, p, p, p, p, None) < 0 and b"n_alias" in lib.ims_last_error()
    P.n_alias = 0
    assert lib.ims_fft_knots_factor(C.byref(P), p, p, 1, 33, p, p, p, p, None) == -1 and b"max_nfft" in lib.ims_last_error()
    assert lib.ims_knot_positions(1, None, 0, None, None, None, None, None) == 0
    assert lib.ims_knot_positions(1, None, 3, None, None, None, None, None) == -1 and b"NULL" in lib.ims_last_error()


# what the numpy restatement of the branch misses image_ref by, per unit flux, on the host (printed below): 1.0e-16 for the
# cases of the GPU test -- far inside the Gaussian-PSF point case's tolerance, which therefore holds for knots as it stands
CASES = ((64, 31.4, 30.7, 2), (64, 31.4, 30.7, 7), (64, 30.2, 33.1, 65))        # nfft, cx, cy, N
SIGMA_PSF = cf.POINT_SIGMAS[0]                                                   # 0.5": n_alias 0


def knot_cloud(n, seed, sigma=0.35, jac=(0.9, 0.3, -0.2, 0.7)):
    """displacements like the kernel's (a sheared Gaussian cloud), from numpy's generator: the closed forms do not care which"""
    g = np.random.default_rng(seed).standard_normal((n, 2)) * sigma
    g = np.clip(g, -3.0 * sigma, 3.0 * sigma)
    return np.stack([jac[0] * g[:, 0] + jac[1] * g[:, 1], jac[2] * g[:, 0] + jac[3] * g[:, 1]], axis=1)


def test_closed_forms_agree_on_the_host():
    worst = 0.0
    for nfft, cx, cy, n in CASES:
        d = knot_cloud(n, 100 + n)
        assert kc.margin_in_sigmas(nfft, cx, cy, d, SIGMA_PSF, cf.PIXEL_SCALE) >= 8.0
        got = kc.numpy_pipeline(nfft, cx, cy, d, SIGMA_PSF, cf.PIXEL_SCALE, 1.0)
        want = kc.image_ref(nfft, cx, cy, d, SIGMA_PSF, cf.PIXEL_SCALE, 1.0)
        err = float(np.abs(got - want).max())
        tol = cf.omitted_alias_bound(SIGMA_PSF, nfft, 0, cf.PIXEL_SCALE) + ROUNDING
        print(f"N {n} grid {nfft}: numpy restatement against image_ref {err:.3e} per unit flux, allowed {tol:.3e}")
        assert err <= tol
        assert abs(want.sum() - 1.0) < 1.0e-12
        worst = max(worst, err)
    assert worst > 0.0
    # S_ref: one knot is a pure phase, two knots at +-d a cosine, and S(0, 0) = 1
    re, im = kc.S_ref([[0.3, -0.2]], 32, 0.2)
    np.testing.assert_allclose(np.hypot(re, im).astype(np.float64), 1.0, rtol=0, atol=4.0 * kc.EPS)
    re, im = kc.S_ref([[0.3, -0.2], [-0.3, 0.2]], 32, 0.2)
    assert float(np.abs(im).max()) <= 4.0 * kc.EPS and re[0, 0] == 1.0
    dk = 2.0 * math.pi / (32 * 0.2)
    assert abs(float(re[3, 5]) - math.cos(5 * dk * 0.3 - 3 * dk * 0.2)) <= 8.0 * kc.EPS
    assert abs(float(re[29, 5]) - math.cos(5 * dk * 0.3 + 3 * dk * 0.2)) <= 8.0 * kc.EPS         # row 29 is ky = -3 dk
