"""The FFT branch's kernels (k_fft_kspace_fill, the inverse transform, k_fft_bbox, the spike kernels, k_fft_finish) where the
parity tests do not go: against closed forms that share nothing with the oracle, on the alias-folding path of the fill, and on
stamps that hang over a CCD that is not square.

(a), (b): the real-space images of a draw against tests/fft_closed_forms.py, to the bounds tests/test_fft_closed_forms.py holds the
oracle to (there with 1e-13 of the flux for rounding, here with the project's 1e-11 of the peak for rocFFT against numpy).
(c): the fill with ims_fft_params_t.n_alias > 0 (kspace_value's (2 m + 1)^2 sum instead of kspace_pair and its LDS tables), bit
for bit against the oracle.  (d): what k_fft_finish adds to the CCD image said in numpy.
(e): the spike step on a stamp that cuts the saturated core.

Measured, worst pixel over the grids of a case, per unit flux, for the oracle on the host (tests/test_fft_closed_forms.py); every
test here prints the same figures for the kernels (pytest -s), which have NOT been recorded on an MI355X yet:
  case                                   bound     + 1e-11 of the peak   oracle error   wrong answer misses by
  point, Gaussian 0.5"  (n_alias 0)      2.6e-16   2.5e-13               1.9e-16
  point, Gaussian 0.2"  (n_alias 1)      3.5e-22   1.4e-12               2.7e-16
  point, Gaussian 0.12" (n_alias 1)      2.6e-9    3.1e-12               1.5e-9         n_alias 0: 9.7e-3, 3.9e6 x the tolerance
  point, Gaussian 0.08" (n_alias 2)      6.4e-11   4.9e-12               4.5e-11
  sheared Gaussian k-table, 0.3"         5.2e-5    2.1e-13               5.0e-6         M^T M: 1.4e-3, 28 x the tolerance
(the sheared case's error is 2.3e-4 of the peak, its wrong answer 6.8e-2 of the peak)"""
import math

import numpy as np
import pytest

from helpers import assert_bits_equal
from imsim_amd import _abi, catalog, configs, fft_draw, tables
from oracle import orc_loader
import fft_closed_forms as cf

pytestmark = pytest.mark.gpu

FFT_VS_NUMPY = 1.0e-11        # of the peak: rocFFT against numpy.fft (test_fft_branch_matches_oracle)
REALIZED_RTOL = 1.0e-12       # realized fluxes: sums of the same values by atomic adds, in any order


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def gaussian_kpsf(sigma):
    return [(_abi.IMS_KPSF_GAUSSIAN, 0, sigma)]


def draw(torch, scene, kpsf, rows, n_alias=None, keep_kspace=False, **kw):
    """one draw on a fresh renderer -> (renderer, drawer, half spectra or None, real-space images, realized fluxes)"""
    from imsim_amd.engine import Renderer
    r = Renderer(scene)
    drawer = fft_draw.FftDrawer(r, kpsf, **kw)
    if n_alias is not None:
        drawer.P.n_alias = n_alias
    drawer.keep_kspace = keep_kspace
    real = torch.zeros(len(rows), dtype=torch.float64, device="cuda")
    kbuf, rbuf = drawer.draw(rows, realized=real)
    r.synchronize()
    return (r, drawer, kbuf.cpu().numpy() if keep_kspace else None, fft_draw.image_from_rbuf(rows, rbuf.cpu().numpy()),
            real.cpu().numpy())


# ---------------------------------------------------------------------------------------------
# (a) point source through a Gaussian PSF: the erf pixel integrals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", cf.POINT_SIGMAS)
def test_point_source_through_a_gaussian_is_the_erf_pixel_integral(torch_cuda, sigma):
    """sigma 0.5": kspace_pair and the LDS tables; the others: kspace_value's alias sum (n_alias 1, 1, 2)"""
    scene = configs.scene_c2(nx=256, ny=256)
    rows = cf.point_rows()
    m = cf.ALIAS_ORDERS[sigma]
    r, drawer, _, image, _ = draw(torch_cuda, scene, gaussian_kpsf(sigma), rows, add_noise=False)
    assert drawer.P.n_alias == m
    wants = cf.point_references(rows, sigma)
    tols = []
    for o, img, want in zip(rows, cf.grids(rows, image), wants):
        n, flux = int(o["nfft"]), float(o["flux"])
        bound = cf.omitted_alias_bound(sigma, n, m, cf.PIXEL_SCALE)
        tols.append(bound * flux + FFT_VS_NUMPY * want.max())
        err = np.abs(img - want).max()
        print(f"sigma {sigma} grid {n}: error {err / flux:.3e}, bound {bound:.3e} + {FFT_VS_NUMPY * want.max() / flux:.3e} per unit flux")
        assert err <= tols[-1]
    if sigma == 0.12:
        # the case can see a fill that leaves the aliases out
        _, _, _, image0, _ = draw(torch_cuda, scene, gaussian_kpsf(sigma), rows, n_alias=0, add_noise=False)
        for o, img, want, tol in zip(rows, cf.grids(rows, image0), wants, tols):
            miss = np.abs(img - want).max()
            print(f"grid {int(o['nfft'])}: n_alias 0 misses by {miss / float(o['flux']):.3e} per unit flux, {miss / tol:.3g} x tolerance")
            assert miss > 100.0 * tol


# ---------------------------------------------------------------------------------------------
# (b) a sheared Gaussian profile from a k-table: the elliptical Gaussian of covariance M M^T + sigma^2 I
# ---------------------------------------------------------------------------------------------
def test_sheared_gaussian_profile_is_the_elliptical_gaussian(torch_cuda):
    q, _ = tables.sersic_ktable(1.0)
    q_step = float(q[1] - q[0])
    scene = configs.scene_c2(nx=256, ny=256)
    rows = cf.shear_rows(prof_ktable=2)
    r, drawer, _, image, _ = draw(torch_cuda, scene, gaussian_kpsf(cf.SHEAR_SIGMA), rows, add_noise=False,
                                  extra_ktables=[np.exp(-0.5 * q * q)])
    assert drawer.P.ktables.n_tables == 3 and drawer.P.n_alias == 0
    bound = cf.interp_bound(q_step, cf.SHEAR_SIGMA, cf.SHEAR_GRID[0], cf.PIXEL_SCALE)
    for o, img, want, wrong in zip(rows, cf.grids(rows, image), cf.shear_references(rows), cf.shear_references(rows, transposed=True)):
        flux = float(o["flux"])
        tol = bound * flux + FFT_VS_NUMPY * want.max()
        err, miss = np.abs(img - want).max(), np.abs(img - wrong).max()
        print(f"prof_scale {float(o['prof_scale'])}: error {err / flux:.3e} ({err / want.max():.2e} of the peak), bound {bound:.3e}; "
              f"M^T M misses by {miss / flux:.3e} ({miss / want.max():.2e} of the peak), {miss / tol:.3g} x tolerance")
        assert err <= tol
        assert miss > 10.0 * tol


# ---------------------------------------------------------------------------------------------
# (c) the alias path, bit for bit against the oracle
# ---------------------------------------------------------------------------------------------
def _mixed_case(n_extra_ktables):
    """a star, n = 1 and n = 4 galaxies and one on an extra Sersic table of the scene, on grids of 6, 10, 32, 64, 96 and 128"""
    scene = configs.scene_c2(nx=256, ny=256)
    configs.add_sersic_tables(scene, [2.5])
    cat = dict(x=np.array([100.3, 60.0, 180.6, 128.5]), y=np.array([120.7, 200.2, 70.1, 40.9]), mag=np.zeros(4),
               nominal_flux=np.array([2.0e6, 5.0e6, 1.5e6, 3.0e6]), kind=np.array([0, 1, 2, 2]),
               hlr=np.array([0.0, 0.4, 0.8, 0.5]), q=np.array([1.0, 0.5, 0.8, 0.7]), pa=np.array([0.0, 30.0, 110.0, 20.0]),
               sersic_n=np.array([0.0, 0.0, 0.0, 2.5]), obj_id=np.arange(4))
    objects, _ = catalog.build_object_table(cat, cat["nominal_flux"].astype(np.int64), stamp_size=np.array([32, 128, 64, 64]),
                                            sersic_index=scene.sersic_index)
    kt = fft_draw.profile_ktable_ids(scene, objects["prof_table"], n_extra_ktables=n_extra_ktables)
    assert list(kt) == [-1, 0, 1, 2 + n_extra_ktables]
    rows, _ = fft_draw.build_fft_objects(objects, cat["nominal_flux"], kt)
    assert list(rows["nfft"]) == [32, 64, 64, 128]
    odd = rows[1:3].copy()
    odd["nfft"] = 96                                        # 3 * 32: the n = 4 and the n = 2.5 galaxy once more
    odd["obj_id"] += 10
    tiny = rows[:2].copy()                                  # the star and the n = 4 galaxy on grids of 36 and 100 pixels: wavefronts
    tiny["nfft"] = (6, 10)                                  # of every elementwise kernel straddle objects (walk_span's lane path)
    tiny["obj_id"] += 20
    tiny["x0"], tiny["y0"] = tiny["stamp_xmin"] + 20, tiny["stamp_ymin"] + 20
    tiny["cx"], tiny["cy"] = 2.3, 3.1
    rows = np.concatenate([tiny, odd, rows])
    rows = rows[np.argsort(rows["nfft"], kind="stable")]
    nf = rows["nfft"].astype(np.int64)
    rows["k_offset"] = np.concatenate([[0], np.cumsum(nf * (nf // 2 + 1))])[:-1]
    rows["r_offset"] = np.concatenate([[0], np.cumsum(nf * nf)])[:-1]
    assert list(nf) == [6, 10, 32, 64, 64, 96, 96, 128]
    return scene, rows


@pytest.mark.parametrize("psf", ["seeing-0.5", "gaussian-0.08"])
def test_alias_path_matches_oracle(torch_cuda, psf):
    extra = []
    if psf == "seeing-0.5":
        kpsf, want_alias = fft_draw.kolmogorov_gaussian_kpsf(*catalog.kolmogorov_gaussian_fwhm(airmass=1.0, raw_seeing=0.5)), 1
    else:
        kpsf, want_alias = gaussian_kpsf(0.08), 2
    scene, rows = _mixed_case(len(extra))
    r, drawer, kbuf, image, real = draw(torch_cuda, scene, kpsf, rows, keep_kspace=True, add_noise=True, extra_ktables=extra)
    orc = orc_loader.OracleFft(scene, kpsf, add_noise=True, extra_ktables=extra)
    print(f"{psf}: n_alias {drawer.P.n_alias}")
    assert drawer.P.n_alias == orc.P.n_alias == want_alias
    assert drawer.P.ktables.n_tables == orc.P.ktables.n_tables == 3 + len(extra)
    okbuf = orc.fill(rows)
    assert_bits_equal(kbuf, okbuf, f"k-space half spectra, {psf}")
    orbuf = orc.inverse(rows, okbuf)
    assert np.abs(image - orbuf).max() < FFT_VS_NUMPY * np.abs(orbuf).max()
    oreal = np.zeros(len(rows))
    orc.finish(rows, image, oreal)                          # noise + add of the SAME real-space images the GPU produced
    assert orc.image.sum() > 0
    assert_bits_equal(r.image_numpy(), orc.image.astype(np.float32), f"noisy FFT image, {psf}")
    np.testing.assert_allclose(real, oreal, rtol=REALIZED_RTOL)


# ---------------------------------------------------------------------------------------------
# (d) clipped stamps on a CCD that is not square
# ---------------------------------------------------------------------------------------------
NX, NY = 142, 255


def _clipped_rows():
    """CCD pixels 1 .. 142 by 1 .. 255.  No CCD pixel lies in more than two stamps: the 256-wide one and at most one other."""
    return cf.make_rows([
        dict(nfft=32, x0=-15, y0=40, cx=14.6, cy=15.3, flux=2.0e5),                 # over the left edge, centre just off the chip
        dict(nfft=32, x0=130, y0=40, cx=11.2, cy=17.7, flux=3.0e5),                 # over the right edge
        dict(nfft=32, x0=55, y0=-20, cx=16.4, cy=21.8, flux=2.5e5),                 # over the bottom edge
        dict(nfft=32, x0=55, y0=240, cx=15.9, cy=14.1, flux=1.5e5),                 # over the top edge
        dict(nfft=32, x0=-10, y0=-12, cx=11.7, cy=13.4, flux=4.0e5),                # over the corner (1, 1)
        dict(nfft=32, x0=125, y0=235, cx=17.3, cy=20.6, flux=3.5e5),                # over the corner (142, 255)
        dict(nfft=32, x0=200, y0=100, cx=16.1, cy=15.8, flux=5.0e5),                # wholly off the chip
        dict(nfft=64, x0=40, y0=80, cx=31.4, cy=31.7, flux=6.0e5, stamp=(55, 87, 95, 127)),     # stamp of 33: pads of 15 and 16
        dict(nfft=256, x0=-50, y0=-40, cx=120.3, cy=150.6, flux=8.0e5),             # 256 wide across the 142-pixel chip
    ])


OFF_CHIP = 6                   # position of the wholly-off-chip row (grids of 32 come first, in the order given)


def _ccd_statement(rows, image, nx, ny, xmin, ymin):
    """what k_fft_finish adds without noise: per row the real-space image clipped at 0, the pixels inside the stamp, those of them
    on the CCD at (px - xmin, py - ymin), added -> (CCD image, clipped sum over the whole stamp per row, pixels on the CCD per row)"""
    ccd = np.zeros((ny, nx))
    total, on_chip = np.zeros(len(rows)), np.zeros(len(rows), dtype=np.int64)
    for k, (o, g) in enumerate(zip(rows, cf.grids(rows, image))):
        n = int(o["nfft"])
        v = np.where(g < 0.0, 0.0, g)
        px, py = int(o["x0"]) + np.arange(n), int(o["y0"]) + np.arange(n)
        sx = np.flatnonzero((px >= o["stamp_xmin"]) & (px <= o["stamp_xmax"]))
        sy = np.flatnonzero((py >= o["stamp_ymin"]) & (py <= o["stamp_ymax"]))
        total[k] = v[np.ix_(sy, sx)].sum()
        sx = sx[(px[sx] - xmin >= 0) & (px[sx] - xmin < nx)]
        sy = sy[(py[sy] - ymin >= 0) & (py[sy] - ymin < ny)]
        on_chip[k] = len(sx) * len(sy)
        ccd[np.ix_(py[sy] - ymin, px[sx] - xmin)] += v[np.ix_(sy, sx)]
    return ccd, total, on_chip


def _coverage(rows, nx, ny, xmin, ymin):
    cover = np.zeros((ny, nx), dtype=np.int64)
    for o in rows:
        x0, x1 = max(int(o["stamp_xmin"]) - xmin, 0), min(int(o["stamp_xmax"]) - xmin, nx - 1)
        y0, y1 = max(int(o["stamp_ymin"]) - ymin, 0), min(int(o["stamp_ymax"]) - ymin, ny - 1)
        if x1 >= x0 and y1 >= y0:
            cover[y0:y1 + 1, x0:x1 + 1] += 1
    return cover


def test_clipped_stamps_on_a_ccd_that_is_not_square(torch_cuda):
    kpsf = fft_draw.kolmogorov_gaussian_kpsf(*catalog.kolmogorov_gaussian_fwhm())
    rows = _clipped_rows()
    assert rows["x0"][OFF_CHIP] == 200 and list(rows["nfft"]) == [32] * 7 + [64, 256]
    images = {}
    for origin in ((1, 1), (-20, 300)):
        scene = configs.scene_c2(nx=NX, ny=NY)
        assert (scene.xmin, scene.ymin) == (1, 1)
        scene.xmin, scene.ymin = origin
        moved = cf.shifted(rows, origin[0] - 1, origin[1] - 1)
        cover = _coverage(moved, NX, NY, *origin)
        assert cover.max() == 2 and cover.min() == 0         # two additions commute: the image does not depend on the atomics' order
        r, drawer, _, image, real = draw(torch_cuda, scene, kpsf, moved, add_noise=False)
        ccd, total, on_chip = _ccd_statement(moved, image, NX, NY, *origin)
        got = r.image64_numpy()
        assert got.shape == (NY, NX)
        assert_bits_equal(got, ccd, f"CCD image without noise, origin {origin}")
        np.testing.assert_allclose(real, total, rtol=REALIZED_RTOL)
        # parts of stamps off the chip count in the realized flux and not in the image
        assert on_chip[OFF_CHIP] == 0 and real[OFF_CHIP] > 0.0 and all(0 < on_chip[k] < 32 * 32 for k in range(6))
        assert on_chip[7] == 33 * 33 and on_chip[8] == NX * (NY - 40)
        assert math.fsum(got.ravel()) < math.fsum(real) - real[OFF_CHIP]
        images[origin] = got
    assert_bits_equal(images[(1, 1)], images[(-20, 300)], "CCD image, origin moved with every row")
    # the wholly-off-chip row alone: an image of zeros, its flux reported all the same
    alone = rows[OFF_CHIP:OFF_CHIP + 1].copy()
    alone["k_offset"] = alone["r_offset"] = 0
    r, drawer, _, image, real = draw(torch_cuda, configs.scene_c2(nx=NX, ny=NY), kpsf, alone, add_noise=False)
    assert not r.image64_numpy().any()
    np.testing.assert_allclose(real, [np.where(image < 0.0, 0.0, image).sum()], rtol=REALIZED_RTOL)
    # noise on: the oracle's finish of the GPU's own real-space images
    scene = configs.scene_c2(nx=NX, ny=NY)
    r, drawer, _, image, real = draw(torch_cuda, scene, kpsf, rows, add_noise=True)
    orc = orc_loader.OracleFft(scene, kpsf, add_noise=True)
    oreal = np.zeros(len(rows))
    orc.finish(rows, image, oreal)
    assert_bits_equal(r.image64_numpy(), orc.image, "noisy CCD image of clipped stamps")
    assert (orc.image != images[(1, 1)]).any()
    np.testing.assert_allclose(real, oreal, rtol=REALIZED_RTOL)


# ---------------------------------------------------------------------------------------------
# (e) spikes on a clipped stamp
# ---------------------------------------------------------------------------------------------
def test_spikes_on_a_stamp_that_cuts_the_saturated_core(torch_cuda, monkeypatch):
    """One star above DiffractionFFT's 1e5 threshold on a grid of 128 with a stamp of 100 (pads of 14): its centre 2.3 pixels inside
    the stamp's left edge, so that saturated pixels of the grid lie outside the stamp, and the stamp over the CCD's corner (1, 1)
    by 1 pixel along x and 30 along y.  The saturated box is taken over the stamp only."""
    from imsim_amd import diffraction_fft as dfft
    scene = configs.scene_c2(nx=NX, ny=NY)
    kpsf = fft_draw.kolmogorov_gaussian_kpsf(*catalog.kolmogorov_gaussian_fwhm())
    n, pad = 128, 14
    x0, y0 = 1 - pad - 1, 1 - pad - 30
    rows = cf.make_rows([dict(nfft=n, x0=x0, y0=y0, cx=pad + 2.3, cy=50.6, flux=4.0e7, obj_id=5,
                              stamp=(x0 + pad, x0 + pad + 99, y0 + pad, y0 + pad + 99))])
    cfg = dfft.DiffractionFFT(exptime=30.0, azimuth=math.radians(114.39), altitude=math.radians(53.16),
                              rotTelPos=math.radians(40.04), spike_length_cutoff=60)
    orc = orc_loader.OracleFft(scene, kpsf, add_noise=False, diffraction_fft=cfg, wavelength=622.2)
    finals = {}
    for listed in ("1", "0"):
        monkeypatch.setenv("IMS_FFT_SPIKE_LIST", listed)
        r, drawer, _, image, real = draw(torch_cuda, scene, kpsf, rows, add_noise=False, diffraction_fft=cfg, wavelength=622.2)
        assert (drawer._last[7] is None) == (listed == "0")
        final = drawer._last[2].cpu().numpy()
        ofinal = orc.spikes(rows, image)
        assert_bits_equal(final, ofinal, f"spiked image of a clipped stamp, IMS_FFT_SPIKE_LIST={listed}")
        r0, r1, c0, c1 = (int(v) for v in drawer._last[6].cpu().numpy()[:4])
        g = image.reshape(n, n)
        over = g > cfg.brightness_threshold
        assert over[:, :pad].any() and over[:, pad:].any()                 # saturated pixels on both sides of the stamp's edge
        assert pad <= c0 <= c1 < pad + 100 and pad <= r0 <= r1 < pad + 100      # the box: inside the stamp,
        inside = np.argwhere(over[pad:pad + 100, pad:pad + 100]) + pad          # around exactly its saturated pixels
        assert (r0, r1, c0, c1) == (inside[:, 0].min(), inside[:, 0].max(), inside[:, 1].min(), inside[:, 1].max())
        assert c0 == pad
        clipped = np.where(g < 0.0, 0.0, g)
        assert np.abs(final.reshape(n, n) - clipped).max() > 1.0           # the spike step did something,
        assert_bits_equal(final.reshape(n, n)[:, :pad], clipped[:, :pad], "pixels outside the stamp are left alone")
        # and the CCD image is the oracle's finish of the spiked image
        orc.image[:] = 0.0
        orc.finish(rows, ofinal, np.zeros(1))
        assert_bits_equal(r.image64_numpy(), orc.image, f"CCD image of the spiked stamp, IMS_FFT_SPIKE_LIST={listed}")
        finals[listed] = final
    assert_bits_equal(finals["1"], finals["0"], "listed against the one-launch form")
