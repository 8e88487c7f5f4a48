"""The oracle of the FFT branch (oracle/orc_fft.c + numpy.fft) against closed forms that share nothing with it
(tests/fft_closed_forms.py).  The oracle restates csrc/ims_fft.h line for line, so a convention both had wrong -- the sign of
the centring phase, half a pixel, the pixel response, which way `jac` acts, prof_scale, the alias sum -- passes every bit-exact
comparison of the two; here the oracle alone is held to the bounds the GPU tests (tests/test_fft_edges_gpu.py) then hold the
kernels to.

Measured (worst pixel over the grids of a case, per unit flux; the bound the same way):
  point source, Gaussian sigma 0.5"  (n_alias 0): error 1.9e-16, bound 2.6e-16 (aliases) + 1e-13 (rounding)
  point source, Gaussian sigma 0.2"  (n_alias 1): error 2.7e-16, bound 3.5e-22 + 1e-13
  point source, Gaussian sigma 0.12" (n_alias 1): error 1.5e-9,  bound 2.6e-9 + 1e-13; with n_alias forced to 0 the miss is
                                                  9.7e-3 .. 1.3e-2, 3.9e6 times the tolerance or more
  point source, Gaussian sigma 0.08" (n_alias 2): error 4.5e-11, bound 6.4e-11 + 1e-13
  sheared Gaussian k-table, sigma 0.3":           error 5.0e-6 (2.3e-4 of the peak), bound 5.2e-5 + 1e-13 (table interpolation);
                                                  the reference with M^T M misses by 1.4e-3 (6.8e-2 of the peak), 28 times the
                                                  tolerance; `jac` doubled with prof_scale 0.5 gives the same image to 7e-18"""
import numpy as np
import pytest

from imsim_amd import _abi, catalog, configs, fft_draw, tables
from oracle import orc_loader
import fft_closed_forms as cf

ROUNDING = 1.0e-13          # per unit flux: a pixel is a sum of n^2 <= 96^2 terms of at most 1 / n^2, each good to a few ulp


def gaussian_kpsf(sigma):
    return [(_abi.IMS_KPSF_GAUSSIAN, 0, sigma)]


def oracle_images(kpsf, rows, n_alias=None, **kw):
    orc = orc_loader.OracleFft(configs.scene_c2(nx=256, ny=256), kpsf, add_noise=False, **kw)
    if n_alias is not None:
        orc.P.n_alias = n_alias
    return orc, cf.grids(rows, orc.inverse(rows, orc.fill(rows)))


def test_alias_orders_of_the_psfs_the_edge_tests_use():
    q_step = float(np.diff(tables.sersic_ktable(1.0)[0][:2])[0])
    kt = np.stack([tables.sersic_ktable(1.0)[1], tables.sersic_ktable(4.0)[1]])
    for sigma, m in cf.ALIAS_ORDERS.items():
        assert fft_draw.alias_order(gaussian_kpsf(sigma), kt, q_step) == m
        assert orc_loader.OracleFft(configs.scene_c2(nx=64, ny=64), gaussian_kpsf(sigma)).P.n_alias == m
    kpsf = fft_draw.kolmogorov_gaussian_kpsf(*catalog.kolmogorov_gaussian_fwhm(airmass=1.0, raw_seeing=0.5))
    assert fft_draw.alias_order(kpsf, kt, q_step) == 1
    # and the default PSF, which every other FFT test draws with, folds nothing
    assert fft_draw.alias_order(fft_draw.kolmogorov_gaussian_kpsf(*catalog.kolmogorov_gaussian_fwhm()), kt, q_step) == 0


@pytest.mark.parametrize("sigma", cf.POINT_SIGMAS)
def test_oracle_point_source_through_a_gaussian_is_the_erf_pixel_integral(sigma):
    rows = cf.point_rows()
    orc, got = oracle_images(gaussian_kpsf(sigma), rows)
    m = cf.ALIAS_ORDERS[sigma]
    assert orc.P.n_alias == m
    worst = 0.0
    for o, img, want in zip(rows, got, cf.point_references(rows, sigma)):
        n, flux = int(o["nfft"]), float(o["flux"])
        bound = cf.omitted_alias_bound(sigma, n, m, cf.PIXEL_SCALE)
        err = np.abs(img - want).max()
        print(f"sigma {sigma} grid {n}: error {err / flux:.3e} bound {bound:.3e} per unit flux")
        assert err <= (bound + ROUNDING) * flux
        worst = max(worst, err / flux)
    assert worst > 0.0 or sigma == 0.5                         # (the comparison is of two different computations)


def test_oracle_without_its_aliases_misses_the_erf_form():
    """sigma 0.12": the case can see a fill that leaves the aliases out"""
    sigma = 0.12
    rows = cf.point_rows()
    orc, got = oracle_images(gaussian_kpsf(sigma), rows, n_alias=0)
    for o, img, want in zip(rows, got, cf.point_references(rows, sigma)):
        n, flux = int(o["nfft"]), float(o["flux"])
        tol = (cf.omitted_alias_bound(sigma, n, cf.ALIAS_ORDERS[sigma], cf.PIXEL_SCALE) + ROUNDING) * flux
        miss = np.abs(img - want).max()
        print(f"grid {n}: n_alias 0 misses by {miss / flux:.3e} per unit flux, {miss / tol:.3g} x tolerance")
        assert miss > 100.0 * tol


def test_oracle_sheared_gaussian_profile_is_the_elliptical_gaussian():
    q, _ = tables.sersic_ktable(1.0)
    q_step = float(q[1] - q[0])
    rows = cf.shear_rows()
    orc, got = oracle_images(gaussian_kpsf(cf.SHEAR_SIGMA), rows, extra_ktables=[np.exp(-0.5 * q * q)])
    assert orc.P.ktables.n_tables == 3
    bound = cf.interp_bound(q_step, cf.SHEAR_SIGMA, cf.SHEAR_GRID[0], cf.PIXEL_SCALE)
    for o, img, want, wrong in zip(rows, got, cf.shear_references(rows), cf.shear_references(rows, transposed=True)):
        flux = float(o["flux"])
        tol = (bound + ROUNDING) * flux
        err, miss = np.abs(img - want).max(), np.abs(img - wrong).max()
        print(f"prof_scale {float(o['prof_scale'])}: error {err / flux:.3e} ({err / want.max():.2e} of the peak) bound {bound:.3e}; "
              f"M^T M misses by {miss / flux:.3e} ({miss / want.max():.2e} of the peak), {miss / tol:.3g} x tolerance")
        assert err <= tol
        assert miss > 10.0 * tol
    # `jac` doubled and prof_scale halved: the same profile
    same = np.abs(got[0] / rows["flux"][0] - got[1] / rows["flux"][1]).max()
    print(f"jac x 2, prof_scale / 2: {same:.3e} per unit flux")
    assert same <= ROUNDING
