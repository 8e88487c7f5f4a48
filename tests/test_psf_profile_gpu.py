"""ims_psf_profile / psf_profile.profile on the GPU: the counts against the numpy restatement of the binning rule applied to the
photon pool of the same rows (integer for integer, no tolerance), determinism, centres, points that lose every photon, the
perturbed-telescope and optical-screen variants, output.psf_profile through the config driver, and a Gaussian's closed form.

The rows, scenes and the pool are those of tests/test_psf_map_gpu.py.  seg_size is not a free parameter of the renderer (the
library accepts 256 only), so the launch geometry is varied through the table instead: a row alone, in a table of 40, and in
the reversed table fall into different runs of different workgroups."""
import math
import os

import numpy as np
import pytest

import test_psf_map_gpu as PM
from test_psf_map_gpu import renderers, torch_cuda                      # noqa: F401  (fixtures)
from imsim_amd import _abi, config, configs, diffraction, fits_io, optics, psf_map, psf_profile
from psf_profile_ref import binning_reference, counts_reference

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((1, 0), (7, 3), (32, 8), (64, 64))


def rows_of(renderers, stage, n):
    sc, r = renderers[stage]
    return sc, r, (PM.stage1_rows(n) if stage == "psf" else PM.stage2_rows(sc, n))


def pool_offsets(r, rows):
    """(dx, dy, flux, offsets into them per row) of the rows' photons, from the unconverted pool as test_psf_map_gpu fetches it"""
    pool = r.shoot_ops_photons(rows, converted=False)
    r.synchronize()
    pool = pool.to_host()
    offs = np.concatenate([[0], np.cumsum(rows["n_phot"])])
    x0, y0 = np.repeat(rows["x0"], rows["n_phot"]), np.repeat(rows["y0"], rows["n_phot"])
    return pool["x"] - x0, pool["y"] - y0, pool["flux"], offs


def bins_from_pool(dx, dy, flux, n_r, n_phi):
    """Squared edges and directions for the pool at hand: log-spaced radii between the 2 % and 98 % quantiles of the arrived
    photons (so the underflow and overflow bins fill), one inner edge replaced by the r2 of an actual photon (the `<=` of the
    rule decides it) and direction 0 an exact power-of-two multiple of an actual photon's offset (t_0 = 0 for it)."""
    ok = flux != 0
    r2 = (dx * dx + dy * dy)[ok]
    lo, hi = np.sqrt(np.quantile(r2, 0.02)), np.sqrt(np.quantile(r2, 0.98))
    r_edges = psf_profile.radial_edges(lo, hi, n_r, "log")
    e2 = r_edges * r_edges
    m = max(1, n_r // 2)
    upper = e2[m + 1] if m + 1 <= n_r else np.inf
    pick = np.flatnonzero((r2 > e2[m - 1]) & (r2 < upper))[0]
    e2[m] = r2[pick]
    if n_phi == 0:
        return r_edges, e2, np.zeros((0, 2)), pick
    px, py = dx[ok][pick + 1], dy[ok][pick + 1]
    dirs = psf_profile.sector_dirs(n_phi, math.atan2(py, px))
    scale = 2.0 ** -math.frexp(max(abs(px), abs(py)))[1]
    dirs[0] = (px * scale, py * scale)
    return r_edges, e2, dirs, pick


def run_profile(r, rows, stage, r_edges, e2, dirs, centre=None):
    run = psf_profile.Prepared(r, rows, stage, r_edges, dirs=dirs, r2_edges=e2, centre=centre)
    run()
    return run.result()


def assert_equals_pool(res, dx, dy, flux, offs, e2, dirs, what, centre=None):
    for i in range(len(offs) - 1):
        sl = slice(offs[i], offs[i + 1])
        cx, cy = (0.0, 0.0) if centre is None else centre[i]
        ref, dropped = counts_reference(dx[sl] - cx if centre is not None else dx[sl], dy[sl] - cy if centre is not None else dy[sl],
                                        flux[sl], e2, dirs)
        assert np.array_equal(res.counts[i], ref), (what, i, int(np.abs(res.counts[i] - ref).sum()))
        assert res.n_dropped[i] == dropped and res.n_used[i] == ref.sum(), (what, i)


@pytest.mark.parametrize("stage", ["psf", "ops"])
def test_counts_equal_the_binned_pool(renderers, stage):
    """40 rows with every photon count of the table (1, 63, 64, 65, 257, 1000, 2^16 + 1), every fourth based above 2^32: the
    counts equal binning_reference of the pool's offsets and `dropped` the pool's zero-flux count, for every shape; each row's
    counts sum to n_used, which is ims_psf_moments' count for the same rows."""
    sc, r, rows = rows_of(renderers, stage, 40)
    assert set(rows["n_phot"]) == set(PM.COUNTS) and (rows["phot_first"] > 2 ** 32).sum() == 10
    dx, dy, flux, offs = pool_offsets(r, rows)
    moments = psf_map.compute(sc, rows, stage=stage, renderer=r)
    for n_r, n_phi in SHAPES:
        r_edges, e2, dirs, pick = bins_from_pool(dx, dy, flux, n_r, n_phi)
        res = run_profile(r, rows, stage, r_edges, e2, dirs)
        assert res.counts.shape == (40, n_r + 2, n_phi + 1) and res.counts.dtype == np.int64
        assert_equals_pool(res, dx, dy, flux, offs, e2, dirs, (stage, n_r, n_phi))
        assert np.array_equal(res.n_used, moments["n_used"]) and np.array_equal(res.n_dropped, moments["n_dropped"])
        assert np.array_equal(res.n_used + res.n_dropped, rows["n_phot"])
        tot = res.counts.sum(axis=0)
        assert tot[0].sum() > 0 and tot[-1].sum() > 0                       # underflow and overflow are exercised
        # the photon whose r2 is an edge sits in the bin above that edge, the one along direction 0 in sector 0
        ok = flux != 0
        m = max(1, n_r // 2)
        ri, si = binning_reference(dx[ok][pick:pick + 2], dy[ok][pick:pick + 2], e2, dirs)
        assert ri[0] == m + 1 and (n_phi == 0 or si[1] == 0)
    if stage == "ops":
        assert res.n_dropped.sum() > 0                                      # the annulus does lose photons


@pytest.mark.parametrize("stage", ["psf", "ops"])
def test_determinism_and_row_order(renderers, stage):
    """two calls give equal counts; a multi-workgroup row alone gives what it gives in the table of 40; the reversed table gives
    the reversed counts"""
    sc, r, rows = rows_of(renderers, stage, 40)
    r_edges = psf_profile.radial_edges(0.05, 6.0, 32, "log")
    kw = dict(n_phi=8, phi0=0.3, stage=stage, renderer=r)
    a = psf_profile.profile(sc, rows, None, r_edges, **kw)
    b = psf_profile.profile(sc, rows, None, r_edges, **kw)
    c = psf_profile.profile(sc, rows[::-1].copy(), None, r_edges, **kw)
    assert a.n_used.sum() > 100_000 and a.counts[:, 1:-1].sum() > 50_000
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.n_dropped, b.n_dropped)
    assert np.array_equal(c.counts[::-1], a.counts) and np.array_equal(c.n_dropped[::-1], a.n_dropped)
    for i in (6, 35, 3):                                                    # the two long rows and a short one
        alone = psf_profile.profile(sc, rows[i:i + 1].copy(), None, r_edges, **kw)
        assert np.array_equal(alone.counts[0], a.counts[i]) and alone.n_dropped[0] == a.n_dropped[i]


def test_centres(renderers):
    """an [n][2] centre shifts the offsets before they are binned, as binning_reference of the shifted offsets says;
    centre="centroid" is the centroids of psf_map.compute passed as that array"""
    sc, r, rows = rows_of(renderers, "ops", 12)
    dx, dy, flux, offs = pool_offsets(r, rows)
    r_edges, e2, dirs, _ = bins_from_pool(dx, dy, flux, 32, 8)
    i = np.arange(12)
    centre = np.stack([0.37 * np.cos(i), -0.21 + 0.05 * i], axis=1)
    res = run_profile(r, rows, "ops", r_edges, e2, dirs, centre=centre)
    assert_equals_pool(res, dx, dy, flux, offs, e2, dirs, "centre", centre=centre)
    plain = run_profile(r, rows, "ops", r_edges, e2, dirs)
    assert not np.array_equal(plain.counts, res.counts) and np.array_equal(plain.n_used, res.n_used)
    m = psf_map.compute(sc, rows, stage="ops", renderer=r)
    cen = np.stack([m["xbar"], m["ybar"]], axis=1)
    a = psf_profile.profile(sc, rows, None, r_edges, n_phi=8, centre="centroid", stage="ops", renderer=r)
    b = psf_profile.profile(sc, rows, None, r_edges, n_phi=8, centre=cen, stage="ops", renderer=r)
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.centre, cen) and a.n_used.sum() > 0


def test_rows_without_photons(renderers):
    """a row of 0 photons, and a stage-2 row 6e4 pixels off the CCD whose photons are all vignetted (test_psf_map_gpu's point):
    zero counts and n_used 0; the neighbours are what they are without them"""
    sc, r = renderers["ops"]
    xy = np.array([[20.5, 30.25], [6.0e4, 32.0], [40.0, 12.5], [11.0, 50.0]])
    rows = psf_map.point_rows(sc, xy, [1000, 1000, 0, 700], "ops")
    r_edges = psf_profile.radial_edges(0.0, 8.0, 16, "linear")
    res = psf_profile.profile(sc, rows, None, r_edges, n_phi=5, stage="ops", renderer=r)
    assert not res.counts[1].any() and (res.n_used[1], res.n_dropped[1]) == (0, 1000)
    assert not res.counts[2].any() and (res.n_used[2], res.n_dropped[2]) == (0, 0)
    r.synchronize()                                                          # (raises on a device-side error)
    others = psf_profile.profile(sc, rows[[0, 3]].copy(), None, r_edges, n_phi=5, stage="ops", renderer=r)
    assert np.array_equal(res.counts[[0, 3]], others.counts) and res.n_used[0] > 900 and res.n_used[3] > 600
    assert np.all(np.isnan(psf_profile.ee_radius(res, 0.5)[[1, 2]])) and np.all(np.isfinite(psf_profile.ee_radius(res, 0.5)[[0, 3]]))


def perturbed_scene():
    """scene_c3 with test_optical_screen_gpu's perturbed telescope (M2 shifted by 50 um): the photon kernels' perturbed layout"""
    sc = configs.scene_c3(nx=64, ny=64, sensor=False)
    tel = optics.apply_perturbations(optics.rubin_like_telescope(configs.VISIT["band"]), [{"M2": {"shift": [50e-6, 0.0, 0.0]}}])
    n = 64
    fp = (100.0, 0.0, (n - 1) / 2.0 + 0.5, 0.0, 100.0, (n - 1) / 2.0 + 0.5)
    po = optics.make_optics(tel, fp, math.radians(configs.VISIT["rottelpos"]))
    assert isinstance(po, _abi.OpticsPerturbed)
    po.img_wcs, po.icrf_to_field = sc.optics.img_wcs, sc.optics.icrf_to_field
    diffraction.fill_optics(po, math.radians(configs.VISIT["latitude"]), math.radians(configs.VISIT["azimuth"]),
                            math.radians(configs.VISIT["altitude"]))
    sc.optics = po
    return sc


def doopt_scene():
    """test_psf_map_gpu's optical-screen scene: the doOpt component alone, an astigmatism linear in the field angle"""
    sc = configs.scene_c3b(nx=64, ny=64, sensor=False, screen_size=102.4, screen_scale=0.1, optical=PM.ON)
    sc.atm.opt.field_matrix[2, 1] = 2.0
    sc.atm.opt.field_matrix[0, 0] = 4.0
    sc.psf, sc.ops = [sc.atm.optical_component()], []
    return sc


@pytest.mark.parametrize("which", ["perturbed", "doOpt"])
def test_other_kernel_variants_against_their_own_pools(torch_cuda, which):
    """one row each of a perturbed telescope (stage ops, the loops over surfaces in their frames) and of the optical phase screen
    (stage psf, the component's LDS set up per row): the counts equal the binned pool of the same scene"""
    if which == "perturbed":
        sc, stage = perturbed_scene(), "ops"
        rows = psf_map.point_rows(sc, np.array([[30.0, 20.0]]), 5000, stage)
    else:
        sc, stage = doopt_scene(), "psf"
        rows = psf_map.point_rows(sc, np.array([[10.0, 20.0]]), 5000, stage, wavelength=620.0)
        rows["atm_tan_x"], rows["atm_tan_y"] = np.radians(1.0), 0.0
        rows["x0"], rows["y0"] = 0.0, 0.0
    r = psf_map.renderer_for(sc)
    dx, dy, flux, offs = pool_offsets(r, rows)
    r_edges, e2, dirs, _ = bins_from_pool(dx, dy, flux, 32, 8)
    res = run_profile(r, rows, stage, r_edges, e2, dirs)
    assert_equals_pool(res, dx, dy, flux, offs, e2, dirs, which)
    assert res.n_used[0] > 4000 and res.counts[0, 1:-1].sum() > 4000


def test_config_end_to_end(torch_cuda, tmp_path, monkeypatch):
    """A one-CCD visit with output.psf_profile (nx 2, 20 000 photons, stage ops): the file is listed; its first HDU is the cube
    profile() returns for the same scene, points and seed; the second, a binary table, holds n_used, n_dropped and the EE radii
    of ee_radius."""
    seen = []
    real = psf_profile.profile

    def spy(scene, points, n_photons, r_edges, **kw):
        seen.append((scene, np.array(points), n_photons, np.array(r_edges), kw))
        return real(scene, points, n_photons, r_edges, **kw)
    monkeypatch.setattr(psf_profile, "profile", spy)
    o = {"input.instance_catalog.file_name": os.path.join(HERE, "golden", "example_instcat_subset.txt"),
         "image.nobjects": 3, "stamp.draw_method": "phot", "output.dir": str(tmp_path), "image.xsize": 64, "image.ysize": 64,
         "output.psf_profile": {"file_name": "psf_profile.fits", "nx": 2, "n_photons": 20000, "stage": "ops", "r_min": 0.0, "r_max": 6.0,
                                "n_r": 24, "spacing": "linear", "n_phi": 6, "phi0": "15 deg", "centre": "centroid"}}
    res = config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")], overrides=o)
    fn = str(tmp_path / "psf_profile.fits")
    assert fn in res.files and not any("psf_profile" in s for s in res.ignored)
    hdus = fits_io.read_fits(fn)
    assert len(hdus) == 2 and len(seen) == 1
    (h, cube), (h2, summ) = hdus
    scene, pts, n_photons, r_edges, kw = seen[0]
    assert (scene.nx, scene.ny) == (64, 64) and pts.tolist() == psf_map.grid_points(64, 64, 2).tolist() and n_photons == 20000
    again = real(scene, pts, 20000, r_edges, **kw)
    assert cube.dtype == np.float64 and cube.shape == (4, 26, 7) and np.array_equal(cube, again.counts.astype(np.float64))
    assert (h["STAGE"], h["NPHOT"], h["DET_NAME"], h["UNITS"], h["N_R"], h["N_PHI"], h["CENTRE"]) == \
        ("ops", 20000, res.det_names[0], "pixel", 24, 6, "centroid")
    assert h["PHI0"] == 15.0 * math.pi / 180.0 and h["WAVELEN"] > 300.0
    assert [h[f"R_EDGE{k}"] for k in range(25)] == (0.25 * np.arange(25)).tolist()
    assert (h2["XTENSION"], h2["EXTNAME"], h2["DET_NAME"]) == ("BINTABLE", "SUMMARY", res.det_names[0])
    assert list(summ) == list(psf_profile.SUMMARY) and summ["n_used"].dtype == np.int64 and summ["EE50"].dtype == np.float64
    summ = np.stack([np.asarray(summ[name], dtype=np.float64) for name in psf_profile.SUMMARY], axis=1)
    assert summ.shape == (4, 5) and np.array_equal(summ[:, 0], again.n_used) and np.array_equal(summ[:, 1], again.n_dropped)
    assert np.all(summ[:, 0] + summ[:, 1] == 20000) and np.all(summ[:, 0] > 18000)
    for k, frac in ((2, 0.5), (3, 0.8), (4, 0.95)):
        assert np.array_equal(summ[:, k], psf_profile.ee_radius(again, frac), equal_nan=True)
    assert np.all(np.isfinite(summ[:, 2])) and np.all(summ[:, 2] < summ[:, 3])


GAUSS_SEED = 398414


def gaussian_chi2(counts, sigma, r_edges, n):
    """(radial chi-square, dof, azimuthal chi-square, dof) of a [n_r + 2][n_phi + 1] table of n photons against the Gaussian's
    multinomial law: P(r_b <= r < r_b+1) = exp(-r_b^2 / 2 s^2) - exp(-r_b+1^2 / 2 s^2), the overflow bin the rest (the first
    edge is 0: no underflow); sectors uniform"""
    radial = counts.sum(axis=1)[1:].astype(np.float64)                       # n_r bins and the overflow
    s = np.exp(-np.asarray(r_edges) ** 2 / (2.0 * sigma * sigma))
    p = np.concatenate([s[:-1] - s[1:], [s[-1]]])
    chi_r = (((radial - n * p) ** 2) / (n * p)).sum()
    az = counts.sum(axis=0)[:-1].astype(np.float64)
    n_az = az.sum()
    chi_a = (((az - n_az / len(az)) ** 2) / (n_az / len(az))).sum()
    return chi_r, len(p) - 1, chi_a, len(az) - 1


def test_gaussian_closed_form(torch_cuda):
    """A pure Gaussian of sigma s, 1e6 photons, 16 linear bins out to 4 s, 8 sectors: the radial chi-square against the
    multinomial law and the azimuthal one against the uniform law each lie within 5 sqrt(2 dof) of their dof.  Seed 398414
    (test_psf_map_gpu's): the same two chi-squares formed on the CPU from tests/photon_source_ref.py's photons for this seed,
    binned by binning_reference, are 16.33 (dof 16) and 3.55 (dof 7) -- the reference alone passes."""
    n, sigma = 1_000_000, 0.7 / 2.3548200450309493
    psf = [(_abi.IMS_PSF_GAUSSIAN, 0, sigma, 0.0, 1.0)]
    r_edges = psf_profile.radial_edges(0.0, 4.0 * sigma, 16, "linear")
    res = psf_profile.profile(psf, np.zeros((1, 2)), n, r_edges, n_phi=8, stage="psf", wavelength=620.0, seed=GAUSS_SEED)
    assert res.n_used[0] == n and res.n_dropped[0] == 0 and res.counts[0, 0].sum() == 0 and res.counts[0, :, 8].sum() == 0
    chi_r, dof_r, chi_a, dof_a = gaussian_chi2(res.counts[0], sigma, r_edges, n)
    print(f"radial chi2 {chi_r:.2f} (dof {dof_r}), azimuthal chi2 {chi_a:.2f} (dof {dof_a})")
    assert abs(chi_r - dof_r) <= 5.0 * math.sqrt(2.0 * dof_r)
    assert abs(chi_a - dof_a) <= 5.0 * math.sqrt(2.0 * dof_a)
