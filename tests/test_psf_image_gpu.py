"""ims_psf_image / psf_image.images on the GPU: the counts against the numpy restatement of the binning rule applied to the photon
pool of the same rows (integer for integer, no tolerance) in all three stages, determinism, centres, points that lose every
photon, the perturbed-telescope and optical-screen variants, a Gaussian's closed form, what the sensor stage adds to the second
moment, and output.psf_image through the config driver.

The rows, scenes and pools are those of tests/test_psf_map_gpu.py and tests/test_psf_profile_gpu.py.  Stages psf and ops are held
to the unconverted pool of ims_shoot_ops_photons, stage sensor to the converted pool (position at the conversion depth, a photon
the sensor loses stored with flux 0).  The launch geometry is varied through the table: a row alone, in a table of 40, and in
the reversed table fall into different runs of different workgroups."""
import dataclasses
import math
import os

import numpy as np
import pytest

import test_psf_map_gpu as PM
import test_psf_profile_gpu as PP
from test_psf_map_gpu import renderers, torch_cuda                      # noqa: F401  (fixtures)
from imsim_amd import _abi, config, configs, fits_io, psf_image, psf_map
from psf_image_ref import cells_reference, counts_reference

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((8, 8), (64, 64), (65, 63), (200, 96), (1, 1))                 # (nx, ny): LDS only; window + global cells; one cell
WIN = 64


@pytest.fixture(scope="module")
def sensor_renderer(torch_cuda):
    """scene_c3 on 64 x 64 pixels with its Silicon sensor, and a renderer of it"""
    from imsim_amd.engine import Renderer
    sc = configs.scene_c3(nx=64, ny=64, sensor=True)
    return sc, Renderer(sc)


def rows_of(renderers, sensor_renderer, stage, n):
    if stage == "sensor":
        sc, r = sensor_renderer
        return sc, r, PM.stage2_rows(sc, n)
    return PP.rows_of(renderers, stage, n)


def pool_offsets(r, rows, stage):
    """(dx, dy, flux, offsets into them per row) of the rows' photons: the unconverted pool for stages psf and ops, the converted
    one for stage sensor"""
    if stage != "sensor":
        return PP.pool_offsets(r, rows)
    pool = r.shoot_ops_photons(rows, converted=True)
    r.synchronize()
    pool = pool.to_host()
    x, y, flux = pool["x"], pool["y"], pool["flux"]
    offs = np.concatenate([[0], np.cumsum(rows["n_phot"])])
    x0, y0 = np.repeat(rows["x0"], rows["n_phot"]), np.repeat(rows["y0"], rows["n_phot"])
    return x - x0, y - y0, flux, offs


def scale_from_pool(dx, dy, flux, nx, ny, q=0.98):
    """the cell side at which a fraction q of the arrived photons falls inside an nx x ny stamp"""
    ok = flux != 0
    return float(np.quantile(np.maximum(np.abs(dx[ok]) / (0.5 * nx), np.abs(dy[ok]) / (0.5 * ny)), q))


def run_image(r, rows, stage, size, scale, centre=None):
    run = psf_image.Prepared(r, rows, stage, size, scale, centre=centre)
    run()
    return run.result()


def assert_equals_pool(res, dx, dy, flux, offs, what, centre=None):
    ny, nx = res.counts.shape[1:]
    for i in range(len(offs) - 1):
        sl = slice(offs[i], offs[i + 1])
        x, y = (dx[sl], dy[sl]) if centre is None else (dx[sl] - centre[i][0], dy[sl] - centre[i][1])
        ref, outside, dropped = counts_reference(x, y, flux[sl], res.inv_scale, nx, ny)
        assert np.array_equal(res.counts[i], ref), (what, i, int(np.abs(res.counts[i] - ref).sum()))
        assert (res.n_outside[i], res.n_dropped[i], res.n_used[i]) == (outside, dropped, ref.sum()), (what, i)


def window_split(counts):
    """(photons in the cells of the 64 x 64 LDS window, photons in the other cells) of [n][ny][nx] counts"""
    ny, nx = counts.shape[1:]
    wx, wy = min(nx, WIN), min(ny, WIN)
    x0, y0 = (nx - wx) // 2, (ny - wy) // 2
    inside = int(counts[:, y0:y0 + wy, x0:x0 + wx].sum())
    return inside, int(counts.sum()) - inside


@pytest.mark.parametrize("stage", ["psf", "ops", "sensor"])
def test_counts_equal_the_binned_pool(renderers, sensor_renderer, stage):
    """40 rows with every photon count of the table (1, 63, 64, 65, 257, 1000, 2^16 + 1: rows shorter than a segment, rows that
    are no multiple of 256, two rows of 257 segments), every fourth based above 2^32: for every shape the counts equal
    counts_reference of the pool's offsets, `outside` and `dropped` with them, and each row's three numbers add up to its
    photons.  The scale puts 98 % of the pool inside the stamp, so that the LDS window holds most photons, the cells beside it
    (shapes beyond 64) some, and `outside` the rest: all three are asserted."""
    sc, r, rows = rows_of(renderers, sensor_renderer, stage, 40)
    assert set(rows["n_phot"]) == set(PM.COUNTS) and (rows["phot_first"] > 2 ** 32).sum() == 10
    dx, dy, flux, offs = pool_offsets(r, rows, stage)
    if stage != "psf":
        assert (flux == 0).sum() > 0                                        # the annulus does lose photons
    for nx, ny in SHAPES:
        scale = scale_from_pool(dx, dy, flux, nx, ny)
        res = run_image(r, rows, stage, (nx, ny), scale)
        assert res.counts.shape == (40, ny, nx) and res.counts.dtype == np.int64
        assert_equals_pool(res, dx, dy, flux, offs, (stage, nx, ny))
        assert np.array_equal(res.n_used + res.n_outside + res.n_dropped, rows["n_phot"])
        in_window, beside_window = window_split(res.counts)
        print(f"{stage} {nx} x {ny}: scale {scale:.4g}, window {in_window}, other cells {beside_window}, outside {res.n_outside.sum()}, "
              f"dropped {res.n_dropped.sum()}")
        assert in_window > 0.5 * rows["n_phot"].sum() and res.n_outside.sum() > 0
        assert (beside_window > 0) == (nx > WIN or ny > WIN)


def test_sensor_stage_leaves_the_other_stages_alone(sensor_renderer):
    """on a renderer with a sensor, stage ops still equals the unconverted pool: the sensor's random block is drawn in stage 3 only"""
    sc, r = sensor_renderer
    rows = PM.stage2_rows(sc, 12)
    dx, dy, flux, offs = pool_offsets(r, rows, "ops")
    res = run_image(r, rows, "ops", (65, 63), scale_from_pool(dx, dy, flux, 65, 63))
    assert_equals_pool(res, dx, dy, flux, offs, "ops on a sensor scene")
    sen = run_image(r, rows, "sensor", (65, 63), res.scale)
    assert not np.array_equal(sen.counts, res.counts) and np.array_equal(sen.n_dropped, res.n_dropped)


@pytest.mark.parametrize("stage", ["psf", "ops", "sensor"])
def test_determinism_and_row_order(renderers, sensor_renderer, stage):
    """two calls give equal stamps; a multi-workgroup row alone gives what it gives in the table of 40; the reversed table gives
    the reversed stamps (96 x 80 cells: the window and the global cells both)"""
    sc, r, rows = rows_of(renderers, sensor_renderer, stage, 40)
    kw = dict(stage=stage, renderer=r)
    a = psf_image.images(sc, rows, None, (96, 80), 0.25, **kw)
    b = psf_image.images(sc, rows, None, (96, 80), 0.25, **kw)
    c = psf_image.images(sc, rows[::-1].copy(), None, (96, 80), 0.25, **kw)
    assert a.n_used.sum() > 100_000 and a.n_outside.sum() > 0 and window_split(a.counts)[1] > 0
    for f in ("counts", "n_outside", "n_dropped"):
        assert np.array_equal(getattr(a, f), getattr(b, f)) and np.array_equal(getattr(c, f)[::-1], getattr(a, f)), f
    for i in (6, 35, 3):                                                    # the two long rows and a short one
        alone = psf_image.images(sc, rows[i:i + 1].copy(), None, (96, 80), 0.25, **kw)
        assert np.array_equal(alone.counts[0], a.counts[i])
        assert (alone.n_outside[0], alone.n_dropped[0]) == (a.n_outside[i], a.n_dropped[i])


def test_centres(renderers, sensor_renderer):
    """an [n][2] centre shifts the offsets before they are binned, as counts_reference of the shifted offsets says;
    centre="centroid" is the centroids of psf_map.compute passed as that array (stage sensor: those of stage ops)"""
    sc, r, rows = rows_of(renderers, sensor_renderer, "ops", 12)
    dx, dy, flux, offs = pool_offsets(r, rows, "ops")
    scale = scale_from_pool(dx, dy, flux, 70, 66)
    i = np.arange(12)
    centre = np.stack([0.37 * np.cos(i), -0.21 + 0.05 * i], axis=1)
    res = run_image(r, rows, "ops", (70, 66), scale, centre=centre)
    assert_equals_pool(res, dx, dy, flux, offs, "centre", centre=centre)
    plain = run_image(r, rows, "ops", (70, 66), scale)
    assert not np.array_equal(plain.counts, res.counts) and np.array_equal(plain.n_dropped, res.n_dropped)
    for stage, (sc, r) in (("ops", renderers["ops"]), ("sensor", sensor_renderer)):
        rows = PM.stage2_rows(sc, 12)
        m = psf_map.compute(sc, rows, stage="ops", renderer=r)
        cen = np.stack([m["xbar"], m["ybar"]], axis=1)
        a = psf_image.images(sc, rows, None, 32, 0.5, centre="centroid", stage=stage, renderer=r)
        b = psf_image.images(sc, rows, None, 32, 0.5, centre=cen, stage=stage, renderer=r)
        n = psf_image.images(sc, rows, None, 32, 0.5, centre="nominal", stage=stage, renderer=r)
        assert np.array_equal(a.counts, b.counts) and np.array_equal(a.centre, cen) and a.n_used.sum() > 0
        assert n.centre is None and not np.array_equal(n.counts, a.counts)


@pytest.mark.parametrize("stage", ["ops", "sensor"])
def test_rows_without_photons(renderers, sensor_renderer, stage):
    """a row of 0 photons, and a row 6e4 pixels off the CCD whose photons are all vignetted (test_psf_map_gpu's point): zero
    counts, nothing outside, n_dropped = n_phot; the neighbours are what they are without them"""
    sc, r = renderers["ops"] if stage == "ops" else sensor_renderer
    xy = np.array([[20.5, 30.25], [6.0e4, 32.0], [40.0, 12.5], [11.0, 50.0]])
    rows = psf_map.point_rows(sc, xy, [1000, 1000, 0, 700], "ops")
    res = psf_image.images(sc, rows, None, (80, 40), 0.25, stage=stage, renderer=r)
    assert not res.counts[1].any() and (res.n_used[1], res.n_outside[1], res.n_dropped[1]) == (0, 0, 1000)
    assert not res.counts[2].any() and (res.n_used[2], res.n_outside[2], res.n_dropped[2]) == (0, 0, 0)
    r.synchronize()                                                          # (raises on a device-side error)
    others = psf_image.images(sc, rows[[0, 3]].copy(), None, (80, 40), 0.25, stage=stage, renderer=r)
    assert np.array_equal(res.counts[[0, 3]], others.counts) and np.array_equal(res.n_outside[[0, 3]], others.n_outside)
    assert res.n_used[0] + res.n_outside[0] > 900 and res.n_used[3] + res.n_outside[3] > 600
    m = psf_image.moments(res)
    assert np.all(np.isnan(m["sigma"][[1, 2]])) and np.all(np.isfinite(m["sigma"][[0, 3]]))


@pytest.mark.parametrize("which", ["perturbed", "perturbed-sensor", "doOpt"])
def test_other_kernel_variants_against_their_own_pools(torch_cuda, which):
    """one row each of a perturbed telescope (stages ops and sensor: the loops over surfaces in their frames) and of the optical
    phase screen (stage psf, the component's LDS set up per row beside the window): the stamp equals the binned pool of the same
    scene"""
    if which == "doOpt":
        sc, stage = PP.doopt_scene(), "psf"
        rows = psf_map.point_rows(sc, np.array([[10.0, 20.0]]), 5000, stage, wavelength=620.0)
        rows["atm_tan_x"], rows["atm_tan_y"] = np.radians(1.0), 0.0
        rows["x0"], rows["y0"] = 0.0, 0.0
        r = psf_map.renderer_for(sc)
    else:
        sc, stage = PP.perturbed_scene(), ("ops" if which == "perturbed" else "sensor")
        rows = psf_map.point_rows(sc, np.array([[30.0, 20.0]]), 5000, "ops")
        if stage == "sensor":
            sc.sensor = configs.scene_c3(nx=64, ny=64, sensor=True).sensor
        r = psf_image.renderer_for(sc, stage)
        assert (r.scene.sensor is not None) == (stage == "sensor") and (r.scene.nx, r.scene.ny) == (1, 1)
    dx, dy, flux, offs = pool_offsets(r, rows, stage)
    res = run_image(r, rows, stage, (90, 70), scale_from_pool(dx, dy, flux, 90, 70))
    assert_equals_pool(res, dx, dy, flux, offs, which)
    in_window, beside_window = window_split(res.counts)
    assert in_window > 2500 and beside_window > 0 and res.n_outside[0] > 0


def test_gaussian_closed_form(torch_cuda):
    """A pure Gaussian of sigma s in stage psf, 1e6 photons, 12 x 12 cells of side s / 2 (out to 3 s; the rarest cell expects 23
    photons): the chi-square of the 144 cells and the `outside` count against the multinomial law, whose cell probabilities are
    products of erf differences, lies within 5 sqrt(2 dof) of its dof = 144 -- test_psf_profile_gpu.test_gaussian_closed_form's
    acceptance level and seed."""
    n, sigma = 1_000_000, 0.7 / 2.3548200450309493
    psf = [(_abi.IMS_PSF_GAUSSIAN, 0, sigma, 0.0, 1.0)]
    res = psf_image.images(psf, np.zeros((1, 2)), n, 12, 0.5 * sigma, stage="psf", wavelength=620.0, seed=PP.GAUSS_SEED)
    assert res.n_used[0] + res.n_outside[0] == n and res.n_dropped[0] == 0
    edges = (np.arange(13) - 6.0) * 0.5                                       # in units of sigma
    cdf = np.array([0.5 * (1.0 + math.erf(e / math.sqrt(2.0))) for e in edges])
    p1 = np.diff(cdf)
    p = np.outer(p1, p1)
    p_out = 1.0 - p.sum()
    assert n * p.min() > 20.0
    chi = (((res.counts[0] - n * p) ** 2) / (n * p)).sum() + (res.n_outside[0] - n * p_out) ** 2 / (n * p_out)
    dof = p.size
    print(f"chi2 {chi:.2f} (dof {dof}), outside {res.n_outside[0]} (expected {n * p_out:.1f})")
    assert abs(chi - dof) <= 5.0 * math.sqrt(2.0 * dof)
    m = psf_image.moments(res)[0]
    assert abs(m["xbar"]) < 0.01 * sigma and abs(m["ybar"]) < 0.01 * sigma and abs(m["e1"]) < 0.01 and abs(m["e2"]) < 0.01


def test_sensor_stage_widens_the_stamp_by_the_conversion_step(sensor_renderer):
    """Eight rows of 25 000 photons, stamps of 64 x 64 cells of 1/4 pixel in stages ops and sensor, added up over the rows:
    M = (Ixx + Iyy)(sensor) - (Ixx + Iyy)(ops) of psf_image.moments is positive, and equals what the pools say the conversion does.

    Reference.  Photon p has the offset r_p in the unconverted pool and r_p + d_p in the converted one; d_p is its diffusion
    step plus the lateral walk of its inclined ray.  Over the set A of photons that lie inside the stamp in both stages, the
    central second moments of the photons themselves differ by exactly
        P = mean |d - mean d|^2 + 2 mean (r - mean r) . (d - mean d),
    the mean squared conversion step and its covariance with where the photon was (not zero: FocusDepth has moved the photon
    along the very direction cosines the walk follows).  Both terms are formed from the two pools.

    Margin: the statistical error of M - P at this photon count N = |A|.  (1) n_x photons are inside the stamp in one stage only
    (they cross its edge, or the sensor loses them).  Each changes Ixx + Iyy of its stage by at most R^2 / N, R the stamp's half
    diagonal, inwards and outwards crossings with opposite signs: standard error sqrt(n_x) R^2 / N.  (2) The stamp puts a
    photon at its cell's centre: an error e_p uniform over the cell, variance s^2 / 12 per axis.  Its s^2 / 6 in Ixx + Iyy is the
    same in both stages and cancels; what is left per stage is 2 mean (r . e), of standard error sqrt(2 T s^2 / 6 / N) for a
    stamp of T = Ixx + Iyy.  Five standard errors: margin = 5 sqrt(n_x R^4 / N^2 + 2 * 2 T_sensor s^2 / (6 N)).

    Measured on the MI355X: M = 0.3281 pixel^2 (sigma 2.377 -> 2.412 pixels); mean squared step 0.3715, covariance term
    -0.0226, P = 0.3489; N = 189 986, n_x = 732, margin 0.0915."""
    sc, r = sensor_renderer
    rows = PM.stage2_rows(sc, 8, n_phot=np.full(8, 25_000), first=1000 * np.arange(8))
    nx = ny = 64
    s = 0.25
    ops = psf_image.images(sc, rows, None, nx, s, stage="ops", renderer=r)
    sen = psf_image.images(sc, rows, None, nx, s, stage="sensor", renderer=r)

    def total(res):
        c = res.counts.sum(axis=0)[None]
        return psf_image.moments(psf_image.Stamps(c, c.sum(axis=(1, 2)), res.n_outside[:1], res.n_dropped[:1], s, 1.0 / s, res.stage))[0]
    mo, ms = total(ops), total(sen)
    M = float(ms["Ixx"] + ms["Iyy"] - mo["Ixx"] - mo["Iyy"])
    ux, uy, uf, _ = pool_offsets(r, rows, "ops")
    cx, cy, cf, _ = pool_offsets(r, rows, "sensor")
    in_o = cells_reference(ux, uy, 1.0 / s, nx, ny)[2] & (uf != 0)
    in_s = cells_reference(cx, cy, 1.0 / s, nx, ny)[2] & (cf != 0)
    assert in_o.sum() == ops.n_used.sum() and in_s.sum() == sen.n_used.sum()
    A = in_o & in_s
    N, n_x = int(A.sum()), int((in_o ^ in_s).sum())
    rx, ry, dx, dy = ux[A], uy[A], (cx - ux)[A], (cy - uy)[A]
    rx, ry, dx, dy = rx - rx.mean(), ry - ry.mean(), dx - dx.mean(), dy - dy.mean()
    step2, cov2 = float((dx * dx + dy * dy).mean()), float(2.0 * (rx * dx + ry * dy).mean())
    P = step2 + cov2
    R2 = 0.25 * (nx * nx + ny * ny) * s * s
    T = float(ms["Ixx"] + ms["Iyy"])
    margin = 5.0 * math.sqrt(n_x * R2 * R2 / (N * N) + 2.0 * 2.0 * T * s * s / (6.0 * N))
    print(f"M {M:.5f} px^2; pools: mean squared step {step2:.5f}, 2 cov {cov2:+.5f}, P {P:.5f}; N {N}, crossing {n_x}, margin {margin:.5f}; "
          f"sigma ops {mo['sigma']:.4f} sensor {ms['sigma']:.4f} px")
    assert N > 150_000 and step2 > 0.01
    assert M > 0.0 and ms["sigma"] > mo["sigma"]
    assert abs(M - P) <= margin and margin < 0.5 * step2


def test_config_end_to_end(torch_cuda, tmp_path, monkeypatch):
    """Two CCDs with output.psf_image (nx 2, 20 000 photons, stage sensor, 40 x 24 cells): one file with an image HDU and a
    SUMMARY table per CCD; the cubes are what images() returns for the same scenes, points and seed; the e-images are those of
    the same config without the key."""
    seen = []
    real = psf_image.images

    def spy(scene, points, n_photons, size, scale, **kw):
        seen.append((scene, np.array(points), n_photons, size, scale, kw))
        return real(scene, points, n_photons, size, scale, **kw)
    monkeypatch.setattr(psf_image, "images", spy)
    o = {"input.instance_catalog.file_name": os.path.join(HERE, "golden", "example_instcat_subset.txt"),
         "image.nobjects": 3, "stamp.draw_method": "phot", "output.dir": str(tmp_path), "image.xsize": 64, "image.ysize": 64,
         "output.nfiles": 2, "image.sky_level": 800.0, "image.noise": {"type": "CCD"}}
    key ={"file_name": "psf_image.fits", "nx": 2, "n_photons": 20000, "stage": "sensor", "size": [40, 24], "scale": 0.5, "centre": "centroid"}
    tmpl = os.path.join(HERE, "data", "test-config-instcat.yaml")
    plain = config.Process(tmpl, template_dirs=[os.path.join(HERE, "data")], overrides=dict(o))
    res = config.Process(tmpl, template_dirs=[os.path.join(HERE, "data")], overrides=dict(o, **{"output.psf_image": key}))
    fn = str(tmp_path / "psf_image.fits")
    assert fn in res.files and fn not in plain.files and not any("psf_image" in s for s in res.ignored)
    assert len(res.images) == len(plain.images) == 2
    for a, b in zip(res.images, plain.images):
        assert np.array_equal(a, b) and a.sum() > 0
    hdus = fits_io.read_fits(fn)
    assert len(hdus) == 4 and len(seen) == 2
    for k in range(2):
        (h, cube), (h2, summ) = hdus[2 * k], hdus[2 * k + 1]
        scene, pts, n_photons, size, scale, kw = seen[k]
        assert (scene.nx, scene.ny) == (64, 64) and scene.sensor is not None and pts.tolist() == psf_map.grid_points(64, 64, 2).tolist()
        assert (n_photons, tuple(size), scale, kw["stage"], kw["centre"]) == (20000, (40, 24), 0.5, "sensor", "centroid")
        again = real(scene, pts, 20000, size, scale, **kw)
        assert cube.dtype == np.float64 and cube.shape == (4, 24, 40) and np.array_equal(cube, again.counts.astype(np.float64))
        assert (h["STAGE"], h["UNITS"], h["SCALE"], h["NPHOT"], h["NX"], h["NY"], h["DET_NAME"], h["CENTRE"], h["N_GRID"]) == \
            ("sensor", "pixel", 0.5, 20000, 40, 24, res.det_names[k], "centroid", 2)
        assert (h["X_FIRST"], h["X_STEP"], h["Y_FIRST"], h["Y_STEP"]) == (16.5, 32.0, 16.5, 32.0) and h["WAVELEN"] > 300.0
        assert (h2["XTENSION"], h2["EXTNAME"], h2["DET_NAME"]) == ("BINTABLE", "SUMMARY", res.det_names[k])
        assert list(summ) == list(psf_image.SUMMARY) and summ["n_used"].dtype == np.int64 and summ["x"].dtype == np.float64
        assert summ["x"].tolist() == pts[:, 0].tolist() and summ["y"].tolist() == pts[:, 1].tolist()
        for name in ("n_used", "n_outside", "n_dropped"):
            assert np.array_equal(summ[name], getattr(again, name)), name
        assert np.all(summ["n_used"] + summ["n_outside"] + summ["n_dropped"] == 20000) and np.all(summ["n_used"] > 15000)
    assert res.det_names[0] != res.det_names[1] and not np.array_equal(hdus[0][1], hdus[2][1])
