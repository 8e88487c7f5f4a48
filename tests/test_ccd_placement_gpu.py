"""Off-axis CCDs on the GPU: the batched field-point trace (ims_trace_field_points) against the numpy tracer, the WCS pair built
from it, image.wcs type Batoid through config.Process, and the oracle's parity away from the axis."""
import math
import os
import warnings

import numpy as np
import pytest

from imsim_amd import _abi, camera, catalog, config, configs, diffraction, instcat, optics, wcs as wcsmod
from helpers import assert_bits_equal

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ARCMIN = math.pi / 10800.0
ARCSEC = math.pi / 648000.0
NX, NY = 4096, 4004
INSTCAT = os.path.join(HERE, "golden", "example_instcat_subset.txt")
# Kernel against numpy trace, position: what tests/test_perturbed_gpu.py accepts for the perturbed photon kernel against
# optics.trace_numpy (1e-6 px = 1e-11 m on the detector; tests/test_opd_gpu.py's kernel-against-numpy bound is on path lengths
# in nm, not on positions).  Both traces here resolve every intersection to f64.
TOL_PX = 1e-6


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def nominal():
    return optics.rubin_like_telescope("r")


def _everything(tel):
    """tests/test_perturbed_gpu.py's perturbation: every kind at realistic size"""
    rng = np.random.default_rng(5)
    coef = [0.0] * 4 + list(0.3e-6 * rng.standard_normal(19))            # Noll 4 .. 22 on M1, um scale
    return optics.apply_perturbations(tel, [
        {"M2": {"shift": [100e-6, 0.0, 0.0], "rotX": ARCMIN}},
        {"LSSTCamera": {"rotY": 0.5 * ARCMIN, "shift": [20e-6, -30e-6, 15e-6]}},
        {"M1": {"Zernike": {"coef": coef}}},
        {"L1": {"shift": [40e-6, 25e-6, 0.0]}}])


def _focal_plane_grid(n=9):
    """field angles over the whole focal plane: along both axes out to 1.07 times the outer edge of the outermost science rafts
    (2.5 raft pitches, 1.9 degrees), so the corners of the square are past the edge of the field"""
    lim = (2.5 * camera.RAFT_PITCH_MM) * 100 * 0.2 * ARCSEC * 1.07
    g = np.linspace(-lim, lim, n)
    thx, thy = np.meshgrid(g, g)
    return thx.ravel(), thy.ravel()


def _numpy_points(tel, thx, thy, fp, rot):
    """optics.field_to_pixel and the number of rays it averaged, point by point"""
    xy = np.full((len(thx), 2), np.nan)
    ngood = np.zeros(len(thx), dtype=np.int32)
    for k, (a, b) in enumerate(zip(thx, thy)):
        pos, vel = optics.pupil_rays(tel, a, b, wave_nm=620.0)
        if tel.perturbed:
            _, _, vig, fail = optics.trace_numpy(optics.with_camera_rotation(tel, rot), pos, vel, 620.0, local_last=True)
        else:
            _, _, vig, fail = optics.trace_numpy(tel, pos, vel, 620.0)
        ngood[k] = int((~(vig | fail)).sum())
        if ngood[k]:
            xy[k] = optics.field_to_pixel(tel, a, b, fp, rot, 620.0)
    return xy, ngood


@pytest.mark.parametrize("which", ["nominal", "perturbed"])
def test_kernel_matches_numpy_field_to_pixel(torch_cuda, nominal, which):
    """Largest differences seen are recorded in DESIGN.md 7."""
    tel = nominal if which == "nominal" else _everything(nominal)
    assert tel.perturbed == (which == "perturbed")
    fp = camera.fp_to_pix("R22_S11", NX, NY)
    rot = 0.6988
    thx, thy = _focal_plane_grid()
    xy, ngood = optics.field_to_pixel_hip(tel, thx, thy, fp, rot, 620.0, "cuda:0")
    ref_xy, ref_ngood = _numpy_points(tel, thx, thy, fp, rot)
    print(which, "good rays per point (of 144):", np.unique(ngood, return_counts=True))
    assert np.array_equal(ngood, ref_ngood), np.flatnonzero(ngood != ref_ngood)
    seen = ngood > 0
    assert seen.sum() >= 45 and (ngood == 144).sum() >= 9 and (~seen).sum() >= 4       # the field, its vignetted rim, and beyond
    assert np.all(np.isnan(xy[~seen]))
    d = np.abs(xy[seen] - ref_xy[seen])
    print(which, "largest |kernel - numpy| [px]:", d.max(), "over", int(seen.sum()), "points out to",
          np.hypot(thx[seen], thy[seen]).max() / ARCMIN / 60, "deg; pixel positions up to", np.abs(xy[seen]).max())
    assert d.max() <= TOL_PX
    # the grid does cover the focal plane: traced points beyond the far corners of the extreme science CCDs
    assert np.abs(xy[seen]).max() > 100 * 2.5 * camera.RAFT_PITCH_MM


def test_two_launches_give_the_same_bits(torch_cuda, nominal):
    thx, thy = _focal_plane_grid(11)
    for tel in (nominal, _everything(nominal)):
        tr = optics.FieldTracer(tel, camera.fp_to_pix("R12_S20", NX, NY), 0.3, 620.0, "cuda:0")
        a, na = tr(thx, thy)
        b, nb = tr(thx, thy)
        assert a.tobytes() == b.tobytes() and na.tobytes() == nb.tobytes()
        # a field's result does not depend on which other fields share the launch
        sub = np.arange(len(thx))[::7][::-1]
        c, nc = tr(thx[sub], thy[sub])
        assert c.tobytes() == a[sub].tobytes() and nc.tobytes() == na[sub].tobytes()


def test_two_neighbours_agree(torch_cuda, nominal):
    """One field angle through the descriptors of R22_S11 and its neighbours: the same spot, one CCD pitch (4225 px) apart
    along one axis and equal along the other.  In the layout table shared with vignetting.detector_center_mm the first digit
    of Sxy counts along focal-plane x, so the neighbour in x is R22_S21 and R22_S12 is the neighbour in y; both are checked."""
    pupil = optics.pupil_rays(nominal, 0.0, 0.0)[0][:, :2]
    thx, thy = np.array([0.001, -0.0042]), np.array([0.0007, 0.0031])
    out = {}
    for det in ("R22_S11", "R22_S21", "R22_S12"):
        o = optics.make_optics(nominal, camera.fp_to_pix(det, NX, NY), 0.0)
        out[det], ngood = optics.field_to_pixel_hip(o, thx, thy, pupil=pupil)
        assert np.all(ngood == 144)
    d = out["R22_S11"] - out["R22_S21"]
    print("R22_S11 - R22_S21:", d)
    assert np.abs(d[:, 0] - 4225.0).max() <= TOL_PX and np.abs(d[:, 1]).max() <= TOL_PX
    d = out["R22_S11"] - out["R22_S12"]
    print("R22_S11 - R22_S12:", d)
    assert np.abs(d[:, 1] - 4225.0).max() <= TOL_PX and np.abs(d[:, 0]).max() <= TOL_PX


def _hexapolar(th):
    pts = [(th[0], th[1])]
    for k in range(1, 7):
        for j in range(6 * k):
            r, a = math.radians(0.16) * k / 6.0, 2 * math.pi * j / (6 * k)
            pts.append((th[0] + r * math.cos(a), th[1] + r * math.sin(a)))
    return np.array(pts)


def _angle(u, v):
    return 2.0 * np.arcsin(0.5 * np.linalg.norm(u - v, axis=-1))


@pytest.mark.parametrize("det", ["R22_S11", "R01_S00", "R43_S22"])
def test_gpu_wcs_pair_against_the_numpy_build(torch_cuda, nominal, det):
    """Corners and centre of the CCD through both WCSs: they agree within twice the numpy fit's own rms residual over its 127 fit
    points.  Measured figures are in EXPERIMENTS.md."""
    nx, ny = camera_size(det)
    fp = camera.fp_to_pix(det, nx, ny)
    args = dict(rot_sky=2.29, rot_tel_pos=0.6988, nx=nx, ny=ny)
    w_np, f_np, th_np = optics.build_wcs_pair(nominal, fp, 1.0557, -0.6661, **args)
    w_gpu, f_gpu, th_gpu = optics.build_wcs_pair(nominal, fp, 1.0557, -0.6661, device="cuda:0", what=det, **args)
    assert bytes(f_np) == bytes(f_gpu)
    # the numpy fit's residual: its own fit points through its own WCS against the sky they were fitted to
    pts = _hexapolar(th_np)
    pix = np.array([optics.field_to_pixel(nominal, a, b, fp, 0.6988) for a, b in pts])
    resid = _angle(wcsmod.tansip_pix_to_vec(w_np, pix[:, 0], pix[:, 1]), wcsmod.tansip_pix_to_vec(f_np, pts[:, 0], pts[:, 1]))
    rms = float(np.sqrt(np.mean(resid ** 2)))
    x = np.array([1.0, nx, 1.0, nx, (nx + 1) / 2.0])
    y = np.array([1.0, 1.0, ny, ny, (ny + 1) / 2.0])
    diff = _angle(wcsmod.tansip_pix_to_vec(w_np, x, y), wcsmod.tansip_pix_to_vec(w_gpu, x, y))
    print(det, "numpy fit residual rms / max [arcsec]:", rms / ARCSEC, resid.max() / ARCSEC, " GPU - numpy at corners and centre "
          "[arcsec]:", diff / ARCSEC, " centre field angle difference [rad]:", th_gpu - th_np)
    assert rms > 0.0 and diff.max() <= 2.0 * rms


def camera_size(det):
    from imsim_amd.lsst_image import DETECTOR_SIZE
    return DETECTOR_SIZE[camera.det_type_of(det)]


def test_unreachable_field_point_is_an_error_naming_the_ccd(torch_cuda, nominal):
    # an affine that puts the CCD 6 degrees off the axis: nothing gets there
    fp = (100.0, 0.0, 2048.0 + 100 * 1080.0, 0.0, 100.0, 2002.0)
    with pytest.raises(ValueError, match="R99_S99.*no ray"):
        optics.build_wcs_pair(nominal, fp, 0.0, 0.0, nx=NX, ny=NY, device="cuda:0", what="CCD R99_S99")


BATOID = {"type": "Batoid", "camera": "LsstCamSim", "det_name": "$det_name", "obstime": "2023-07-18T10:07:03",
          "boresight": {"type": "RADec", "ra": {"type": "Degrees", "theta": {"type": "OpsimData", "field": "fieldRA"}},
                        "dec": {"type": "Degrees", "theta": {"type": "OpsimData", "field": "fieldDec"}}}}


def _process(tmp_path, **over):
    o = {"input.instance_catalog.file_name": INSTCAT, "stamp.draw_method": "phot", "output.dir": str(tmp_path)}
    o.update(over)
    return config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")],
                          overrides=o)


def test_centre_ccd_is_the_default_path_bit_for_bit(torch_cuda, tmp_path):
    """Both runs render R22_S11 with the same affine; one fits its WCS through host-traced points, the other through GPU-traced
    ones, and the two WCSs differ by about 1e-7 arcsec (1e-6 px).  The images are the same bits as long as no photon of these 12
    objects lands within that distance of a pixel edge -- true for this catalog and seed, but a property of them: if a change
    of catalog, seed or summation order ever makes this differ in a handful of pixels by one count, look there first."""
    a = _process(tmp_path / "a", **{"image.nobjects": 12})
    b = _process(tmp_path / "b", **{"image.nobjects": 12, "image.wcs": BATOID})
    assert a.det_names == b.det_names == ["R22_S11"]
    assert a.images[0].sum() > 0
    assert_bits_equal(a.images[0], b.images[0], "R22_S11 with and without image.wcs")
    assert not any(s.startswith("image.wcs") for s in a.ignored)
    assert [s for s in b.ignored if s.startswith("image.wcs")] == [config.WCS_IGNORED["obstime"]]


def _centroids(img, xs, ys, half=12):
    out = []
    for x, y in zip(xs, ys):
        i0, j0 = int(round(x)) - 1, int(round(y)) - 1          # pixel (1, 1) is array [0, 0]
        w = img[j0 - half:j0 + half + 1, i0 - half:i0 + half + 1].astype(np.float64)
        jj, ii = np.mgrid[-half:half + 1, -half:half + 1]
        s = w.sum()
        out.append((i0 + 1 + (w * ii).sum() / s, j0 + 1 + (w * jj).sum() / s, s))
    return np.array(out)


@pytest.mark.parametrize("det_num, det", [(0, "R01_S00"), (188, "R43_S22")])
def test_process_renders_an_off_axis_ccd_in_place(torch_cuda, nominal, tmp_path, det_num, det):
    """Stars put, through the host-built WCS of the CCD, on chosen pixels: the truth catalog lists them and their photons land
    there.  On a commit that does not read image.wcs the CCD looks at the centre of the field and culls them all."""
    assert config.det_name_of(det_num) == det
    nx, ny = camera_size(det)
    meta = instcat.read_header(INSTCAT)
    rot_tel = math.radians(meta["rotTelPos"])
    w_np, _, _ = optics.build_wcs_pair(nominal, camera.fp_to_pix(det, nx, ny), math.radians(meta["fieldRA"]),
                                       math.radians(meta["fieldDec"]), rot_sky=math.radians(meta["rotSkyPos"]), rot_tel_pos=rot_tel,
                                       nx=nx, ny=ny)
    want = np.array([(400.0, 500.0), (3600.3, 420.7), (2036.5, 2000.5), (612.25, 3550.5), (3500.8, 3600.1), (1500.0, 1200.4)])
    vec = wcsmod.tansip_pix_to_vec(w_np, want[:, 0], want[:, 1])
    ra, dec = np.degrees(np.arctan2(vec[:, 1], vec[:, 0])) % 360.0, np.degrees(np.arcsin(vec[:, 2]))
    ids = [900001 + k for k in range(len(want))]
    cat_file = tmp_path / "stars.txt"
    with open(INSTCAT) as f:
        header = [ln for ln in f if not ln.startswith("object")]
    with open(cat_file, "w") as f:
        f.writelines(header)
        for i, a, d in zip(ids, ra, dec):                       # magnorm 17.5: about 8.6e5 photons shot
            f.write(f"object {i} {float(a)!r} {float(d)!r} 17.5 starSED/kurucz/km10_5250.fits_g15_5250.gz 0 0 0 0 0 0 point none CCM 0.01 3.1\n")
    over = {"input.instance_catalog.file_name": str(cat_file), "image.nobjects": len(want), "output.det_num.first": det_num}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                          # no tree-ring data for this CCD in the test file
        res = _process(tmp_path / "out", **{**over, "image.wcs": BATOID})
    assert res.det_names == [det] and res.images[0].shape == (ny, nx)
    truth = res.truth[0]
    listed = [str(v) for v in truth["object_id"]]
    order = [listed.index(str(i)) if str(i) in listed else -1 for i in ids]
    assert min(order) >= 0, ("stars missing from the truth catalog", truth["object_id"])
    tx, ty, flux = truth["x"][order], truth["y"][order], truth["realized_flux"][order]
    print(det, "truth - chosen [px]:", tx - want[:, 0], ty - want[:, 1])
    # 1e5 photons at the very least, after the vignetting of the field's edge as well
    assert np.all(truth["phot_flux"][order] >= 1e5) and np.all(flux >= 1e5), (truth["phot_flux"][order], flux)
    # the GPU-built WCS puts the catalog where the host-built one does (a tenth of a pixel is already a failed fit)
    assert np.abs(tx - want[:, 0]).max() < 0.1 and np.abs(ty - want[:, 1]).max() < 0.1
    c = _centroids(res.images[0], want[:, 0], want[:, 1])
    print(det, "centroid - chosen [px]:", c[:, 0] - want[:, 0], c[:, 1] - want[:, 1], "counts", c[:, 2])
    assert np.all(c[:, 2] > 0.5 * flux)
    assert np.all(np.hypot(c[:, 0] - want[:, 0], c[:, 1] - want[:, 1]) < 1.0)


def test_oracle_parity_off_axis(torch_cuda, nominal):
    """the C3 scene of the parity tests with the descriptor of an off-axis CCD: HIP and oracle images are the same bits"""
    from imsim_amd.engine import Renderer
    from oracle import orc_loader
    n = 256
    scene = configs.scene_c3(nx=n, ny=n)
    scene.sensor.scratch_cells = 400_000
    v = configs.VISIT
    rot_tel = math.radians(v["rottelpos"])
    fp = camera.fp_to_pix("R01_S00", n, n)
    o = _abi.Optics()
    optics.fill_optics(o, nominal, fp, rot_tel)
    o.img_wcs, o.icrf_to_field, th = optics.build_wcs_pair(nominal, fp, math.radians(v["ra"]), math.radians(v["dec"]),
                                                           rot_sky=math.radians(v["rotskypos"]), rot_tel_pos=rot_tel, nx=n, ny=n,
                                                           device="cuda:0", what="R01_S00")
    diffraction.fill_optics(o, math.radians(v["latitude"]), math.radians(v["azimuth"]), math.radians(v["altitude"]))
    assert np.hypot(*th) > 0.03 and tuple(o.fp_to_pix) == fp and tuple(scene.optics.fp_to_pix) != fp
    scene.optics = o
    cat = catalog.synthetic_catalog(60, nx=n, ny=n)
    phot = catalog.realize_fluxes(cat["nominal_flux"], 7)
    objects, _ = configs.c3_objects(cat, phot, scene)
    r = Renderer(scene, "cuda:0")
    r.render_lsst_image(objects, nrecalc=1000)
    r.synchronize()
    gpu = r.image_numpy()
    orc = orc_loader.OracleScene(scene)
    orc.render_lsst_image(objects, nrecalc=1000)
    # off the axis part of the pupil is vignetted: the image holds fewer photons than were shot, but most of them
    assert 0.2 * objects["n_phot"].sum() < gpu.sum() < objects["n_phot"].sum()
    assert_bits_equal(gpu, orc.image, "off-axis C3 image")
