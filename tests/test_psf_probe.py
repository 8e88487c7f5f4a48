"""The host half the four PSF probes share (psf_map.compute, psf_map.adaptive, psf_profile.profile, psf_image.images), pinned
without a GPU: the exact text of every refusal that comes before the first launch, what an empty table of points returns, the
exact text of the config errors of the three `output.*` keys, and the bytes of the two counts-cube files.

Written against the four copies this logic had before imsim_amd/psf_probe.py: every test here passed on them as it stands, the
file hashes are theirs, with one exception.  test_profile_checks_its_centre_string_as_images_does states the one behaviour the
shared path changed on purpose: psf_profile.profile used to check a centre string only once it had a renderer, so not at all for
an empty table; it now checks it where psf_image.images always did."""
import hashlib

import numpy as np
import pytest

from imsim_amd import _abi, config, configs, psf_image, psf_map, psf_profile
from imsim_amd.lsst_image import GalSimConfigError

PTS = np.array([[10.0, 20.0], [50.5, 40.25]])
NONE = np.zeros((0, 2))
NO_GPU = dict(device="no such device")                   # every call below has to return or raise before a renderer is made
# probe -> (the name in its messages, a call (scene, points, n_photons, **kw) with the probe's own arguments filled in)
PROBES = {
    "compute": ("psf_map", lambda sc, pts, n, **kw: psf_map.compute(sc, pts, n, **NO_GPU, **kw)),
    "adaptive": ("psf_map", lambda sc, pts, n, **kw: psf_map.adaptive(sc, pts, n, **NO_GPU, **kw)),
    "profile": ("psf_profile", lambda sc, pts, n, **kw: psf_profile.profile(sc, pts, n, [0.0, 1.0, 2.0], n_phi=3, **NO_GPU, **kw)),
    "images": ("psf_image", lambda sc, pts, n, **kw: psf_image.images(sc, pts, n, (5, 3), 0.5, **NO_GPU, **kw)),
}
CENTRE_TEXT = "{}: centre must be 'nominal', 'centroid' or an [n][2] array, not 'bogus'"


@pytest.fixture(scope="module")
def scene():
    return configs.scene_c3(nx=64, ny=64, sensor=False)


@pytest.fixture(scope="module")
def ratio_scene():
    sc = configs.scene_c3(nx=64, ny=64, sensor=False)
    sc.ops = list(sc.ops) + [(_abi.IMS_OP_BANDPASS_RATIO, 0, [])]
    return sc


def raises_exactly(exc, text, fn, *args, **kw):
    with pytest.raises(exc) as e:
        fn(*args, **kw)
    assert str(e.value) == text


@pytest.mark.parametrize("probe", PROBES)
def test_refusals_common_to_the_four_probes(scene, probe):
    name, call = PROBES[probe]
    stages = "['ops', 'psf', 'sensor']" if probe == "images" else "['ops', 'psf']"
    raises_exactly(ValueError, f"{name}: stage must be one of {stages}, not 'pixel'", call, scene, PTS, 10, stage="pixel")
    raises_exactly(ValueError, f"{name}: n_photons is required with pixel positions", call, scene, PTS, None)
    raises_exactly(ValueError, f"{name}: n_photons is required with pixel positions", call, scene, NONE, None)
    # (the rows are psf_map.point_rows' for every probe, and the message is its own)
    raises_exactly(ValueError, "psf_map: negative photon count", call, scene, PTS, -1)
    raises_exactly(ValueError, "psf_map: negative photon count", call, scene, PTS, [5, -5], stage="ops")


@pytest.mark.parametrize("probe", PROBES)
def test_ready_rows_need_no_n_photons(scene, probe):
    """OBJECT_DTYPE rows carry their own counts: n_photons None is no error for them (an empty table, so that nothing is launched)"""
    name, call = PROBES[probe]
    rows = psf_map.point_rows(scene, PTS, [3, 4], "ops")[:0]
    for n in (None, 7):
        out = call(scene, rows, n)
        assert len(out if name == "psf_map" else out.counts) == 0


def test_centre_string_is_checked_before_any_gpu_work(scene):
    for pts in (PTS, NONE):
        raises_exactly(ValueError, CENTRE_TEXT.format("psf_image"), PROBES["images"][1], scene, pts, 10, centre="bogus")
        raises_exactly(ValueError, CENTRE_TEXT.format("psf_image"), PROBES["images"][1], scene, pts, 10, centre="bogus", stage="ops")
    for centre in (None, "nominal", "centroid"):
        assert PROBES["images"][1](scene, NONE, 10, centre=centre).centre is None


def test_profile_checks_its_centre_string_as_images_does(scene):
    """for an empty table too, and before a renderer is made"""
    for pts in (PTS, NONE):
        raises_exactly(ValueError, CENTRE_TEXT.format("psf_profile"), PROBES["profile"][1], scene, pts, 10, centre="bogus")
    for centre in (None, "nominal", "centroid"):
        assert PROBES["profile"][1](scene, NONE, 10, centre=centre).centre is None


def test_flux_operators_and_the_missing_sensor_are_refused(scene, ratio_scene):
    text = "{}: the photon-operator chain holds a BandpassRatio operator, whose photons carry unequal flux; the {} counts photons unweighted"
    raises_exactly(ValueError, text.format("psf_profile", "profile"), PROBES["profile"][1], ratio_scene, PTS, 10, stage="ops")
    raises_exactly(ValueError, text.format("psf_profile", "profile"), psf_profile.refuse_flux_operators, ratio_scene, "ops")
    raises_exactly(GalSimConfigError, "output.psf_profile: " + text.format("psf_profile", "profile"), psf_profile.check_scene, ratio_scene, "ops")
    for stage in ("ops", "sensor"):
        raises_exactly(ValueError, text.format("psf_image", "stamp"), PROBES["images"][1], ratio_scene, PTS, 10, stage=stage)
        raises_exactly(ValueError, text.format("psf_image", "stamp"), psf_image.refuse_flux_operators, ratio_scene, stage)
    # stage psf runs no operator: nothing to refuse, and the empty table comes back
    for mod in (psf_profile, psf_image):
        assert mod.refuse_flux_operators(ratio_scene, "psf") is None and mod.refuse_flux_operators(scene, "ops") is None
    assert psf_profile.check_scene(scene, "ops") is None and psf_profile.check_scene(ratio_scene, "psf") is None
    assert PROBES["profile"][1](ratio_scene, NONE, 10, stage="psf").counts.shape == (0, 4, 4)
    assert PROBES["images"][1](ratio_scene, NONE, 10, stage="psf").counts.shape == (0, 3, 5)
    # the moments are weighted sums: psf_map refuses nothing
    assert len(PROBES["compute"][1](ratio_scene, NONE, 10, stage="ops")) == 0
    no_sensor = "psf_image: stage 'sensor' needs a scene with a Silicon sensor (scene.sensor is None)"
    raises_exactly(ValueError, no_sensor, PROBES["images"][1], scene, PTS, 10, stage="sensor")
    raises_exactly(ValueError, no_sensor, psf_image.require_sensor, scene, "sensor")
    assert psf_image.require_sensor(scene, "ops") is None


@pytest.mark.parametrize("stage", ["psf", "ops"])
def test_an_empty_table_of_points_returns_empty_fields(scene, stage):
    m = PROBES["compute"][1](scene, NONE, 10, stage=stage)
    assert m.shape == (0,) and m.dtype == psf_map.MOMENTS_DTYPE
    a = PROBES["adaptive"][1](scene, NONE, 10, stage=stage)
    assert a.shape == (0,) and a.dtype == psf_map.ADAPTIVE_DTYPE
    p = PROBES["profile"][1](scene, NONE, 10, stage=stage, phi0=0.25)
    assert isinstance(p, psf_profile.Profile) and (p.counts.shape, p.counts.dtype) == ((0, 4, 4), np.int64)
    assert (p.n_used.shape, p.n_used.dtype, p.n_dropped.shape, p.n_dropped.dtype) == ((0,), np.int64, (0,), np.int64)
    assert p.r_edges.tolist() == [0.0, 1.0, 2.0] and p.r_edges.dtype == np.float64 and p.r2_edges.tolist() == [0.0, 1.0, 4.0]
    assert p.dirs.shape == (3, 2) and p.dirs.dtype == np.float64 and p.dirs.tobytes() == psf_profile.sector_dirs(3, 0.25).tobytes()
    assert (p.phi0, p.stage, p.centre, p.n_r, p.n_phi) == (0.25, stage, None, 2, 3)
    s = PROBES["images"][1](scene, NONE, 10, stage=stage)
    assert isinstance(s, psf_image.Stamps) and (s.counts.shape, s.counts.dtype) == ((0, 3, 5), np.int64)
    for v in (s.n_used, s.n_outside, s.n_dropped):
        assert (v.shape, v.dtype) == ((0,), np.int64)
    assert (s.scale, s.inv_scale, s.stage, s.centre, s.nx, s.ny) == (0.5, 2.0, stage, None, 5, 3)


# ---------------- parse_config of the three outputs ----------------
OUTPUTS = {
    "psf_map": (psf_map, {"file_name": "p.fits"}, "['ops', 'psf']"),
    "psf_profile": (psf_profile, {"file_name": "p.fits", "r_min": 1, "r_max": 2}, "['ops', 'psf']"),
    "psf_image": (psf_image, {"file_name": "p.fits", "scale": 0.1}, "['ops', 'psf', 'sensor']"),
}


@pytest.mark.parametrize("name", OUTPUTS)
def test_config_errors_of_the_common_head(name):
    mod, good, stages = OUTPUTS[name]
    ev = config.Evaluator({})
    assert mod.parse_config(dict(good), ev)["stage"] == "psf"
    raises_exactly(GalSimConfigError, f"output.{name} must be a dict", mod.parse_config, "p.fits", ev)
    raises_exactly(GalSimConfigError, f"output.{name} must be a dict", mod.parse_config, ["p.fits"], ev)
    raises_exactly(GalSimConfigError, f"Unexpected attribute ny found in output.{name}", mod.parse_config, dict(good, ny=4), ev)
    # an unexpected key is reported before a missing one
    raises_exactly(GalSimConfigError, f"Unexpected attribute ny found in output.{name}", mod.parse_config, {"ny": 4}, ev)
    for k in good:
        cfg = {j: v for j, v in good.items() if j != k}
        raises_exactly(GalSimConfigError, f"Attribute {k} is required in output.{name}", mod.parse_config, cfg, ev)
    raises_exactly(GalSimConfigError, f"output.{name}.nx must be at least 1", mod.parse_config, dict(good, nx=0), ev)
    raises_exactly(GalSimConfigError, f"output.{name}.n_photons must be at least 1", mod.parse_config, dict(good, n_photons=0), ev)
    raises_exactly(GalSimConfigError, f"output.{name}.nx must be at least 1", mod.parse_config, dict(good, nx=0, n_photons=0, stage="pixel"), ev)
    raises_exactly(GalSimConfigError, f"output.{name}.n_photons must be at least 1", mod.parse_config, dict(good, n_photons=0, stage="pixel"), ev)
    raises_exactly(GalSimConfigError, f"output.{name}.stage must be one of {stages}, not pixel", mod.parse_config, dict(good, stage="pixel"), ev)
    if name == "psf_map":                                # the moments have no centre to choose
        raises_exactly(GalSimConfigError, "Unexpected attribute centre found in output.psf_map", mod.parse_config, dict(good, centre="peak"), ev)
    else:
        raises_exactly(GalSimConfigError, f"output.{name}.centre must be nominal or centroid, not peak", mod.parse_config, dict(good, centre="peak"), ev)
        raises_exactly(GalSimConfigError, f"output.{name}.stage must be one of {stages}, not pixel", mod.parse_config,
                       dict(good, stage="pixel", centre="peak"), ev)
        assert mod.parse_config(dict(good, centre="centroid"), ev)["centre"] == "centroid"


def test_defaults_of_the_common_head():
    ev = config.Evaluator({})
    assert psf_map.parse_config({"file_name": "p.fits"}, ev) == dict(nx=8, n_photons=100000, stage="psf")
    kw = psf_profile.parse_config({"file_name": "p.fits", "r_min": 1, "r_max": 2}, ev)
    assert (kw["nx"], kw["n_photons"], kw["stage"], kw["centre"]) == (4, 1000000, "psf", "nominal")
    kw = psf_image.parse_config({"file_name": "p.fits", "scale": 0.1, "nx": "3", "n_photons": 7.0, "stage": "sensor"}, ev)
    assert (kw["nx"], kw["n_photons"], kw["stage"], kw["centre"]) == (3, 7, "sensor", "nominal")


# ---------------- the files ----------------
def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def test_profile_file_bytes(tmp_path):
    """two CCDs into one file; the hash is that of the file psf_profile.write wrote before the writers were shared"""
    counts = np.arange(2 * 4 * 4, dtype=np.int64).reshape(2, 4, 4)
    r = np.array([1.0, 2.0, 4.0])
    res = psf_profile.Profile(counts=counts, n_used=counts.sum(axis=(1, 2)), n_dropped=np.array([5, 2 ** 40]), r_edges=r, r2_edges=r * r,
                              dirs=psf_profile.sector_dirs(3, 0.5), phi0=0.5, stage="ops")
    items = [(res.counts.astype(np.float64), psf_profile.make_header(det, res, 622.2, 19, 4096, 4000, 1, centre, sampled=sampled),
              psf_profile.summary(res), psf_profile.summary_header(det))
             for det, centre, sampled in (("R22_S11", "nominal", True), ("R22_S12", "centroid", False))]
    fn = str(tmp_path / "sub" / "profile.fits")
    psf_profile.write(fn, items)
    assert sha(fn) == "474d2fec474bda5ada386a2bc2dbf891ebca7000363f4e0dbd892e3fc5bb8d7e"


def test_image_file_bytes(tmp_path):
    """two CCDs into one file; the hash is that of the file psf_image.write wrote before the writers were shared"""
    counts = np.arange(4 * 3 * 5, dtype=np.int64).reshape(4, 3, 5)
    res = psf_image.Stamps(counts, counts.sum(axis=(1, 2)), np.array([1, 2, 3, 4]), np.array([5, 6, 7, 2 ** 40]), 0.2, 5.0, "sensor", None)
    pts = np.array([[512.5, 500.5], [1536.5, 500.5], [512.5, 1500.5], [1536.5, 1500.5]])
    items = [(res.counts.astype(np.float64), psf_image.make_header(det, res, 622.2, 19, 2048, 2000, 2, centre, sampled=sampled),
              psf_image.summary(res, pts), psf_image.summary_header(det))
             for det, centre, sampled in (("R22_S11", "nominal", True), ("R22_S12", "centroid", False))]
    fn = str(tmp_path / "sub" / "image.fits")
    psf_image.write(fn, items)
    assert sha(fn) == "91bafc18d13d16a99adab064c1ec2f0a02db63a437fd0e3ccbe2f9ba1be314be"


def test_map_header_keeps_its_cards_and_their_order():
    """psf_map.make_header is the probes' common cards followed by the PLANE cards; the other two headers drop the planes"""
    h = psf_map.make_header("R22_S11", "ops", 700.0, 5, 4096, 4000, 2, adaptive=(1e-6, 100))
    common = ["det_name", "stage", "units", "wavelen", "nphot", "x_first", "x_step", "y_first", "y_step"]
    assert list(h) == common + [f"PLANE{k}" for k in range(1, 25)] + ["TOL", "MAXITER"]
    assert h["units"] == ("pixel", "of the centroids; squared for the moments") and h["wavelen"] == (700.0, "(nm) of every photon")
    assert h["stage"] == ("ops", "psf: arcsec after the PSF; ops: pixels after the operators")
    assert h["x_first"] == (1024.5, "CCD pixel x of the first column") and h["y_step"] == (2000.0, "pixels per row")
    assert psf_map.make_header("R22_S11", "psf", 622.2, 5, 4096, 4000, 2, sampled=True)["wavelen"] == (622.2, "(nm) effective; photons sample the bandpass")
