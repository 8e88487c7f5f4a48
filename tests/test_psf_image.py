"""psf_image without a GPU: the C-ABI's declarations and refusals, the config key, the numpy restatement of the binning rule on
hand-made offsets, the estimators, and the FITS layout."""
import ctypes as C
import os

import numpy as np
import pytest

from imsim_amd import _abi, config, configs, fits_io, psf_image
from imsim_amd.lsst_image import GalSimConfigError
from psf_image_ref import cells_reference, counts_reference

HERE = os.path.dirname(os.path.abspath(__file__))


def _ev():
    return config.Evaluator({})


def _stamps(counts, scale=0.5, stage="psf", outside=None, dropped=None, centre=None):
    counts = np.asarray(counts, dtype=np.int64)
    counts = counts[None] if counts.ndim == 2 else counts
    zeros = np.zeros(len(counts), dtype=np.int64)
    return psf_image.Stamps(counts, counts.sum(axis=(1, 2)), zeros if outside is None else np.asarray(outside),
                            zeros if dropped is None else np.asarray(dropped), scale, 1.0 / scale, stage, centre)


def test_entry_point_is_declared_exported_and_sized():
    lib = _abi.load()
    with open(os.path.join(HERE, "..", "include", "imsim_hip.h")) as f:
        header = f.read()
    assert "#define IMS_ABI_VERSION 22" in header and "ims_psf_image(" in header and "ims_psf_image_t" in header
    assert "ims_psf_image" in _abi.EXPORTS and hasattr(lib, "ims_psf_image") and lib.ims_abi_version() == 22
    assert lib.ims_struct_size(_abi.PSF_IMAGE_STRUCT_INDEX) == C.sizeof(_abi.PsfImage) == 16
    # the struct is the last index: every earlier one is what it was (tests/test_abi.py holds their sizes)
    assert _abi.PSF_IMAGE_STRUCT_INDEX == 30 and lib.ims_struct_size(31) == -1 and lib.ims_struct_size(29) > 0
    assert _abi.PsfImage not in _abi.STRUCTS and _abi.PSF_IMAGE_MAX == 512 and "#define IMS_PSF_IMAGE_MAX 512" in header


def test_argument_errors_are_reported_before_any_launch():
    """every refusal of ims_psf_image returns its code and names its argument; nothing is written"""
    lib = _abi.load()
    spec = _abi.PsfImage(8, 8, 2.0)
    call = lib.ims_psf_image
    assert call(None, 1, C.byref(spec), None, None, None, None, None) == -1 and b"params is NULL" in lib.ims_last_error()
    P = _abi.RenderParams()
    P.seg_size = 256
    assert call(C.byref(P), 1, None, None, None, None, None, None) == -1 and b"spec is NULL" in lib.ims_last_error()
    for stage in (0, 4, -1):
        assert call(C.byref(P), stage, C.byref(spec), None, None, None, None, None) == -1 and b"stage" in lib.ims_last_error()
    assert P.sensor is None
    assert call(C.byref(P), 3, C.byref(spec), None, None, None, None, None) == -1 and b"sensor" in lib.ims_last_error()
    for nx, ny, word in ((0, 8, b"nx"), (513, 8, b"nx"), (-4, 8, b"nx"), (8, 0, b"ny"), (8, 513, b"ny")):
        bad = _abi.PsfImage(nx, ny, 2.0)
        assert call(C.byref(P), 1, C.byref(bad), None, None, None, None, None) == -1 and word + b" must" in lib.ims_last_error()
    for inv in (0.0, -1.0, float("inf"), float("nan")):
        bad = _abi.PsfImage(8, 8, inv)
        assert call(C.byref(P), 1, C.byref(bad), None, None, None, None, None) == -1 and b"inv_scale" in lib.ims_last_error()
    for ok in (_abi.PsfImage(1, 1, 2.0), _abi.PsfImage(512, 512, 1e-3)):
        assert call(C.byref(P), 2, C.byref(ok), None, None, None, None, None) == 0                # no rows: nothing to do
    rows = (C.c_double * 32)()
    pre = (C.c_int64 * 2)(0, 1)
    P.n_objects, P.objects, P.seg_prefix, P.n_segments = 1, C.cast(rows, C.c_void_p), C.cast(pre, C.c_void_p), 1
    out = (C.c_int64 * 64)(*([7] * 64))
    for args in ((None, out, out), (out, None, out), (out, out, None)):
        assert call(C.byref(P), 2, C.byref(spec), None, *args, None) == -1
        assert b"counts / outside / dropped is NULL" in lib.ims_last_error()
    P.n_ops = 1
    P.ops[0].kind = _abi.IMS_OP_BANDPASS_RATIO
    one = (C.c_double * 4)()
    for stage in (2, 3):
        P.sensor = C.cast(one, C.c_void_p) if stage == 3 else None
        assert call(C.byref(P), stage, C.byref(spec), None, out, out, out, None) == -4 and b"BandpassRatio" in lib.ims_last_error()
    P.sensor = None
    P.seg_size = 128
    assert call(C.byref(P), 1, C.byref(spec), None, out, out, out, None) == -1 and b"seg_size" in lib.ims_last_error()
    assert list(out) == [7] * 64                                                                  # nothing was written


def test_parse_output_psf_image():
    kw = psf_image.parse_config({"file_name": "p.fits", "scale": 0.05}, _ev())
    assert kw == dict(nx=4, n_photons=1000000, stage="psf", size=(64, 64), scale=0.05, centre="nominal")
    kw = psf_image.parse_config({"file_name": "p.fits", "dir": "out", "nx": 2, "n_photons": 5000, "stage": "sensor", "size": [96, 33],
                                 "scale": "0.25", "centre": "centroid"}, _ev())
    assert kw == dict(nx=2, n_photons=5000, stage="sensor", size=(96, 33), scale=0.25, centre="centroid")
    for size in (1, 512):
        assert psf_image.parse_config({"file_name": "p.fits", "scale": 1, "size": size, "stage": "ops"}, _ev())["size"] == (size, size)


@pytest.mark.parametrize("cfg,match", [
    ("p.fits", "must be a dict"),
    ({"scale": 0.1}, "file_name is required"),
    ({"file_name": "p.fits"}, "scale is required"),
    ({"file_name": "p.fits", "scale": 0.1, "ny": 4}, "Unexpected attribute ny"),
    ({"file_name": "p.fits", "scale": 0.1, "r_max": 4}, "Unexpected attribute r_max"),
    ({"file_name": "p.fits", "scale": 0.1, "stage": "pixel"}, "stage must be one of"),
    ({"file_name": "p.fits", "scale": 0.1, "size": 0}, "size must be 1 .. 512"),
    ({"file_name": "p.fits", "scale": 0.1, "size": 513}, "size must be 1 .. 512"),
    ({"file_name": "p.fits", "scale": 0.1, "size": [64, 0]}, "size must be 1 .. 512"),
    ({"file_name": "p.fits", "scale": 0.1, "size": [64, 64, 64]}, "size must be an int or"),
    ({"file_name": "p.fits", "scale": 0.0}, "scale must be positive"),
    ({"file_name": "p.fits", "scale": -0.2}, "scale must be positive"),
    ({"file_name": "p.fits", "scale": 0.1, "centre": "peak"}, "centre must be"),
    ({"file_name": "p.fits", "scale": 0.1, "nx": 0}, "nx must be at least 1"),
    ({"file_name": "p.fits", "scale": 0.1, "n_photons": 0}, "n_photons must be at least 1"),
])
def test_parse_output_psf_image_errors(cfg, match):
    with pytest.raises(GalSimConfigError, match=match):
        psf_image.parse_config(cfg, _ev())


def test_refusals_of_the_python_layer_come_before_any_gpu_work():
    """BandpassRatio in stages ops and sensor, a sensor stage without a sensor, bad sizes and scales: ValueError from images(),
    a config error from config.Process; a config error of the key itself comes first"""
    sc = configs.scene_c3(nx=64, ny=64, sensor=False)
    pts = np.array([[10.0, 20.0]])
    with pytest.raises(ValueError, match="sensor"):
        psf_image.images(sc, pts, 100, 8, 0.5, stage="sensor", device="no such device")
    for size, scale, match in ((0, 0.5, "size"), (513, 0.5, "size"), ((8, 8, 8), 0.5, "size"), (8, 0.0, "scale"), (8, float("nan"), "scale")):
        with pytest.raises(ValueError, match=match):
            psf_image.images(sc, pts, 100, size, scale, stage="ops", device="no such device")
    with pytest.raises(ValueError, match="stage"):
        psf_image.images(sc, pts, 100, 8, 0.5, stage="pixel", device="no such device")
    with pytest.raises(ValueError, match="centre"):
        psf_image.images(sc, pts, 100, 8, 0.5, stage="ops", centre="peak", device="no such device")
    sc.ops = list(sc.ops) + [(_abi.IMS_OP_BANDPASS_RATIO, 0, [])]
    for stage in ("ops", "sensor"):
        with pytest.raises(ValueError, match="BandpassRatio"):
            psf_image.images(sc, pts, 100, 8, 0.5, stage=stage, device="no such device")
    psf_image.refuse_flux_operators(sc, "psf")
    o = {"input.instance_catalog.file_name": os.path.join(HERE, "golden", "example_instcat_subset.txt"), "image.nobjects": 3,
         "stamp.draw_method": "phot",
         "stamp.photon_ops": [{"type": "BandpassRatio", "target_bandpass": "@bandpass", "initial_bandpass": "@bandpass"}],
         "output.psf_image": {"file_name": "p.fits", "stage": "sensor", "scale": 0.25}}
    tmpl = os.path.join(HERE, "data", "test-config-instcat.yaml")
    with pytest.raises(GalSimConfigError, match="BandpassRatio"):
        config.Process(tmpl, template_dirs=[os.path.join(HERE, "data")], overrides=o)
    o["output.psf_image"] = {"file_name": "p.fits", "stage": "sensor"}
    with pytest.raises(GalSimConfigError, match="scale is required"):
        config.Process(tmpl, template_dirs=[os.path.join(HERE, "data")], overrides=o)


def test_cells_reference_on_hand_made_offsets():
    """cell edges belong to the upper cell, the stamp's far edge and a NaN to `outside`; even sizes have a corner at the centre,
    odd ones a cell's middle"""
    # 4 cells of side 1/2 along x (inv_scale 2): edges at -1, -1/2, 0, 1/2, 1
    dx = np.array([-1.0, -0.75, -0.5, -0.0, 0.0, 0.49, 0.5, 0.999, 1.0, -1.0000001, np.nan, np.inf, -np.inf, 1e300])
    ix, iy, inside = cells_reference(dx, np.zeros(len(dx)), 2.0, 4, 2)
    assert ix.tolist() == [0, 0, 1, 2, 2, 2, 3, 3, -1, -1, -1, -1, -1, -1]
    assert inside.tolist() == [True] * 8 + [False] * 6 and set(iy[inside]) == {1}                 # dy = 0 is the upper of 2 rows
    # odd size: the centre is the middle of cell 2 of 5; its edges at +-1/4
    ix, _, inside = cells_reference([-0.25, -0.2500001, 0.0, 0.2499999, 0.25, 1.2499, 1.25, -1.25, -1.2500001], np.zeros(9), 2.0, 5, 1)
    assert ix.tolist() == [2, 1, 2, 2, 3, 4, -1, 0, -1] and inside.tolist() == [True] * 6 + [False, True, False]
    # a NaN or a miss along y alone puts the photon outside
    ix, iy, inside = cells_reference([0.0, 0.0, 0.0], [np.nan, 5.0, -0.5], 2.0, 4, 2)
    assert inside.tolist() == [False, False, True] and (ix[2], iy[2]) == (2, 0)
    # 1 x 1: one cell of side `scale` around the centre, lower edges included
    ix, iy, inside = cells_reference([0.0, -0.5, 0.5, 0.49, -0.51, 0.0, 0.0], [0.0, -0.5, 0.0, 0.49, 0.0, 0.5, -0.5], 1.0, 1, 1)
    assert inside.tolist() == [True, True, False, True, False, False, True] and set(ix[inside]) == {0} and set(iy[inside]) == {0}
    # every operation is rounded once: fl(fl(dx s) + nx / 2) with an inexact product and an inexact sum
    d, s = np.float64(0.1), np.float64(1.0 / 0.3)
    assert cells_reference([d], [0.0], s, 7, 1)[0][0] == int(np.floor(np.float64(d * s) + np.float64(3.5)))


def test_counts_reference_counts_every_photon_once():
    rng = np.random.default_rng(5)
    dx, dy = rng.normal(0.0, 1.0, 5000), rng.normal(0.0, 2.0, 5000)
    flux = (rng.random(5000) > 0.1).astype(np.float64)
    dx[7], dy[11] = np.nan, np.nan
    for nx, ny in ((1, 1), (8, 8), (9, 4), (65, 63)):
        counts, outside, dropped = counts_reference(dx, dy, flux, 4.0, nx, ny)
        assert counts.shape == (ny, nx) and counts.dtype == np.int64 and counts.min() >= 0
        assert counts.sum() + outside + dropped == 5000 and dropped == int((flux == 0).sum()) and outside >= 2 - int(flux[7] == 0) - int(flux[11] == 0)
    counts, outside, dropped = counts_reference([0.3, 0.3, -0.3], [0.1, 0.1, 0.6], [1.0, 2.5, 0.0], 1.0, 2, 2)
    assert counts.tolist() == [[0, 0], [0, 2]] and (outside, dropped) == (0, 1)


def test_moments_and_surface_brightness_on_synthetic_stamps():
    """a single cell, two cells, and a separable binned Gaussian whose moments are the sums over its cells; an empty stamp is NaN"""
    one = np.zeros((5, 7), dtype=np.int64)
    one[1, 5] = 10                                                   # cell centres: x = (5 + 1/2 - 7/2) s = 2 s, y = (1 + 1/2 - 5/2) s = -s
    two = np.zeros((5, 7), dtype=np.int64)
    two[2, 1], two[2, 5] = 3, 1                                      # x = -2 s (3 photons) and +2 s (1): mean -s, variance 3 s^2
    empty = np.zeros((5, 7), dtype=np.int64)
    res = _stamps(np.stack([one, two, empty]), scale=0.25)
    m = psf_image.moments(res)
    assert m["n"].tolist() == [10, 4, 0]
    assert (m["xbar"][0], m["ybar"][0], m["Ixx"][0], m["Iyy"][0], m["Ixy"][0]) == (0.5, -0.25, 0.0, 0.0, 0.0)
    assert (m["xbar"][1], m["ybar"][1], m["Iyy"][1], m["Ixy"][1]) == (-0.25, 0.0, 0.0, 0.0) and abs(m["Ixx"][1] - 3 * 0.0625) < 1e-15
    assert all(np.isnan(m[f][2]) for f in ("xbar", "ybar", "Ixx", "Iyy", "Ixy", "sigma", "e1", "e2"))
    x = psf_image.cell_centres(64, 0.1)
    assert abs(x[0] + 3.15) < 1e-15 and abs(x[32] - 0.05) < 1e-15 and abs(psf_image.cell_centres(5, 2.0)[2]) == 0.0
    gx, gy = np.round(1e6 * np.exp(-0.5 * ((x - 0.3) / 0.5) ** 2)), np.round(1e3 * np.exp(-0.5 * ((x + 0.2) / 0.8) ** 2))
    g = _stamps(np.outer(gy, gx).astype(np.int64), scale=0.1)
    mg = psf_image.moments(g)[0]
    xb, yb = (gx * x).sum() / gx.sum(), (gy * x).sum() / gy.sum()
    assert abs(mg["xbar"] - xb) < 1e-12 and abs(mg["ybar"] - yb) < 1e-12 and abs(mg["Ixy"]) < 1e-12
    assert abs(mg["Ixx"] - (gx * (x - xb) ** 2).sum() / gx.sum()) < 1e-12 and abs(mg["Iyy"] - (gy * (x - yb) ** 2).sum() / gy.sum()) < 1e-12
    # (the table samples the Gaussian at the cell centres, so its variance is sigma^2 without the s^2 / 12 of a cell integral)
    assert abs(mg["Ixx"] - 0.25) < 1e-4 and mg["e1"] < 0.0 and abs(mg["sigma"] ** 4 - mg["Ixx"] * mg["Iyy"]) < 1e-12
    sb = psf_image.surface_brightness(res)
    assert sb.shape == (3, 5, 7) and sb[0, 1, 5] == 1.0 / 0.0625 and abs(sb[1].sum() * 0.0625 - 1.0) < 1e-15 and np.all(np.isnan(sb[2]))


def test_file_written_and_read_back(tmp_path):
    """two CCDs: per CCD the cube as an f64 image [point][ny][nx] and the SUMMARY table"""
    counts = np.arange(4 * 3 * 5, dtype=np.int64).reshape(4, 3, 5)
    res = _stamps(counts, scale=0.2, stage="sensor", outside=[1, 2, 3, 4], dropped=[5, 6, 7, 2 ** 40])
    pts = np.array([[512.5, 500.5], [1536.5, 500.5], [512.5, 1500.5], [1536.5, 1500.5]])
    h = psf_image.make_header("R22_S11", res, 622.2, 19, 2048, 2000, 2, "centroid", sampled=True)
    fn = str(tmp_path / "sub" / "p.fits")
    item = (res.counts.astype(np.float64), h, psf_image.summary(res, pts), psf_image.summary_header("R22_S11"))
    psf_image.write(fn, [item, item])
    hdus = fits_io.read_fits(fn)
    assert len(hdus) == 4 and hdus[2][0]["XTENSION"] == "IMAGE"
    hc, cube = hdus[0]
    assert cube.dtype == np.float64 and cube.shape == (4, 3, 5) and np.array_equal(cube, counts)
    assert (hc["STAGE"], hc["UNITS"], hc["SCALE"], hc["NPHOT"], hc["NX"], hc["NY"], hc["CENTRE"], hc["DET_NAME"], hc["N_GRID"]) == \
        ("sensor", "pixel", 0.2, 19, 5, 3, "centroid", "R22_S11", 2)
    assert (hc["X_FIRST"], hc["X_STEP"], hc["Y_FIRST"], hc["Y_STEP"]) == (512.5, 1024.0, 500.5, 1000.0) and "PLANE1" not in hc
    assert psf_image.make_header("R22_S11", _stamps(counts, stage="psf"), 622.2, 19, 2048, 2000, 2, "nominal")["units"][0] == "arcsec"
    ht, t = hdus[3]
    assert (ht["XTENSION"], ht["EXTNAME"], ht["DET_NAME"]) == ("BINTABLE", "SUMMARY", "R22_S11") and list(t) == list(psf_image.SUMMARY)
    assert t["x"].tolist() == pts[:, 0].tolist() and t["y"].tolist() == pts[:, 1].tolist() and t["x"].dtype == np.float64
    assert t["n_used"].tolist() == counts.sum(axis=(1, 2)).tolist() and t["n_used"].dtype == np.int64
    assert t["n_outside"].tolist() == [1, 2, 3, 4] and t["n_dropped"].tolist() == [5, 6, 7, 2 ** 40]
