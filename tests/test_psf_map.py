"""output.psf_map on the host (no GPU): the parsing of the config key, the host formulae on hand-made sums, the point rows, the
FITS cube read back, and the argument checks of ims_psf_moments."""
import ctypes as C
import math

import numpy as np
import pytest

from imsim_amd import _abi, config, configs, fits_io, psf_map
from imsim_amd.lsst_image import GalSimConfigError


def _ev():
    return config.Evaluator({})


def test_parse_output_psf_map():
    assert psf_map.parse_config({"file_name": "m.fits"}, _ev()) == dict(nx=8, n_photons=100000, stage="psf")
    kw = psf_map.parse_config({"file_name": "m.fits", "dir": "out", "nx": 3, "n_photons": 2000, "stage": "ops"}, _ev())
    assert kw == dict(nx=3, n_photons=2000, stage="ops")


@pytest.mark.parametrize("cfg,match", [
    ("m.fits", "must be a dict"),
    ({"nx": 4}, "file_name is required"),
    ({"file_name": "m.fits", "ny": 4}, "Unexpected attribute ny"),
    ({"file_name": "m.fits", "stage": "sensor"}, "stage must be one of"),
    ({"file_name": "m.fits", "nx": 0}, "nx must be at least 1"),
    ({"file_name": "m.fits", "n_photons": 0}, "n_photons must be at least 1"),
])
def test_parse_output_psf_map_errors(cfg, match):
    with pytest.raises(GalSimConfigError, match=match):
        psf_map.parse_config(cfg, _ev())


def test_moments_from_hand_made_sums():
    """three photons of weight 1, 2, 1 at (1, 0), (0, 1), (-1, 0); a point that lost everything; a single photon"""
    w, x, y = np.array([1.0, 2.0, 1.0]), np.array([1.0, 0.0, -1.0]), np.array([0.0, 1.0, 0.0])
    s = [w.sum(), (w * x).sum(), (w * y).sum(), (w * x * x).sum(), (w * x * y).sum(), (w * y * y).sum()]
    m = psf_map.moments_from_sums([s, [0.0] * 6, [1.0, 0.5, -0.25, 0.25, -0.125, 0.0625]], [[3, 1], [0, 7], [1, 0]])
    assert m.dtype == psf_map.MOMENTS_DTYPE
    a = m[0]
    assert (a["flux"], a["n_used"], a["n_dropped"], a["xbar"], a["ybar"]) == (4.0, 3, 1, 0.0, 0.5)
    assert (a["Ixx"], a["Iyy"], a["Ixy"]) == (0.5, 0.25, 0.0)
    assert a["sigma"] == (0.5 * 0.25) ** 0.25 and a["fwhm"] == 2.3548200450309493 * a["sigma"]
    assert a["e1"] == (0.5 - 0.25) / 0.75 and a["e2"] == 0.0
    b = m[1]
    assert (b["flux"], b["n_used"], b["n_dropped"]) == (0.0, 0, 7)
    assert all(np.isnan(b[f]) for f in ("xbar", "ybar", "Ixx", "Iyy", "Ixy", "sigma", "e1", "e2", "fwhm"))
    c = m[2]                                                   # one photon at (0.5, -0.25): no width
    assert (c["xbar"], c["ybar"], c["Ixx"], c["Iyy"], c["Ixy"], c["sigma"]) == (0.5, -0.25, 0.0, 0.0, 0.0, 0.0)
    # e2 and the cross moment: weights 1, 1 at (1, 1) and (-1, -1)
    d = psf_map.moments_from_sums([[2.0, 0.0, 0.0, 2.0, 2.0, 2.0]], [[2, 0]])[0]
    assert (d["Ixx"], d["Iyy"], d["Ixy"], d["e1"], d["e2"], d["sigma"]) == (1.0, 1.0, 1.0, 0.0, 1.0, 0.0)
    assert len(psf_map.moments_from_sums(np.zeros((0, 6)), np.zeros((0, 2)))) == 0


def test_point_rows():
    sc = configs.scene_c3(nx=64, ny=64, sensor=False)
    xy = np.array([[10.0, 20.0], [50.5, 40.25]])
    a = psf_map.point_rows(sc, xy, 1000, "psf")
    assert a["obj_id"].tolist() == [0, 1] and a["n_phot"].tolist() == [1000, 1000] and np.all(a["prof_table"] == _abi.IMS_PROF_POINT)
    assert np.all(a["winv"] == (1.0, 0.0, 0.0, 1.0)) and np.all(a["sed_table"] == 0) and np.all(a["flux_per_photon"] == 1.0)
    thx, thy = configs.field_angles(sc, xy[:, 0], xy[:, 1])
    assert np.array_equal(a["atm_tan_x"], thx) and np.array_equal(a["atm_tan_y"], thy)
    b = psf_map.point_rows(sc, xy, [5, 7], "ops", wavelength=700.0)
    assert b["n_phot"].tolist() == [5, 7] and np.all(b["sed_table"] == -1) and np.all(b["sed_wave"] == 700.0)
    assert np.array_equal(b["winv"], configs.local_wcs_inverse(sc.optics.img_wcs, xy[:, 0], xy[:, 1])[0])
    assert (b["x0"].tolist(), b["y0"].tolist()) == (xy[:, 0].tolist(), xy[:, 1].tolist())
    bare = psf_map._as_scene([(_abi.IMS_PSF_GAUSSIAN, 0, 0.3, 0.0, 1.0)])
    with pytest.raises(ValueError, match="wavelength"):
        psf_map.point_rows(bare, xy, 10, "psf")
    on_axis = psf_map.point_rows(bare, xy, 10, "psf", wavelength=620.0)
    assert np.all(on_axis["atm_tan_x"] == 0.0) and np.all(on_axis["atm_tan_y"] == 0.0)
    with pytest.raises(ValueError, match="stage"):
        psf_map.compute(bare, xy, 10, stage="sensor", wavelength=620.0)


def test_grid_and_cube_written_and_read_back(tmp_path):
    pts = psf_map.grid_points(4096, 4000, 2)
    assert pts.tolist() == [[1024.5, 1000.5], [3072.5, 1000.5], [1024.5, 3000.5], [3072.5, 3000.5]]
    sums = np.array([[10.0, 1.0, 2.0, 30.0, 0.5, 20.0], [0.0] * 6, [4.0, 0.0, 0.0, 4.0, 0.0, 16.0], [2.0, 2.0, 2.0, 4.0, 2.0, 4.0]])
    m = psf_map.moments_from_sums(sums, [[10, 0], [0, 5], [4, 1], [2, 3]])
    cube = psf_map.cube(m, 2)
    assert cube.shape == (len(psf_map.PLANES), 2, 2)
    hdr = psf_map.make_header("R22_S11", "psf", 622.2, 5, 4096, 4000, 2, sampled=True)
    fn = str(tmp_path / "sub" / "map.fits")
    psf_map.write(fn, [(cube, hdr), (cube[:, ::-1], psf_map.make_header("R22_S12", "ops", 700.0, 5, 4096, 4000, 2))])
    hdus = fits_io.read_fits(fn)
    assert len(hdus) == 2
    h, data = hdus[0]
    assert data.dtype == np.float64 and data.tobytes() == cube.tobytes()
    assert [h[f"PLANE{k + 1}"] for k in range(len(psf_map.PLANES))] == [name for name, _ in psf_map.PLANES]
    assert [name for name, _ in psf_map.PLANES] == list(psf_map.MOMENTS_DTYPE.names)
    assert (h["DET_NAME"], h["STAGE"], h["UNITS"], h["WAVELEN"], h["NPHOT"]) == ("R22_S11", "psf", "arcsec", 622.2, 5)
    assert (h["X_FIRST"], h["X_STEP"], h["Y_FIRST"], h["Y_STEP"]) == (1024.5, 2048.0, 1000.5, 2000.0)
    names = [name for name, _ in psf_map.PLANES]
    assert data[names.index("n_dropped")].tolist() == [[0.0, 5.0], [1.0, 3.0]]               # [ny][nx], x fastest
    assert np.isnan(data[names.index("sigma")][0, 1]) and data[names.index("flux")][0, 1] == 0.0
    assert data[names.index("Iyy")][1, 0] == 4.0 and data[names.index("e1")][1, 0] == (1.0 - 4.0) / 5.0
    h2, d2 = hdus[1]
    assert (h2["XTENSION"], h2["DET_NAME"], h2["STAGE"], h2["UNITS"]) == ("IMAGE", "R22_S12", "ops", "pixel")
    assert d2.tobytes() == np.ascontiguousarray(cube[:, ::-1]).tobytes()


def test_argument_errors_are_reported_before_any_launch():
    lib = _abi.load()
    assert "ims_psf_moments" in _abi.EXPORTS
    assert lib.ims_psf_moments(None, 1, None, None, None, None) == -1 and b"NULL" in lib.ims_last_error()
    P = _abi.RenderParams()
    P.seg_size = 256
    assert lib.ims_psf_moments(C.byref(P), 3, None, None, None, None) == -1 and b"stage" in lib.ims_last_error()
    assert lib.ims_psf_moments(C.byref(P), 1, None, None, None, None) == 0          # no points: nothing to do
    rows = (C.c_double * 32)()
    pre = (C.c_int64 * 2)(0, 1)
    P.n_objects, P.objects, P.seg_prefix, P.n_segments = 1, C.cast(rows, C.c_void_p), C.cast(pre, C.c_void_p), 1
    assert lib.ims_psf_moments(C.byref(P), 2, None, None, None, None) == -1 and b"sums" in lib.ims_last_error()
    out = (C.c_double * 8)()
    assert lib.ims_psf_moments(C.byref(P), 2, None, out, out, None) == -1 and b"partial" in lib.ims_last_error()
    P.seg_size = 128
    assert lib.ims_psf_moments(C.byref(P), 1, out, out, out, None) == -1 and b"seg_size" in lib.ims_last_error()
    assert math.isfinite(psf_map.FWHM_PER_SIGMA) and psf_map.FWHM_PER_SIGMA == 2.3548200450309493
