"""output.psf_profile on the host (no GPU): the numpy restatement of the binning rule on hand-made offsets, the estimators on
synthetic counts with known answers, the parsing of the config key, the refusals, and the argument checks of ims_psf_profile."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from imsim_amd import _abi, config, configs, fits_io, psf_profile
from imsim_amd.lsst_image import GalSimConfigError
from psf_profile_ref import binning_reference, counts_reference

HERE = os.path.dirname(os.path.abspath(__file__))


def _ev():
    return config.Evaluator({})


def _result(radial, r_edges, n_phi=0):
    """a Profile of one point per row of `radial` (counts per radial index, all in sector column 0)"""
    radial = np.atleast_2d(np.asarray(radial, dtype=np.int64))
    counts = np.zeros(radial.shape + (n_phi + 1,), dtype=np.int64)
    counts[:, :, 0] = radial
    r = np.asarray(r_edges, dtype=np.float64)
    return psf_profile.Profile(counts=counts, n_used=counts.sum(axis=(1, 2)), n_dropped=np.zeros(len(counts), dtype=np.int64),
                               r_edges=r, r2_edges=r * r, dirs=psf_profile.sector_dirs(n_phi))


def test_binning_reference_radial_edges():
    """edges 1, 4, 9 (radii 1, 2, 3): on an edge -> the bin above it; below the first -> underflow; at or beyond the last -> overflow"""
    e = np.array([1.0, 4.0, 9.0])
    dx = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 0.0, 3.0, 5.0, 0.6, np.nan])
    dy = np.array([0.0, 0.5, 0.0, 0.0, 0.0, -2.5, 0.0, 5.0, 0.8, 0.0])
    radial, sector = binning_reference(dx, dy, e, np.zeros((0, 2)))
    #                          centre .5,.5  r=1  1.5  r=2  2.5  r=3  far  r=1 (0.36 + 0.64 rounds to 1)  NaN
    assert radial.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 1, 0]
    assert sector.tolist() == [0] * 10
    counts, dropped = counts_reference(dx, dy, np.array([1.0] * 8 + [0.0, 1.0]), e, np.zeros((0, 2)))
    assert counts.shape == (4, 1) and counts[:, 0].tolist() == [3, 2, 2, 2] and dropped == 1


def test_binning_reference_sectors():
    """four sectors from the exact directions (1,0), (0,1), (-1,0), (0,-1): a point on a sector's start direction belongs to that
    sector, the centre and a NaN to none (index n_phi)"""
    d = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    dx = np.array([1.0, 1.0, 0.0, -1.0, -2.0, -1.0, 0.0, 1.0, 0.0, np.nan])
    dy = np.array([0.0, 1.0, 3.0, 1.0, 0.0, -1.0, -0.5, -1.0, 0.0, 1.0])
    _, sector = binning_reference(dx, dy, [1.0, 2.0], d)
    assert sector.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    # the directions the product forms for phi0 = 0: cos(pi / 2) is 6e-17, not 0, so direction 1 lies a hair clockwise of the +y
    # axis and a point on that axis has t_1 = 6e-17 > 0: sector 1 -- the rule is stated on the array the device gets
    p = psf_profile.sector_dirs(4)
    assert p.shape == (4, 2) and p[0].tolist() == [1.0, 0.0] and p[1, 0] > 0.0
    _, s2 = binning_reference([0.0, 1.0], [1.0, 0.0], [1.0, 2.0], p)
    assert s2.tolist() == [1, 0]
    # an offset exactly along direction b (any exact multiple of it) has t_b = 0: sector b
    dd = np.array([[3.0, 1.0], [-1.0, 3.0], [-3.0, -1.0], [1.0, -3.0]]) / 4.0
    _, s3 = binning_reference(8.0 * dd[:, 0], 8.0 * dd[:, 1], [1.0, 2.0], dd)
    assert s3.tolist() == [0, 1, 2, 3]


def test_surface_density_and_encircled_energy():
    """10 photons: 1 inside r = 1, 3 in [1, 2), 4 in [2, 4), 2 beyond"""
    res = _result([[1, 3, 4, 2], [0, 0, 0, 0]], [1.0, 2.0, 4.0])
    sd = psf_profile.surface_density(res)
    assert sd[0].tolist() == [3.0 / (math.pi * 3.0) / 10.0, 4.0 / (math.pi * 12.0) / 10.0]
    ee = psf_profile.encircled_energy(res)
    assert ee[0].tolist() == [0.1, 0.4, 0.8]
    assert np.all(np.isnan(sd[1])) and np.all(np.isnan(ee[1]))                  # no photon arrived: nothing raises
    assert psf_profile.radial_counts(res)[0].tolist() == [1, 3, 4, 2]


def test_ee_radius_is_linear_between_edges():
    res = _result([[1, 3, 4, 2], [0, 0, 0, 0]], [1.0, 2.0, 4.0])
    assert psf_profile.ee_radius(res, 0.4)[0] == 2.0 and psf_profile.ee_radius(res, 0.1)[0] == 1.0
    assert psf_profile.ee_radius(res, 0.8)[0] == 4.0
    assert psf_profile.ee_radius(res, 0.25)[0] == pytest.approx(1.5, abs=1e-15)
    assert psf_profile.ee_radius(res, 0.6)[0] == pytest.approx(3.0, abs=1e-15)
    assert np.isnan(psf_profile.ee_radius(res, 0.05)[0]) and np.isnan(psf_profile.ee_radius(res, 0.9)[0])
    assert np.isnan(psf_profile.ee_radius(res, 0.5)[1])
    s = psf_profile.summary(res)
    assert s.shape == (2, 5) and s[0, :2].tolist() == [10.0, 0.0] and abs(s[0, 2] - 2.5) < 1e-14 and s[0, 3] == 4.0 and np.isnan(s[0, 4])


def test_halo_law_recovers_an_exact_inverse_square_table():
    """Edges 2^k: the annulus [2^k, 2^(k+1)) has area 3 pi 4^k and geometric-mean radius r_mid = 2^(k + 1/2), so equal counts C
    in every bin give the density C / (3 pi 4^k N) = (2 C / (3 pi N)) / r_mid^2: an exact 1/r^2 table, slope -2 and intercept
    log10(2 C / (3 pi N)), N the photons that arrived."""
    edges = 2.0 ** np.arange(0, 9)
    c = 1000
    res = _result([[0] + [c] * 8 + [0]], edges)
    slope, icpt = psf_profile.halo_law(res, 1.0, 256.0)
    assert abs(slope[0] + 2.0) <= 1e-12
    assert abs(icpt[0] - math.log10(2.0 * c / (3.0 * math.pi * 8 * c))) <= 1e-12
    # a sub-range, and empty bins left out: the same line
    sparse = _result([[0, c, 0, c, c, 0, c, c, c, 0]], edges)
    s2, i2 = psf_profile.halo_law(sparse, 1.0, 256.0)
    assert abs(s2[0] + 2.0) <= 1e-12 and abs(i2[0] - math.log10(2.0 * c / (3.0 * math.pi * 6 * c))) <= 1e-12
    s3, _ = psf_profile.halo_law(res, 4.0, 64.0)
    assert abs(s3[0] + 2.0) <= 1e-12
    # a flat density (counts proportional to the area): slope 0; fewer than two bins: NaN
    flat = _result([[0] + [3 * 4 ** k for k in range(8)] + [0]], edges)
    assert abs(psf_profile.halo_law(flat, 1.0, 256.0)[0][0]) <= 1e-12
    assert np.isnan(psf_profile.halo_law(res, 1.0, 2.0)[0][0]) and np.isnan(psf_profile.halo_law(res, 300.0, 400.0)[1][0])


def test_file_written_and_read_back(tmp_path):
    """two CCDs: per CCD the cube as an f64 image and the SUMMARY table, NaN radii kept"""
    res = _result([[1, 3, 4, 2], [0, 0, 0, 0]], [1.0, 2.0, 4.0], n_phi=3)
    res.n_dropped = np.array([5, 9])
    h = psf_profile.make_header("R22_S11", res, 622.2, 19, 4096, 4000, 1, "nominal", sampled=True)
    fn = str(tmp_path / "sub" / "p.fits")
    item = (res.counts.astype(np.float64), h, psf_profile.summary(res), psf_profile.summary_header("R22_S11"))
    psf_profile.write(fn, [item, item])
    hdus = fits_io.read_fits(fn)
    assert len(hdus) == 4 and hdus[2][0]["XTENSION"] == "IMAGE"
    hc, cube = hdus[0]
    assert cube.dtype == np.float64 and cube.shape == (2, 4, 4) and np.array_equal(cube, res.counts)
    assert (hc["STAGE"], hc["UNITS"], hc["N_R"], hc["N_PHI"], hc["PHI0"], hc["NPHOT"], hc["CENTRE"]) == ("psf", "arcsec", 2, 3, 0.0, 19, "nominal")
    assert [hc[f"R_EDGE{k}"] for k in range(3)] == [1.0, 2.0, 4.0] and "PLANE1" not in hc
    ht, t = hdus[3]
    assert (ht["XTENSION"], ht["EXTNAME"], ht["DET_NAME"]) == ("BINTABLE", "SUMMARY", "R22_S11") and list(t) == list(psf_profile.SUMMARY)
    assert t["n_used"].tolist() == [10, 0] and t["n_dropped"].tolist() == [5, 9]
    assert abs(t["EE50"][0] - 2.5) < 1e-14 and t["EE80"][0] == 4.0 and np.isnan(t["EE95"][0]) and np.isnan(t["EE50"][1])


def test_radial_edges_and_bins_checked():
    assert psf_profile.radial_edges(0.0, 4.0, 4, "linear").tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    e = psf_profile.radial_edges(0.01, 100.0, 32, "log")
    assert len(e) == 33 and e[0] == 0.01 and e[-1] == 100.0 and np.all(np.diff(e) > 0) and abs(e[16] - 1.0) < 1e-12
    for bad, match in (([1.0], "n_r"), (np.arange(67.0), "n_r"), ([1.0, 1.0], "ascending"), ([2.0, 1.0], "ascending"),
                       ([-1.0, 1.0], "ascending"), ([0.0, np.inf], "ascending")):
        with pytest.raises(ValueError, match=match):
            psf_profile.check_bins(bad, 0)
    for n_phi in (1, 2, 65, -3):
        with pytest.raises(ValueError, match="n_phi"):
            psf_profile.check_bins([0.0, 1.0], n_phi)
    assert psf_profile.check_bins([0.0, 1.0], 64)[1] == 64


def test_parse_output_psf_profile():
    kw = psf_profile.parse_config({"file_name": "p.fits", "r_min": 0.01, "r_max": 10.0}, _ev())
    assert (kw["nx"], kw["n_photons"], kw["stage"], kw["n_phi"], kw["phi0"], kw["centre"]) == (4, 1000000, "psf", 0, 0.0, "nominal")
    assert kw["r_edges"].tolist() == psf_profile.radial_edges(0.01, 10.0, 32, "log").tolist()
    kw = psf_profile.parse_config({"file_name": "p.fits", "dir": "out", "nx": 2, "n_photons": 5000, "stage": "ops", "r_min": 0, "r_max": 8,
                                   "n_r": 16, "spacing": "linear", "n_phi": 12, "phi0": "30 deg", "centre": "centroid"}, _ev())
    assert (kw["nx"], kw["n_photons"], kw["stage"], kw["n_phi"], kw["centre"]) == (2, 5000, "ops", 12, "centroid")
    assert kw["phi0"] == 30.0 * math.pi / 180.0 and kw["r_edges"].tolist() == (0.5 * np.arange(17)).tolist()


@pytest.mark.parametrize("cfg,match", [
    ("p.fits", "must be a dict"),
    ({"r_min": 1, "r_max": 2}, "file_name is required"),
    ({"file_name": "p.fits", "r_max": 2}, "r_min is required"),
    ({"file_name": "p.fits", "r_min": 1, "r_max": 2, "ny": 4}, "Unexpected attribute ny"),
    ({"file_name": "p.fits", "r_min": 1, "r_max": 2, "stage": "sensor"}, "stage must be one of"),
    ({"file_name": "p.fits", "r_min": 1, "r_max": 2, "n_r": 0}, "n_r must be"),
    ({"file_name": "p.fits", "r_min": 1, "r_max": 2, "n_r": 65}, "n_r must be"),
    ({"file_name": "p.fits", "r_min": 1, "r_max": 2, "n_phi": 2}, "n_phi must be"),
    ({"file_name": "p.fits", "r_min": 1, "r_max": 2, "n_phi": 65}, "n_phi must be"),
    ({"file_name": "p.fits", "r_min": 2, "r_max": 2}, "r_min must be below r_max"),
    ({"file_name": "p.fits", "r_min": 3, "r_max": 2, "spacing": "linear"}, "r_min must be below r_max"),
    ({"file_name": "p.fits", "r_min": 0, "r_max": 2}, "r_min must be positive with spacing: log"),
    ({"file_name": "p.fits", "r_min": 1, "r_max": 2, "spacing": "sqrt"}, "spacing must be"),
    ({"file_name": "p.fits", "r_min": 1, "r_max": 2, "centre": "peak"}, "centre must be"),
    ({"file_name": "p.fits", "r_min": 1, "r_max": 2, "phi0": "north"}, "phi0"),
    ({"file_name": "p.fits", "r_min": 1, "r_max": 2, "nx": 0}, "nx must be at least 1"),
    ({"file_name": "p.fits", "r_min": 1, "r_max": 2, "n_photons": 0}, "n_photons must be at least 1"),
])
def test_parse_output_psf_profile_errors(cfg, match):
    with pytest.raises(GalSimConfigError, match=match):
        psf_profile.parse_config(cfg, _ev())


def test_bandpass_ratio_is_refused():
    """the counts are unweighted: profile() raises ValueError and config.Process a config error, both naming the operator, before
    any GPU work; stage psf, which runs no operator, is not refused on that account"""
    sc = configs.scene_c3(nx=64, ny=64, sensor=False)
    sc.ops = list(sc.ops) + [(_abi.IMS_OP_BANDPASS_RATIO, 0, [])]
    with pytest.raises(ValueError, match="BandpassRatio"):
        psf_profile.profile(sc, np.array([[10.0, 20.0]]), 100, [0.0, 1.0], stage="ops", device="no such device")
    psf_profile.refuse_flux_operators(sc, "psf")
    with pytest.raises(GalSimConfigError, match="BandpassRatio"):
        psf_profile.check_scene(sc, "ops")
    o = {"input.instance_catalog.file_name": os.path.join(HERE, "golden", "example_instcat_subset.txt"), "image.nobjects": 3,
         "stamp.draw_method": "phot",
         "stamp.photon_ops": [{"type": "BandpassRatio", "target_bandpass": "@bandpass", "initial_bandpass": "@bandpass"}],
         "output.psf_profile": {"file_name": "p.fits", "stage": "ops", "r_min": 0.1, "r_max": 10.0}}
    with pytest.raises(GalSimConfigError, match="BandpassRatio"):
        config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")], overrides=o)
    # a config error of the key itself comes first, and a flat lists the key as ignored
    o["output.psf_profile"] = {"file_name": "p.fits", "r_min": 3.0, "r_max": 1.0}
    with pytest.raises(GalSimConfigError, match="r_min must be below r_max"):
        config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")], overrides=o)


def test_argument_errors_are_reported_before_any_launch():
    lib = _abi.load()
    assert "ims_psf_profile" in _abi.EXPORTS and lib.ims_abi_version() == 22
    with open(os.path.join(HERE, "..", "include", "imsim_hip.h")) as f:
        header = f.read()
    assert "#define IMS_ABI_VERSION 22" in header and "ims_psf_profile(" in header and C.sizeof(_abi.PsfProfile) == 24
    spec = _abi.PsfProfile(4, 3, None, None)
    assert lib.ims_psf_profile(None, 1, C.byref(spec), None, None, None, None) == -1 and b"NULL" in lib.ims_last_error()
    P = _abi.RenderParams()
    P.seg_size = 256
    assert lib.ims_psf_profile(C.byref(P), 1, None, None, None, None, None) == -1 and b"spec is NULL" in lib.ims_last_error()
    for stage in (0, 3):
        assert lib.ims_psf_profile(C.byref(P), stage, C.byref(spec), None, None, None, None) == -1 and b"stage" in lib.ims_last_error()
    for n_r, n_phi, word in ((0, 0, b"n_r"), (65, 0, b"n_r"), (-1, 0, b"n_r"), (4, 1, b"n_phi"), (4, 2, b"n_phi"), (4, 65, b"n_phi"),
                             (4, -3, b"n_phi")):
        bad = _abi.PsfProfile(n_r, n_phi, None, None)
        assert lib.ims_psf_profile(C.byref(P), 1, C.byref(bad), None, None, None, None) == -1 and word in lib.ims_last_error()
    assert lib.ims_psf_profile(C.byref(P), 1, C.byref(spec), None, None, None, None) == 0          # no rows: nothing to do
    rows = (C.c_double * 32)()
    pre = (C.c_int64 * 2)(0, 1)
    P.n_objects, P.objects, P.seg_prefix, P.n_segments = 1, C.cast(rows, C.c_void_p), C.cast(pre, C.c_void_p), 1
    out = (C.c_int64 * 64)(*([7] * 64))
    tab = (C.c_double * 8)()
    tab_p = C.cast(tab, C.c_void_p)
    assert lib.ims_psf_profile(C.byref(P), 2, C.byref(spec), None, None, out, None) == -1 and b"counts" in lib.ims_last_error()
    assert lib.ims_psf_profile(C.byref(P), 2, C.byref(spec), None, out, out, None) == -1 and b"r2_edge" in lib.ims_last_error()
    no_dir = _abi.PsfProfile(4, 3, tab_p, None)
    assert lib.ims_psf_profile(C.byref(P), 2, C.byref(no_dir), None, out, out, None) == -1 and b"dir" in lib.ims_last_error()
    full = _abi.PsfProfile(4, 3, tab_p, tab_p)
    P.n_ops = 1
    P.ops[0].kind = _abi.IMS_OP_BANDPASS_RATIO
    assert lib.ims_psf_profile(C.byref(P), 2, C.byref(full), None, out, out, None) == -4 and b"BandpassRatio" in lib.ims_last_error()
    P.seg_size = 128
    assert lib.ims_psf_profile(C.byref(P), 1, C.byref(full), None, out, out, None) == -1 and b"seg_size" in lib.ims_last_error()
    assert list(out) == [7] * 64                                                                  # nothing was written
