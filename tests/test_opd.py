"""The `opd` extra output, host side (no GPU): the annular Zernike basis, the field projections, the parsing of
output.opd, the header, and the argument checks of ims_opd."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from imsim_amd import _abi, config, optics, opd
from imsim_amd.lsst_image import GalSimConfigError

HERE = os.path.dirname(os.path.abspath(__file__))


def _polar(n=4000, seed=3, eps=0.0):
    rng = np.random.default_rng(seed)
    r = np.sqrt(rng.uniform(eps * eps, 1.0, n))
    th = rng.uniform(0.0, 2.0 * np.pi, n)
    return r, th


def test_zernike_basis_at_eps_zero_is_noll():
    r, th = _polar()
    Z = opd.zernike_basis(11, r * np.cos(th), r * np.sin(th), 1.0, 0.0)
    s3, s5, s6, s8 = math.sqrt(3), math.sqrt(5), math.sqrt(6), math.sqrt(8)
    noll = [np.ones_like(r), 2 * r * np.cos(th), 2 * r * np.sin(th), s3 * (2 * r * r - 1),
            s6 * r * r * np.sin(2 * th), s6 * r * r * np.cos(2 * th),
            s8 * (3 * r ** 3 - 2 * r) * np.sin(th), s8 * (3 * r ** 3 - 2 * r) * np.cos(th),
            s8 * r ** 3 * np.sin(3 * th), s8 * r ** 3 * np.cos(3 * th), s5 * (6 * r ** 4 - 6 * r * r + 1)]
    for j in range(11):
        np.testing.assert_allclose(Z[j], noll[j], rtol=0, atol=1e-13, err_msg=f"Z{j + 1}")


def test_zernike_basis_is_mahajans_annular_form():
    e = 0.612
    r, th = _polar(eps=e)
    R_o = 4.18
    Z = opd.zernike_basis(11, R_o * r * np.cos(th), R_o * r * np.sin(th), R_o, e)
    e2 = e * e
    np.testing.assert_allclose(Z[1], 2 * r * np.cos(th) / math.sqrt(1 + e2), rtol=0, atol=1e-12)
    np.testing.assert_allclose(Z[3], math.sqrt(3) * (2 * r * r - 1 - e2) / (1 - e2), rtol=0, atol=1e-12)
    np.testing.assert_allclose(Z[10], math.sqrt(5) * (6 * r ** 4 - 6 * (1 + e2) * r * r + 1 + 4 * e2 + e2 * e2) / (1 - e2) ** 2,
                               rtol=0, atol=1e-11)


@pytest.mark.parametrize("eps", [0.0, 0.612])
def test_zernike_basis_is_orthonormal_on_the_annulus(eps):
    """mean of Z_j Z_k over the annulus = delta_jk, by Gauss-Legendre in r (exact for these polynomials) and a uniform
    azimuth grid (exact for |m| + |m'| < 64)"""
    jmax = opd.MAX_JMAX
    gx, gw = np.polynomial.legendre.leggauss(40)
    r = eps + (1 - eps) * (gx + 1) / 2
    wr = gw * (1 - eps) / 2
    nt = 64
    th = 2 * np.pi * np.arange(nt) / nt
    R, T = np.meshgrid(r, th)
    W = np.meshgrid(wr, th)[0] * R * (2 * np.pi / nt) / (np.pi * (1 - eps * eps))
    Z = opd.zernike_basis(jmax, R * np.cos(T), R * np.sin(T), 1.0, eps)
    G = np.einsum("aij,bij,ij->ab", Z, Z, W)
    assert np.abs(G - np.eye(jmax)).max() < 1e-10


def test_noll_order_and_device_table():
    assert [opd.noll_to_nm(j) for j in range(1, 12)] == [(0, 0), (1, 1), (1, -1), (2, 0), (2, -2), (2, 2), (3, -1), (3, 1),
                                                         (3, -3), (3, 3), (4, 0)]
    assert [opd.noll_to_nm(j) for j in (22, 37, 55, 56, 65, 66)] == [(6, 0), (8, 0), (9, -9), (10, 0), (10, -10), (10, 10)]
    poly, m = opd.zernike_table(66, 0.3)
    assert poly.shape == (66, _abi.IMS_OPD_NPOW) and m.dtype == np.int32
    with pytest.raises(ValueError):
        opd.zernike_table(67, 0.3)


def test_projections():
    for proj in opd.PROJECTIONS:
        for th in [(0.0, 0.0), (0.02, -0.01), (0.3, 0.2)]:
            d = opd.field_direction(*th, proj)
            assert abs(np.linalg.norm(d) - 1.0) < 1e-15 and d[2] < 0
        d = opd.field_direction(0.01, 0.0, proj)
        assert d[0] > 0 and abs(d[1]) == 0.0          # +thx gives +x
    # the three agree to second order in small angles: differences are O(theta^3)
    for a in (1e-3, 2e-3, 4e-3):
        ds = [opd.field_direction(a, -0.5 * a, p) for p in opd.PROJECTIONS]
        for k in (1, 2):
            assert np.linalg.norm(ds[k] - ds[0]) < a ** 3
    # gnomonic is optics.pupil_rays' direction
    tel = optics.Telescope([], pupil_outer=4.18, pupil_inner=2.558)
    _, vel = optics.pupil_rays(tel, 0.013, -0.007)
    np.testing.assert_allclose(opd.field_direction(0.013, -0.007, "gnomonic"), vel[0] / np.linalg.norm(vel[0]), rtol=0, atol=4e-16)
    with pytest.raises(ValueError, match="projection"):
        opd.field_direction(0.0, 0.0, "stereographic")


def test_field_rotation():
    r = opd.rotate_field(0.01, 0.0, math.radians(90.0))
    assert abs(r[0]) < 1e-18 and abs(r[1] - 0.01) < 1e-18
    assert opd.rotate_field(0.01, -0.02, 0.0) == (0.01, -0.02)


def _ev():
    return config.Evaluator({})


def test_parse_output_opd():
    kw = config.parse_opd({"file_name": "opd.fits", "fields": [{"thx": "1.121 deg", "thy": "1.231 deg"}, {"thx": 0.0, "thy": 0.0}],
                           "nx": 64, "projection": "zemax", "wavelength": 694.0, "rotTelPos": "30 deg", "jmax": 22}, _ev())
    assert kw["fields"][0] == (math.radians(1.121), math.radians(1.231)) and kw["fields"][1] == (0.0, 0.0)
    assert (kw["nx"], kw["projection"], kw["wavelength"], kw["jmax"], kw["reference"]) == (64, "zemax", 694.0, 22, "chief")
    assert kw["rot_tel_pos"] == math.radians(30.0) and kw["sphere_radius"] is None and kw["eps"] is None
    d = config.parse_opd({"file_name": "o.fits", "fields": []}, _ev())
    assert (d["nx"], d["projection"], d["jmax"], d["wavelength"], d["rot_tel_pos"]) == (255, "postel", 28, None, 0.0)


@pytest.mark.parametrize("cfg,match", [
    ({"file_name": "o.fits"}, "fields"),
    ({"fields": []}, "file_name"),
    ({"file_name": "o.fits", "fields": [], "n_x": 3}, "n_x"),
    ({"file_name": "o.fits", "fields": [], "projection": "stereographic"}, "projection"),
    ({"file_name": "o.fits", "fields": [], "reference": "centroid"}, "reference"),
    ({"file_name": "o.fits", "fields": [], "jmax": 67}, "jmax"),
    ({"file_name": "o.fits", "fields": [{"thx": 0.0}]}, "thx"),
])
def test_parse_output_opd_errors(cfg, match):
    with pytest.raises(GalSimConfigError, match=match):
        config.parse_opd(cfg, _ev())


def test_header_keys():
    zk = np.arange(1.0, 29.0)
    h = opd.make_header(0.01, 0.02, 0.015, 0.01, 0.0328, 620.0, "postel", 2.7, "chief", 0.612, 28, "rubin_like_r", zk)
    assert list(h) == list(opd.HEADER_KEYS) + [f"AZ_{j:03d}" for j in range(1, 29)]
    assert h["AZ_028"][0] == 28.0 and h["thx"][0] == math.degrees(0.01) and h["units"][0] == "nm"
    w = opd.wcs_cards(255, 0.0328)
    assert w["GS_SCALE"][0] == w["CD1_1"][0] == w["CD2_2"][0] == 0.0328 and w["CD1_2"][0] == w["CD2_1"][0] == 0.0
    assert w["GS_U0"][0] == 0.0 and opd.wcs_cards(256, 0.0328)["GS_U0"][0] == 0.5 * 0.0328


def test_write_reads_back(tmp_path):
    from imsim_amd import fits_io
    a = np.full((5, 5), np.nan)
    a[0, 1] = 1.5
    h = opd.make_header(0.0, 0.0, 0.0, 0.0, 0.2, 620.0, "postel", 2.7, "mean", 0.2, 3, "t", [1.0, 2.0, 3.0])
    fn = str(tmp_path / "opd.fits")
    opd.write(fn, [(a, h), (a * 2, h)])
    hdus = fits_io.read_fits(fn)
    assert len(hdus) == 2
    assert hdus[0][1].dtype == np.float64 and np.array_equal(np.isnan(hdus[0][1]), np.isnan(a)) and hdus[1][1][0, 1] == 3.0
    assert hdus[1][0]["XTENSION"] == "IMAGE" and hdus[0][0]["AZ_003"] == 3.0 and hdus[0][0]["SPH_REF"] == "mean"
    assert hdus[0][0]["GS_SCALE"] == hdus[0][0]["CD1_1"] == 0.2


def test_compute_checks_parameters_before_the_gpu():
    tel = optics.Telescope([], pupil_outer=0.5, pupil_inner=0.1)
    with pytest.raises(ValueError, match="sphere"):
        opd.compute(tel, [(0.0, 0.0)], 620.0)                 # no sphere radius known
    with pytest.raises(ValueError, match="jmax"):
        opd.compute(tel, [(0.0, 0.0)], 620.0, sphere_radius=1.0, jmax=80)
    with pytest.raises(ValueError, match="reference"):
        opd.compute(tel, [(0.0, 0.0)], 620.0, sphere_radius=1.0, reference="centroid")


def test_telescope_sphere_radius_and_eps():
    assert optics.Telescope([]).sphere_radius is None and optics.Telescope([]).eps is None
    assert optics.rubin_like_telescope(refocus=False).sphere_radius == optics.RUBIN_LIKE_SPHERE_RADIUS


def test_batoid_yaml_sphere_radius(tmp_path):
    p = tmp_path / "t.yaml"
    p.write_text("opticalSystem:\n  type: CompoundOptic\n  name: T\n  pupilSize: 1.0\n  pupilObscuration: 0.25\n"
                 "  sphereRadius: 3.5\n  items:\n    - type: Detector\n      name: D\n      coordSys: {z: 2.0}\n"
                 "      surface: {type: Plane}\n")
    tel = optics.load_batoid_yaml(str(p))
    assert (tel.sphere_radius, tel.eps, tel.pupil_outer, tel.pupil_inner) == (3.5, 0.25, 0.5, 0.125)


def test_ims_opd_checks_arguments_before_any_hip_call():
    lib = _abi.load()
    assert lib.ims_opd(None, None, None) == -1 and b"NULL" in lib.ims_last_error()
    P = _abi.Opd()
    P.n_fields, P.nx, P.reference, P.jmax, P.dx, P.wavelength, P.sphere_radius = 1, 0, 0, 0, 0.01, 620.0, 1.0
    opt = C.c_void_p(8)                                   # never dereferenced: every check fails first
    assert lib.ims_opd(C.byref(P), opt, None) == -1 and b"nx" in lib.ims_last_error()
    P.nx = 4097
    assert lib.ims_opd(C.byref(P), opt, None) == -1 and b"nx" in lib.ims_last_error()
    P.nx, P.reference = 16, 2
    assert lib.ims_opd(C.byref(P), opt, None) == -1 and b"reference" in lib.ims_last_error()
    P.reference, P.jmax = 1, 67
    assert lib.ims_opd(C.byref(P), opt, None) == -1 and b"jmax" in lib.ims_last_error()
    P.jmax, P.sphere_radius = 0, 0.0
    assert lib.ims_opd(C.byref(P), opt, None) == -1 and b"sphere_radius" in lib.ims_last_error()
    P.sphere_radius = 1.0
    assert lib.ims_opd(C.byref(P), opt, None) == -1 and b"NULL" in lib.ims_last_error()       # no dirs / opd / scratch
    P.dirs = P.opd = P.scratch = 8
    P.jmax = 4
    assert lib.ims_opd(C.byref(P), opt, None) == -1 and b"Zernike" in lib.ims_last_error()
    P.n_fields = 0
    assert lib.ims_opd(C.byref(P), opt, None) == 0                                            # nothing to do
    assert lib.ims_struct_size(_abi.OPD_STRUCT_INDEX) == C.sizeof(_abi.Opd) and _abi.Opd not in _abi.STRUCTS
    assert _abi.opd_scratch_bytes(3, 255, 28) == 8 * 3 * (10 * (255 * 255 + 1) + 6 * 255 + 4 + 16 * (28 * 31 // 2))
