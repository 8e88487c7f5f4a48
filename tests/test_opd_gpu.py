"""The `opd` extra output on the GPU (ims_opd): closed-form telescopes, the numpy restatement (tests/opd_numpy.py),
determinism, and the end-to-end run through config.Process."""
import math
import os

import numpy as np
import pytest

from imsim_amd import config, fits_io, opd, optics, tables
import opd_numpy

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _grid(tel, nx):
    dx = 2.0 * tel.pupil_outer / nx
    c = (np.arange(nx) - (nx - 1) / 2.0) * dx
    return np.meshgrid(c, c)


def _zk(header, jmax):
    return np.array([header[f"AZ_{j:03d}"][0] for j in range(1, jmax + 1)])


def test_perfect_paraboloid_on_axis(torch_cuda):
    tel = opd_numpy.one_mirror()
    for R_s in (1.0, 10.0, 50.0):
        (m, h), = opd.compute(tel, [(0.0, 0.0)], 620.0, nx=128, sphere_radius=R_s)
        f = np.isfinite(m)
        assert f.sum() > 10000 and np.abs(m[f]).max() < 1e-3
        assert h["sph_rad"][0] == R_s


@pytest.mark.parametrize("dz", [1e-4, -1e-4])
def test_defocus_is_pure_z4(torch_cuda, dz):
    tel = opd_numpy.one_mirror(det_z=10.0 + dz)
    (m, h), = opd.compute(tel, [(0.0, 0.0)], 620.0, nx=255)
    zk = _zk(h, 28)
    expect = dz * 0.5 ** 2 * (1 - 0.2 ** 2) / (4 * math.sqrt(3) * 10.0 ** 2) * 1e9
    assert abs(zk[3] / expect - 1) < 5e-3 and np.sign(zk[3]) == np.sign(dz)
    assert np.abs(zk[4:]).max() <= 1e-2 * abs(zk[3])


def _against_model(m, tel, W):
    X, Y = _grid(tel, m.shape[0])
    w = W(np.hypot(X, Y))
    f = np.isfinite(m)
    res = (m[f] - m[f].mean()) - (w[f] - w[f].mean())
    return np.abs(res).max() / np.ptp(w[f])


def test_spherical_mirror_third_order(torch_cuda):
    tel = opd_numpy.one_mirror(conic=0.0, det_z=10.0)
    (m, _), = opd.compute(tel, [(0.0, 0.0)], 620.0, nx=255)
    assert _against_model(m, tel, lambda h: h ** 4 / (4 * 20.0 ** 3) * 1e9) < 0.01
    X, Y = _grid(tel, 255)
    edge = np.isfinite(m) & (np.hypot(X, Y) > 0.45)
    assert (m[edge] > 0).all()                         # edge rays travel the shorter path: t_chief - t > 0


def test_asphere_below_the_photon_newton_threshold(torch_cuda):
    """a = 4e-8 r^4 on the paraboloid: at most 2.5 nm of sag, below the 1e-8 |G| at which the photon path's Newton stops
    without a step -- the OPD trace must resolve it: W = 2 a h^4 (~5 nm at the edge)"""
    tel = opd_numpy.one_mirror(asph=(4e-8,))
    (m, _), = opd.compute(tel, [(0.0, 0.0)], 620.0, nx=255)
    assert np.nanmax(m) > 4.0
    assert _against_model(m, tel, lambda h: 2 * 4e-8 * h ** 4 * 1e9) < 0.02


FIELDS = [(0.0, 0.0), (math.radians(0.5), math.radians(0.3)), (math.radians(1.2), math.radians(-0.8))]


@pytest.fixture(scope="module")
def rubin():
    return optics.rubin_like_telescope()


@pytest.mark.parametrize("nx", [64, 255])
@pytest.mark.parametrize("projection", ["postel", "zemax"])
@pytest.mark.parametrize("reference", ["chief", "mean"])
def test_against_numpy_restatement(torch_cuda, rubin, nx, projection, reference):
    wl = 622.0
    out = opd.compute(rubin, FIELDS, wl, nx=nx, projection=projection, reference=reference)
    X, Y = _grid(rubin, nx)
    for (thx, thy), (m, h) in zip(FIELDS, out):
        ref = opd_numpy.opd_map(rubin, thx, thy, wl, nx, projection=projection, reference=reference)
        f = np.isfinite(m)
        assert np.array_equal(f, np.isfinite(ref)) and f.sum() > 0.3 * nx * nx
        assert np.abs(m[f] - ref[f]).max() < 1e-3
        Z = opd.zernike_basis(28, X[f], Y[f], rubin.pupil_outer, 2.558 / 4.18)
        zk = np.linalg.lstsq(Z.T, m[f], rcond=None)[0]
        assert np.abs(_zk(h, 28) - zk).max() < 1e-6
        if reference == "mean":
            assert abs(np.nanmean(m)) < 1e-4
        assert (h["prjct"][0], h["sph_ref"][0], h["sph_rad"][0]) == (projection, reference, optics.RUBIN_LIKE_SPHERE_RADIUS)


def test_deterministic_and_independent_of_the_other_fields(torch_cuda, rubin):
    kw = dict(nx=96, reference="mean", jmax=36)
    a = opd.compute(rubin, FIELDS, 620.0, **kw)
    b = opd.compute(rubin, FIELDS, 620.0, **kw)
    for (ma, ha), (mb, hb) in zip(a, b):
        assert ma.tobytes() == mb.tobytes() and ha == hb
    for k, fld in enumerate(FIELDS):
        (m1, h1), = opd.compute(rubin, [fld], 620.0, **kw)
        assert m1.tobytes() == a[k][0].tobytes() and h1 == a[k][1]


def test_rot_tel_pos_traces_the_rotated_field_and_fits_the_unrotated_one(torch_cuda, rubin):
    rot = math.radians(30.0)
    fld = [FIELDS[2]]
    (m, h), = opd.compute(rubin, fld, 620.0, nx=96, rot_tel_pos=rot)
    r = opd.rotate_field(*fld[0], rot)
    (m_r, _), = opd.compute(rubin, [r], 620.0, nx=96)
    (_, h_u), = opd.compute(rubin, fld, 620.0, nx=96)
    assert m.tobytes() == m_r.tobytes()
    assert np.array_equal(_zk(h, 28), _zk(h_u, 28))
    assert (h["r_thx"][0], h["r_thy"][0]) == (math.degrees(r[0]), math.degrees(r[1]))
    assert (h["thx"][0], h["thy"][0]) == (math.degrees(fld[0][0]), math.degrees(fld[0][1]))


def _process(tmp_path, **opd_cfg):
    cfg = {"file_name": "opd.fits", "fields": [{"thx": "0.0 deg", "thy": "0.0 deg"}, {"thx": "1.121 deg", "thy": "-0.4 deg"}]}
    cfg.update(opd_cfg)
    o = {"input.instance_catalog.file_name": os.path.join(HERE, "golden", "example_instcat_subset.txt"),
         "image.nobjects": 3, "stamp.draw_method": "phot", "output.dir": str(tmp_path), "output.opd": cfg}
    return config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")],
                          overrides=o)


@pytest.mark.parametrize("nx", [255, 256])
def test_process_writes_the_opd_file(torch_cuda, tmp_path, nx):
    res = _process(tmp_path / "a", nx=nx)
    fn = str(tmp_path / "a" / "opd.fits")
    assert fn in res.files and "output.opd" not in res.ignored
    hdus = fits_io.read_fits(fn)
    assert len(hdus) == 2
    keys = [k.upper() for k in opd.HEADER_KEYS] + [f"AZ_{j:03d}" for j in range(1, 29)]
    dx = 2 * optics.Telescope([]).pupil_outer / nx          # the stand-in's pupil: the Telescope defaults
    for hdr, data in hdus:
        assert data.shape == (nx, nx) and data.dtype == np.float64
        assert all(k in hdr for k in keys)
        assert np.isnan(data[nx // 2, nx // 2]) and np.isfinite(data).sum() > 0.3 * nx * nx
        assert hdr["GS_SCALE"] == hdr["CD1_1"] == hdr["CD2_2"] == hdr["DX"] == dx
        assert hdr["CD1_2"] == hdr["CD2_1"] == 0.0
    assert abs(hdus[1][0]["THX"] - 1.121) < 1e-12 and hdus[1][0]["JMAX"] == 28 and hdus[0][0]["SPH_REF"] == "chief"
    if nx == 255:
        # the bandpass's effective wavelength is the default: giving it explicitly changes no bit
        wl, thr = tables.synthetic_r_band()
        wl_eff = tables.effective_wavelength(wl, thr)
        assert hdus[0][0]["WAVELEN"] == wl_eff
        _process(tmp_path / "b", nx=nx, wavelength=wl_eff)
        again = fits_io.read_fits(str(tmp_path / "b" / "opd.fits"))
        for (h1, d1), (h2, d2) in zip(hdus, again):
            assert d1.tobytes() == d2.tobytes()
            assert [h1[f"AZ_{j:03d}"] for j in range(1, 29)] == [h2[f"AZ_{j:03d}"] for j in range(1, 29)]
