"""Cosmic rays painted on the GPU (ims_paint_cosmic_rays) and the per-CCD catalogs written by config.Process: the kernel
against CosmicRays.paint bit for bit, the centroid files against the truth record, cosmic rays in a run (e-image and
readout), and the overlapped focal plane against CCDs rendered one after the other."""
import os

import numpy as np
import pytest

from imsim_amd import config, cosmic_rays, instcat, truth, wcs as wcsmod
from imsim_amd.cosmic_rays import CosmicRays, write_cosmic_ray_catalog

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CATALOG = os.path.join(HERE, "golden", "example_instcat_subset.txt")
KEYS = ("truth", "photon_pooling_truth", "process_info", "cosmic_ray_rate")
COLUMNS = {"object_id": "@object_id", "ra": "$sky_pos.ra.deg", "dec": "$sky_pos.dec.deg", "x": "$image_pos.x", "y": "$image_pos.y",
           "nominal_flux": "@nominal_flux", "phot_flux": "@phot_flux", "fft_flux": "@fft_flux"}
NAME = {"type": "FormattedStr", "format": "centroid_%08d-%1d-%s-%s-det%03d.txt.gz",
        "items": [{"type": "OpsimData", "field": "observationId"}, {"type": "OpsimData", "field": "snap"}, "$band", "$det_name",
                  "@output.det_num"]}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _process(**over):
    o = {"input.instance_catalog.file_name": CATALOG}
    o.update(over)
    return config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")], overrides=o)


def _paint_both(torch, crs, base, seed, num_crs=None, exptime=30.0):
    want = crs.paint(base.copy(), np.random.default_rng(seed), exptime=exptime, num_crs=num_crs)
    dev = torch.from_numpy(base.copy()).to("cuda:0")
    hits = crs.paint_hip(dev, np.random.default_rng(seed), exptime=exptime, num_crs=num_crs)
    torch.cuda.synchronize()
    return want, dev.cpu().numpy(), hits


def test_paint_equals_numpy_small_with_edges_and_overlaps(torch_cuda, tmp_path):
    """a 40 x 30 image with thousands of hits: footprints hang over every edge and pile up on each other (tens of layers), and
    one footprint covers a pixel twice; the image is not integer-valued, so only the numpy order gives these bits"""
    fn = str(tmp_path / "cr.fits")
    write_cosmic_ray_catalog((0, 0, 0, 1, 2, 2, 3, 3), (10, 10, 10, 0, 5, 4, 7, 8), (20, 21, 22, 100, 40, 41, 9, 9),
                             [[0, 10, 0], [20, 30, 20], [0, 40, 0], [100], [7, 8, 9, 10], [11, 12], [1, 2, 3], [4, 5]],
                             1.0, 100, outfile=fn)
    for crs in (CosmicRays.read_catalog(fn, ccd_rate=1.0), CosmicRays(ccd_rate=1.0)):
        base = np.random.default_rng(1).uniform(0.0, 1.0e4, (40, 30)) + 1.0 / 3.0
        want, got, hits = _paint_both(torch_cuda, crs, base, 5, num_crs=2000)
        table, layer_first = crs.hit_table(hits, "cuda:0")
        assert len(layer_first) > 10 and not np.array_equal(want, base)
        assert np.array_equal(got, want)


def test_paint_equals_numpy_on_a_4k_ccd(torch_cuda):
    """a 4004 x 4096 CCD: the Poisson count of a 30 s exposure at imSim's rate, and a dense 5000-hit draw"""
    crs = CosmicRays(ccd_rate=0.2)
    base = np.random.default_rng(2).poisson(800.0, (4004, 4096)).astype(np.float64) + 0.25
    for num_crs, seed in ((None, 7), (5000, 8)):
        want, got, hits = _paint_both(torch_cuda, crs, base, seed, num_crs=num_crs)
        assert len(hits) > (1 if num_crs is None else 4999)
        assert np.array_equal(got, want)
        edge = (hits[:, 1] > 4090) | (hits[:, 2] > 3998)
        if num_crs:
            assert edge.any()
    # no hits: the image is untouched
    want, got, hits = _paint_both(torch_cuda, crs, base, 9, num_crs=0)
    assert len(hits) == 0 and np.array_equal(got, base)


def _check_file_against_truth(fn, t, img_wcs, flux_keys):
    rows = truth.read(fn)
    assert list(rows["object_id"]) == [str(s) for s in t["object_id"]]
    assert len(rows["x"]) == len(t["x"]) > 0
    for k in ("x", "y") + flux_keys:
        np.testing.assert_allclose(rows[k], np.asarray(t[k], dtype=np.float64), rtol=2e-8, atol=1e-300, err_msg=k)
    vec = wcsmod.unit_vector(np.radians(rows["ra"]), np.radians(rows["dec"])).T
    x, y = wcsmod.tansip_vec_to_pix(img_wcs, vec)
    assert np.abs(x - t["x"]).max() < 1e-3 and np.abs(y - t["y"]).max() < 1e-3


def test_centroid_file_rows_equal_the_truth_record(torch_cuda, tmp_path, monkeypatch):
    """output.truth in the template's form: one row per drawn object (FFT and faint ones included), gzip, in res.files"""
    wcs_seen = []
    orig = config.opticsmod.build_wcs_pair
    monkeypatch.setattr(config.opticsmod, "build_wcs_pair", lambda *a, **k: wcs_seen.append(orig(*a, **k)) or wcs_seen[-1])
    res = _process(**{"image.nobjects": 40, "stamp.fft_sb_thresh": 2.0e3, "output.dir": str(tmp_path),
                      "output.truth": {"dir": str(tmp_path / "truth"), "file_name": NAME,
                                       "columns": dict(COLUMNS, realized_flux="@realized_flux")},
                      "output.process_info": {"file_name": "process_info.txt"}})
    t = res.truth[0]
    assert not any(s.startswith("output." + k) for k in KEYS for s in res.ignored)
    fn = str(tmp_path / "truth" / "centroid_00398414-0-r-R22_S11-det094.txt.gz")
    assert fn in res.files and os.path.isfile(fn)
    assert {"fft", "phot"} <= set(t["mode"])
    _check_file_against_truth(fn, t, wcs_seen[-1][0], ("nominal_flux", "phot_flux", "fft_flux", "realized_flux"))
    info = truth.read(str(tmp_path / "process_info.txt"))
    assert list(info) == list(truth.PROCESS_INFO_COLUMNS) and list(info["object_id"]) == [str(s) for s in t["object_id"]]
    assert set(info["pid"].tolist()) == {os.getpid()} and len(set(info["rss"].tolist())) == 1


def test_photon_pooling_truth(torch_cuda, tmp_path, monkeypatch):
    """LSST_PhotonPoolingImage: output.truth "" (as the pooling template sets it) writes nothing, photon_pooling_truth writes
    the incident fluxes"""
    wcs_seen = []
    orig = config.opticsmod.build_wcs_pair
    monkeypatch.setattr(config.opticsmod, "build_wcs_pair", lambda *a, **k: wcs_seen.append(orig(*a, **k)) or wcs_seen[-1])
    res = _process(**{"image.nobjects": 30, "image.type": "LSST_PhotonPoolingImage", "stamp.type": "LSST_Photons", "image.nbatch": 4,
                      "image.nsubbatch": 3, "input.checkpoint": "", "output.dir": str(tmp_path), "output.truth": "",
                      "output.photon_pooling_truth": {"file_name": "pool_%s.txt" % "centroid",
                                                      "columns": dict(COLUMNS, incident_flux="@incident_flux")}})
    assert not any(s.startswith("output." + k) for k in KEYS for s in res.ignored)
    fn = os.path.join(str(tmp_path), "pool_centroid.txt")
    assert res.files == [fn]
    _check_file_against_truth(fn, res.truth[0], wcs_seen[-1][0], ("nominal_flux", "phot_flux", "fft_flux", "incident_flux"))


def _ccd_seed(det=94):
    return config.ccd_seed(int(instcat.read_header(CATALOG)["seed"]), det)


def test_cosmic_rays_in_a_run(torch_cuda):
    """cosmic_ray_rate > 0: the e-image is the one without them plus exactly the footprints CosmicRays.paint lays down with the
    CCD's stream, and the readout sees them; rate 0 leaves the image as it is without the key"""
    common = {"image.nobjects": 5, "stamp.draw_method": "phot"}
    exptime = float(instcat.read_header(CATALOG)["exptime"])
    a = _process(**common)
    b = _process(**common, **{"output.cosmic_ray_rate": 0.5})
    assert not any(s.startswith("output.cosmic_ray") for s in b.ignored)
    base = a.eimages[0].array.cpu().numpy()
    want = CosmicRays(ccd_rate=0.5).paint(base.copy(), cosmic_rays.ccd_rng(_ccd_seed()), exptime=exptime)
    got = b.eimages[0].array.cpu().numpy()
    assert (want != base).sum() > 50
    assert np.array_equal(got, want)
    assert np.array_equal(b.images[0], got.astype(np.float32))
    ro = {"readout_time": 3.0, "dark_current": 0.0, "bias_level": 1000.0, "scti": 0.0, "pcti": 0.0, "read_noise": 0.0}
    c = _process(**common, **{"output.cosmic_ray_rate": 0.0, "output.readout": ro})
    d = _process(**common, **{"output.cosmic_ray_rate": 0.5, "output.readout": ro})
    assert np.array_equal(c.images[0], a.images[0])
    assert np.array_equal(d.images[0], b.images[0])
    raw_c = np.concatenate([np.asarray(h[1], dtype=np.float64).ravel() for h in c.raw[0][1:]])
    raw_d = np.concatenate([np.asarray(h[1], dtype=np.float64).ravel() for h in d.raw[0][1:]])
    assert (raw_d - raw_c).sum() > 0.25 * (want - base).sum()                # gains of ~1-2 e- per ADU
    assert (raw_d != raw_c).sum() >= 0.5 * (want != base).sum()


def test_focal_plane_overlapped_equals_one_ccd_at_a_time(torch_cuda, tmp_path, monkeypatch):
    over = {"image.nobjects": 20, "output.nfiles": 2, "stamp.draw_method": "phot", "output.cosmic_ray_rate": 0.5,
            "output.truth": {"file_name": {"type": "FormattedStr", "format": "centroid_%s.txt", "items": ["$det_name"]},
                             "columns": dict(COLUMNS, realized_flux="@realized_flux")}}
    a = _process(**over, **{"output.dir": str(tmp_path / "a")})
    monkeypatch.setenv("IMS_PROCESS_FOCAL", "0")
    b = _process(**over, **{"output.dir": str(tmp_path / "b")})
    assert a.det_names == b.det_names and len(a.images) == 2 and len(a.files) == 2
    for k in range(2):
        assert np.array_equal(a.images[k], b.images[k]), a.det_names[k]
        with open(a.files[k], "rb") as fa, open(b.files[k], "rb") as fb:
            assert fa.read() == fb.read()
    assert not np.array_equal(a.images[0], a.images[1])
