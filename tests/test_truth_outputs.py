"""The per-CCD catalog outputs (output.truth, output.photon_pooling_truth, output.process_info) and the host half of
cosmic-ray painting (output.cosmic_ray_rate): config parsing, file names, the text writer, column evaluation, and the
hit table of ims_paint_cosmic_rays restated in numpy against CosmicRays.paint.  No GPU."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from imsim_amd import _abi, config, cosmic_rays, truth
from imsim_amd.cosmic_rays import CosmicRays, write_cosmic_ray_catalog
from imsim_amd.lsst_image import GalSimConfigError

HERE = os.path.dirname(os.path.abspath(__file__))

# the columns of config/imsim-config.yaml:381-392 and imsim-config-photon-pooling.yaml:58-68
TEMPLATE_COLUMNS = {"object_id": "@object_id", "ra": "$sky_pos.ra.deg", "dec": "$sky_pos.dec.deg", "x": "$image_pos.x",
                    "y": "$image_pos.y", "nominal_flux": "@nominal_flux", "phot_flux": "@phot_flux", "fft_flux": "@fft_flux",
                    "realized_flux": "@realized_flux"}
CENTROID_NAME = {"type": "FormattedStr", "format": "centroid_%08d-%1d-%s-%s-det%03d.txt.gz",
                 "items": [{"type": "OpsimData", "field": "observationId"}, {"type": "OpsimData", "field": "snap"}, "$band",
                           "$det_name", "@output.det_num"]}


def _evaluator(det=94):
    cfg = config.load_config({"output": {"dir": "out", "det_num": {"type": "Sequence", "first": 94}, "truth": {}},
                              "_opsim_data": {"observationId": 961899, "snap": 0, "band": "r"}})
    ev = config.Evaluator(cfg)
    ev.vars.update(band="r", det_name=config.det_name_of(det), _sequence_index=det)
    return ev


def _empty_objects():
    tr = {k: np.zeros(0) for k in ("index", "x", "y", "nominal_flux", "phot_flux", "fft_flux", "realized_flux")}
    return truth.object_columns(tr, {"object_id": np.zeros(0, str)}, None)


def test_parse_switches_and_keys():
    assert truth.parse("", "truth") is None and truth.parse(None, "truth") is None
    assert truth.parse({"dir": "output"}, "truth") is None                   # no file_name: nothing to write (GalSim skips it)
    c = {"file_name": "t.txt", "columns": {"x": "$image_pos.x"}}
    assert truth.parse(c, "truth") is c
    with pytest.raises(GalSimConfigError, match="nope"):
        truth.parse({"file_name": "t.txt", "nope": 1}, "truth")
    with pytest.raises(GalSimConfigError, match="columns"):
        truth.parse({"file_name": "t.txt", "columns": ["x"]}, "truth")
    with pytest.raises(GalSimConfigError):
        truth.parse({"file_name": "p.txt", "columns": {}}, "process_info", truth.PROCESS_INFO_KEYS)


def test_file_name_is_evaluated_per_ccd():
    ev = _evaluator(94)
    c = {"dir": "output", "file_name": CENTROID_NAME}
    assert truth.file_name(c, ev, {"dir": "fits"}) == os.path.join("output", "centroid_00961899-0-r-R22_S11-det094.txt.gz")
    ev.vars.update(det_name=config.det_name_of(95), _sequence_index=95)
    assert truth.file_name({"file_name": CENTROID_NAME}, ev, {"dir": "fits"}) == os.path.join("fits", "centroid_00961899-0-r-R22_S12-det095.txt.gz")
    with pytest.raises(GalSimConfigError, match="text"):
        truth.file_name({"file_name": "truth.fits"}, ev, {})


def test_writer_round_trips_header_types_and_gzip(tmp_path):
    cols = {"object_id": np.array(["a1", "1234567890123"]), "n": np.array([3, -4]), "x": np.array([1.25, -2.0e-7]),
            "f": np.array([123456.789, 0.0])}
    for name in ("t.txt", "t.txt.gz"):
        fn = str(tmp_path / "sub" / name)
        truth.write(fn, cols)
        raw = (gzip.open(fn, "rt") if name.endswith(".gz") else open(fn)).read().splitlines()
        if name.endswith(".gz"):
            with open(fn, "rb") as f:
                assert f.read(2) == b"\x1f\x8b"
        # galsim.OutputCatalog.writeAscii: names centred in 16 columns, 16-wide fields, floats as %16.8e
        assert raw[0] == "# " + " ".join(f"{k:^16}" for k in cols) + " "
        assert raw[1] == " ".join(["%16s" % "a1", "%16d" % 3, "%16.8e" % 1.25, "%16.8e" % 123456.789])
        back = truth.read(fn)
        assert list(back) == list(cols)
        assert list(back["object_id"]) == ["a1", "1234567890123"] and back["n"].dtype == np.int64
        assert back["n"].tolist() == [3, -4] and back["x"].dtype == np.float64
        np.testing.assert_allclose(back["x"], cols["x"], rtol=1e-8)
        np.testing.assert_allclose(back["f"], cols["f"], rtol=1e-8)
    truth.write(str(tmp_path / "empty.txt"), {"object_id": np.zeros(0, str), "x": np.zeros(0)})
    assert truth.read(str(tmp_path / "empty.txt"))["x"].shape == (0,)


def test_columns_evaluate_as_whole_columns():
    objs = _empty_objects()
    ev = _evaluator()
    got = truth.evaluate_columns(dict(TEMPLATE_COLUMNS, det="$det_name", num="@output.det_num", twice="$2 * image_pos.x"), objs, ev)
    assert list(got)[:9] == list(TEMPLATE_COLUMNS) and all(len(v) == 0 for v in got.values())
    assert "image_pos" not in ev.vars                                       # the per-object names do not leak into the config
    for bad in ("@no_such_value", "$image_pos.z", "$undefined_name + 1", {"type": "Nope"}):
        with pytest.raises(GalSimConfigError, match="truth column bad"):
            truth.evaluate_columns({"bad": bad}, objs, ev)


def test_process_parses_catalogs_before_any_gpu_work():
    ev = _evaluator()
    cols = dict(TEMPLATE_COLUMNS)
    out = {"truth": {"file_name": "t.txt", "columns": cols}}
    assert [k for k, _ in config.parse_catalogs(out, ev, "LSST_Image")] == ["truth"]
    # LSST_PhotonPoolingImage has incident_flux, not realized_flux (imsim-config-photon-pooling.yaml:58-68)
    with pytest.raises(GalSimConfigError, match="realized_flux"):
        config.parse_catalogs(out, ev, "LSST_PhotonPoolingImage")
    pool_cols = dict(cols, incident_flux="@incident_flux")
    del pool_cols["realized_flux"]
    pool = {"truth": "", "photon_pooling_truth": {"file_name": "t.txt", "columns": pool_cols}, "process_info": {"file_name": "p.txt"}}
    assert [k for k, _ in config.parse_catalogs(pool, ev, "LSST_PhotonPoolingImage")] == ["photon_pooling_truth", "process_info"]
    assert config.parse_catalogs({"truth": "", "photon_pooling_truth": ""}, ev, "LSST_Image") == []
    with pytest.raises(GalSimConfigError, match="columns"):
        config.parse_catalogs({"truth": {"file_name": "t.txt"}}, ev, "LSST_Image")
    with pytest.raises(GalSimConfigError, match="no_such"):
        config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")],
                       overrides={"input.instance_catalog.file_name": os.path.join(HERE, "golden", "example_instcat_subset.txt"),
                                  "output.truth": {"file_name": "t.txt", "columns": {"no_such": "@no_such"}}}, device="cpu")


def test_process_info_columns():
    cols = truth.process_info_columns(np.array(["a", "b"]))
    assert tuple(cols) == truth.PROCESS_INFO_COLUMNS
    assert cols["pid"].tolist() == [os.getpid()] * 2 and cols["rss"][0] > 0 and cols["uss"][0] > 0
    assert cols["rss"][0] == cols["rss"][1] and cols["user_time"][0] > 0


def test_cosmic_ray_catalog_and_rate(tmp_path):
    ev = _evaluator()
    assert config.parse_cosmic_rays({}, ev, None) is None and config.parse_cosmic_rays({"cosmic_ray_rate": 0}, ev, None) is None
    crs = config.parse_cosmic_rays({"cosmic_ray_rate": 0.2}, ev, None)
    assert crs.ccd_rate == 0.2 and len(crs) > 1000                         # the packaged catalog
    assert cosmic_rays.find_catalog(None, None) == cosmic_rays.DEFAULT_CATALOG
    own = _small_catalog(tmp_path)
    assert cosmic_rays.find_catalog(os.path.basename(own), str(tmp_path)) == os.path.join(str(tmp_path), os.path.basename(own))
    assert len(config.parse_cosmic_rays({"cosmic_ray_rate": 1.0, "cosmic_ray_catalog": own}, ev, None)) == 4
    with pytest.raises(FileNotFoundError):
        config.parse_cosmic_rays({"cosmic_ray_rate": 0.2, "cosmic_ray_catalog": str(tmp_path / "none.fits")}, ev, str(tmp_path))
    with pytest.raises(GalSimConfigError):
        config.parse_cosmic_rays({"cosmic_ray_rate": -1.0}, ev, None)


def _small_catalog(tmp_path):
    """four footprints; fp 3 covers pixel (row 0, col 1) twice (two spans of one row that overlap)"""
    fn = str(tmp_path / "cr_small.fits")
    write_cosmic_ray_catalog((0, 0, 0, 1, 2, 2, 3, 3), (10, 10, 10, 0, 5, 4, 7, 8), (20, 21, 22, 100, 40, 41, 9, 9),
                             [[0, 10, 0], [20, 30, 20], [0, 40, 0], [100], [7, 8, 9, 10], [11, 12], [1, 2, 3], [4, 5]],
                             1.0, 100, outfile=fn)
    return fn


def paint_numpy(crs, image, hits):
    """ims_paint_cosmic_rays restated: the hit table's layers in turn, each hit's span pixels added where they fall"""
    t = crs.device_tables("cpu")
    table, layer_first = crs.hit_table(hits, "cpu")
    ny, nx = image.shape
    vals = t["values_dev"].numpy()
    for layer in range(len(layer_first) - 1):
        touched = set()
        for h in table[layer_first[layer]:layer_first[layer + 1]]:
            base = t["spans"][h["first_span"]]["first_pixel"]
            seen = 0
            for s in t["spans"][h["first_span"]:h["first_span"] + h["n_spans"]]:
                assert s["first_pixel"] - base == seen
                seen += s["n"]
                for dx in range(s["n"]):
                    row, col = h["y0"] + s["row"], h["x0"] + s["col"] + dx
                    if 0 <= row < ny and 0 <= col < nx:
                        assert (row, col) not in touched             # a layer's hits are disjoint
                        touched.add((row, col))
                        image[row, col] += vals[s["value_offset"] + dx]
            assert seen == h["n_pixels"]
    return image


@pytest.mark.parametrize("shape, num_crs", [((40, 30), 300), ((300, 200), 1500)])
def test_hit_table_restated_equals_paint(tmp_path, shape, num_crs):
    """the layering keeps every pixel's adds in draw order: bit-identical to CosmicRays.paint on a non-integer image"""
    for crs in (CosmicRays.read_catalog(_small_catalog(tmp_path), ccd_rate=5000.0), CosmicRays(ccd_rate=20.0)):
        base = np.random.default_rng(3).uniform(0.0, 1.0e3, shape) + 0.1
        want = crs.paint(base.copy(), np.random.default_rng(11), exptime=30.0, num_crs=num_crs)
        hits = crs.draw(shape, np.random.default_rng(11), exptime=30.0, num_crs=num_crs)
        got = paint_numpy(crs, base.copy(), hits)
        assert len(hits) > 20 and not np.array_equal(want, base)
        assert np.array_equal(got, want)
    table, layer_first = crs.hit_table(hits, "cpu")
    assert layer_first[0] == 0 and layer_first[-1] == len(table) and np.all(np.diff(layer_first) > 0)


def test_hit_layers_order_overlaps():
    # boxes [r0, r1) x [c0, c1): 0 and 2 overlap, 1 is apart, 3 overlaps 2
    r0, r1 = np.array([0, 10, 1, 2]), np.array([3, 12, 4, 6])
    c0, c1 = np.array([0, 10, 1, 2]), np.array([3, 12, 4, 6])
    assert cosmic_rays.hit_layers(r0, r1, c0, c1).tolist() == [0, 0, 1, 2]
    assert cosmic_rays.hit_layers(r0[:0], r1[:0], c0[:0], c1[:0]).tolist() == []


def test_ccd_rng_is_per_ccd_and_apart_from_the_flux_stream():
    a, b = cosmic_rays.ccd_rng(7).random(4), cosmic_rays.ccd_rng(7).random(4)
    assert np.array_equal(a, b) and not np.array_equal(a, cosmic_rays.ccd_rng(8).random(4))
    assert not np.array_equal(a, np.random.default_rng([7, 0x5151]).random(4))


def test_paint_entry_point_is_exported_and_checks_arguments():
    lib = _abi.load()
    assert "ims_paint_cosmic_rays" in _abi.EXPORTS and lib.ims_abi_version() == 22
    assert lib.ims_struct_size(_abi.CR_SPAN_STRUCT_INDEX) == C.sizeof(_abi.CrSpan) == _abi.CR_SPAN_DTYPE.itemsize == 24
    assert lib.ims_struct_size(_abi.CR_HIT_STRUCT_INDEX) == C.sizeof(_abi.CrHit) == _abi.CR_HIT_DTYPE.itemsize == 24
    assert _abi.CrSpan not in _abi.STRUCTS and _abi.CrHit not in _abi.STRUCTS
    # nothing to paint, and refusals -- all decided on the host, before any launch
    assert lib.ims_paint_cosmic_rays(None, 4, 4, None, 0, None, 0, None, None, 0, None) == 0
    lf = (C.c_int64 * 2)(0, 0)
    assert lib.ims_paint_cosmic_rays(None, 4, 4, None, 0, None, 0, None, lf, 1, None) == 0
    lf = (C.c_int64 * 2)(0, 3)
    assert lib.ims_paint_cosmic_rays(None, 4, 4, None, 1, None, 1, None, lf, 1, None) != 0 and b"NULL" in lib.ims_last_error()
    assert lib.ims_paint_cosmic_rays(None, 4, 4, None, 0, None, 0, None, None, 1, None) != 0
    assert lib.ims_paint_cosmic_rays(None, 4, 4, None, 0, None, 0, None, None, -1, None) != 0
