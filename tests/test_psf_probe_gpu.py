"""The launch base the four PSF probes share (psf_probe.FieldPointLaunch) on the GPU: one table of rows through every Prepared
class on one renderer.  Every probe has to account for every photon of every row, and the probes that see the same photons have to
lose the same ones; nothing here has a tolerance.  What each probe computes from its photons is held to its own reference in
tests/test_psf_map_gpu.py, test_psf_adaptive_gpu.py, test_psf_profile_gpu.py and test_psf_image_gpu.py."""
import numpy as np
import pytest

from imsim_amd import config, configs, psf_image, psf_map, psf_profile

pytestmark = pytest.mark.gpu
R_EDGES = [0.0, 0.5, 2.0, 8.0]
SIZE, SCALE = (9, 6), 0.5


@pytest.fixture(scope="module")
def launch_table():
    """(renderer, rows): the renderer that keeps the sensor serves every stage of every probe; three field points with no photon,
    one photon, and one photon more than a segment holds"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    scene = configs.scene_c3(nx=64, ny=64, sensor=True)
    r = psf_image.renderer_for(scene, "sensor")
    rows = psf_map.point_rows(scene, np.array([[10.0, 20.0], [50.5, 40.25], [32.0, 7.5]]), (0, 1, scene.seg_size + 1), "ops")
    return r, rows


def prepared(r, rows):
    """every launch class on the rows: name -> a Prepared object, not yet run"""
    return {"moments": psf_map.Prepared(r, rows, "ops"),
            "profile": psf_profile.Prepared(r, rows, "ops", R_EDGES, n_phi=4),
            "image_ops": psf_image.Prepared(r, rows, "ops", SIZE, SCALE),
            "image_sensor": psf_image.Prepared(r, rows, "sensor", SIZE, SCALE)}


def test_every_probe_accounts_for_every_photon(launch_table):
    r, rows = launch_table
    n_phot = rows["n_phot"]
    assert n_phot.tolist() == [0, 1, r.scene.seg_size + 1]
    runs = prepared(r, rows)
    for run in runs.values():
        run()
    m, p, i_ops, i_sensor = (runs[k].result() for k in ("moments", "profile", "image_ops", "image_sensor"))
    assert np.array_equal(m["n_used"] + m["n_dropped"], n_phot)
    assert p.counts.shape == (3, len(R_EDGES) + 1, 5) and np.array_equal(p.counts.sum(axis=(1, 2)) + p.n_dropped, n_phot)
    assert np.array_equal(p.n_used, p.counts.sum(axis=(1, 2)))
    for im in (i_ops, i_sensor):
        assert im.counts.shape == (3, SIZE[1], SIZE[0]) and np.array_equal(im.n_used + im.n_outside + im.n_dropped, n_phot)
        assert np.array_equal(im.n_used, im.counts.sum(axis=(1, 2)))
    # stage ops: the same photons in all three reductions
    assert np.array_equal(m["n_dropped"], p.n_dropped) and np.array_equal(m["n_dropped"], i_ops.n_dropped)
    assert np.array_equal(m["n_used"], p.n_used)
    # the adaptive moments, started as psf_map.adaptive starts them, with a width that lets the single photon's row run
    state, status = psf_map.adaptive_start(m, guess_sigma=1.0)
    assert status[0] == psf_map.EMPTY and status[2] == psf_map.RUNNING
    aux = np.stack([np.full(3, np.nan), m["flux"], m["n_used"].astype(np.float64), m["n_dropped"].astype(np.float64)], axis=1)
    ad = psf_map.PreparedAdaptive(r, rows, "ops", state, status, aux, max_iter=2)
    ad()
    _, _, aux_out = ad.raw()
    assert np.array_equal(aux_out[:, 2] + aux_out[:, 3], n_phot.astype(np.float64)) and ad.done >= 1
    a = ad.result()
    assert np.array_equal(a["n_used"], m["n_used"]) and np.array_equal(a["n_dropped"], m["n_dropped"])
    # one upload, one set of render parameters: every class addresses the same table
    for run in list(runs.values()) + [ad]:
        assert (run.params.n_objects, run.params.n_segments) == (3, 3) and (run.n, run.n_segments, run.photons) == (3, 3, int(n_phot.sum()))


def test_a_launch_without_rows_returns_empty_results(launch_table):
    r, rows = launch_table
    none = rows[:0]
    runs = prepared(r, none)
    for run in runs.values():
        assert (run.n, run.n_segments, run.photons, run.params.n_objects, run.params.n_segments) == (0, 0, 0, 0, 0)
        run()
    assert runs["moments"].result().shape == (0,)
    p = runs["profile"].result()
    assert p.counts.shape == (0, len(R_EDGES) + 1, 5) and p.n_used.shape == p.n_dropped.shape == (0,)
    for k in ("image_ops", "image_sensor"):
        im = runs[k].result()
        assert im.counts.shape == (0, SIZE[1], SIZE[0]) and im.n_used.shape == im.n_outside.shape == im.n_dropped.shape == (0,)
    ad = psf_map.PreparedAdaptive(r, none, "ops", np.zeros((0, 5)), np.zeros(0, dtype=np.int32))
    ad()
    assert ad.done == 0                                      # nothing is running: no round is enqueued
    ad.rounds(1)                                             # the entry point itself takes an empty table
    assert ad.result().shape == (0,) and ad.result().dtype == psf_map.ADAPTIVE_DTYPE


def test_a_flat_lists_the_five_extra_outputs_as_ignored(launch_table, tmp_path):
    """a flat has no telescope to trace and no PSF: the keys are named in res.ignored, in this order, and nothing is written"""
    names = ("opd", "sag", "psf_map", "psf_profile", "psf_image")
    flat = config.Process({"image": {"type": "LSST_Flat", "random_seed": 1234, "xsize": 64, "ysize": 48, "counts_per_pixel": 100,
                                     "max_counts_per_iter": 100},
                           "output": {k: {"file_name": str(tmp_path / f"{k}.fits")} for k in reversed(names)}})
    assert [s for s in flat.ignored if s.startswith("output.")] == [f"output.{k}" for k in names]
    assert not any(tmp_path.iterdir())
