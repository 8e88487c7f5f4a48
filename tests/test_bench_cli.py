"""bench.py's command line and --dump-outputs, without a GPU: a plain run is lean unless --full is given, and the dumped outputs
are float64, within 64 MB and the same sample from run to run."""
import os
import sys
import types

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_lean_and_full_is_opt_in(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_of_a_full_ccd_is_a_fixed_sample_within_64_mb(tmp_path):
    rng = np.random.default_rng(3)
    img = torch.from_numpy(rng.integers(0, 50, size=(4096, 4096)).astype(np.float64))
    step = types.SimpleNamespace()
    bench.dump_outputs(str(tmp_path / "a"), step, img, 0, 1, None)
    bench.dump_outputs(str(tmp_path / "b"), step, img, 0, 1, None)
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert set(a) == {"image_row_sums", "image_col_sums", "image_sample"}
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= 64_000_000
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k])
    full = img.numpy()
    assert np.array_equal(a["image_row_sums"], full.sum(axis=1)) and np.array_equal(a["image_col_sums"], full.sum(axis=0))
    assert a["image_sample"].size == bench.DUMP_SAMPLE and np.isin(a["image_sample"], full).all()


def test_dump_of_a_small_image_is_whole_and_of_a_focal_plane_is_by_ccd(tmp_path):
    img = torch.arange(64 * 48, dtype=torch.float64).reshape(48, 64)
    bench.dump_outputs(str(tmp_path / "s"), types.SimpleNamespace(), img, 0, 1, None)
    got = _files(tmp_path / "s")
    assert np.array_equal(got["image"], img.numpy())
    focal = types.SimpleNamespace(checksums={5: 2.5, 0: 1.0, 3: 7.0})
    bench.dump_outputs(str(tmp_path / "f"), focal, None, 0, 1, None)
    got = _files(tmp_path / "f")
    assert got["ccd_ids"].tolist() == [0.0, 3.0, 5.0] and got["ccd_checksums"].tolist() == [1.0, 7.0, 2.5]
    bench.dump_outputs(str(tmp_path / "r1"), types.SimpleNamespace(), img, 1, 2, None)       # only rank 0 writes
    assert not os.path.exists(tmp_path / "r1")
