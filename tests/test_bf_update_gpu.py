"""The device's brighter-fatter boundary update (k_update_distortions, k_update_distortions_q3 in its table forms, k_refresh_changed)
against the exact scatter of tests/bf_update_ref.py, on the cases of tests/bf_update_cases.py, through the entry points a render
uses: Renderer(scene, lazy_static=False), the charge written into the renderer's delta array (or deposited by a real round), then
Renderer.update_distortions.  The assertions are the ones tests/test_bf_update.py holds the oracle to, plus the `changed` flags.

Forms (the library reports none of them; the host's rule -- bf_dl present, IMS_UPD_DPP, n_tiles <= IMS_UPD_DPP_MAX, and inside the
kernel gridDim.x <= 64 -- selects them, and the tile counts of the cases are asserted to fall where the rule is unambiguous):
IMS_UPD_DPP=1 with at most 64 tiles (DPP broadcasts, table fetched early), with 65 .. 128 tiles (fetched late: the 70 one-tile
regions), IMS_UPD_DPP=0 and IMS_UPD_DPP_MAX=0 (scalar loads from bf_dl), and the generic kernel by model (32 vertices per edge) and
by qdist (2 and 4).  The LDS-table form of the q3 kernel runs only for a sensor block without bf_dl; every renderer with qdist 3
uploads bf_dl (engine.BoundScene), so the public path cannot reach it and it is left out.

Out of scope: the joint-launch and tile-list forms (k_update_distortions_q3_j, k_update_list_j, k_refresh_list_j, k_build_active_j)
are driven only through ims_plans_run_joint, where the delta charge of a round cannot be observed; they stay tied to the per-CCD
chain by test_joint_top_chains_of_a_focal_plane_equal_a_chain_per_ccd, and this file anchors that chain.

measured (MI355X): worst |device - exact| / bound over every case, field and form: 0.575 (a ratio above 1 fails)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import bf_update_cases as cases
import bf_update_ref as ref
import test_bf_update as cpu
from test_bf_update import check_update

pytestmark = pytest.mark.gpu
RATIOS = {}
FORMS = {"dpp": {"IMS_UPD_DPP": "1"}, "scalar": {"IMS_UPD_DPP": "0"}, "dpp_max_0": {"IMS_UPD_DPP": "1", "IMS_UPD_DPP_MAX": "0"}}
RUNS = [(n, f) for n in cases.Q3_FAST for f in FORMS] + [(n, "dpp") for n in cases.GENERIC]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# the reference of a launch depends on the points before it and the charge alone: computed once, shared by the forms
_REFERENCES = {}
_update = ref.update


def _shared_update(m, qdist, nx, ny, points, delta):
    key = (m.name, qdist, nx, ny, hashlib.sha1(np.ascontiguousarray(points).tobytes()).hexdigest(),
           hashlib.sha1(np.ascontiguousarray(delta).tobytes()).hexdigest())
    if key not in _REFERENCES:
        _REFERENCES[key] = _update(m, qdist, nx, ny, points, delta)
    return _REFERENCES[key]


@pytest.fixture(autouse=True)
def shared_references(monkeypatch):
    monkeypatch.setattr(ref, "update", _shared_update)


def _host(t):
    return t.cpu().numpy().view(np.float64).copy()


def _renderer(monkeypatch, scene, env):
    from imsim_amd.engine import Renderer
    for k in ("IMS_UPD_DPP", "IMS_UPD_DPP_MAX"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = Renderer(scene, lazy_static=False)
    r.synchronize()
    return r


@pytest.mark.parametrize("name,form", RUNS, ids=[f"{n}-{f}" for n, f in RUNS])
def test_update_matches_the_reference(torch_cuda, monkeypatch, name, form):
    """every field of the case, one launch each on the same renderer: points within (T + 2) 2^-53 S of the reference applied to the
    points read before, untouched points bit for bit, `changed` the reference's flags on every owner cell, every bounds line the
    rectangles of the device's own points, delta all zero.  measured: worst error / bound 0.575"""
    c = cases.case(name)
    r = _renderer(monkeypatch, cases.scene(c), FORMS[form])
    assert bool(r.bound.sensor_host.bf_dl) == (c.qdist == 3), "bf_dl goes with qdist 3"
    n_tiles = cases.tiles(c)
    assert n_tiles <= 64 or (name == "many_regions_itl4" and 64 < n_tiles <= 128)
    arr = r.bound.sensor_arrays
    total = cases.offsets(c)[1]
    delta_t = arr["delta"].view(torch_cuda.float64)
    assert not _host(arr["delta"])[:total].any()
    for k, field in enumerate(c.fields):
        before = _host(arr["boundary"])
        d = cases.delta_of(c, field)
        delta_t[:total] = torch_cuda.from_numpy(d).to(delta_t.device)
        r.update_distortions(c.first_slot, c.n_slots, bf_tag=0)
        r.synchronize()
        res = check_update(c, d, before, _host(arr["boundary"]), _host(arr["bounds"]), _host(arr["delta"]), r._changed.cpu().numpy(),
                           f"{name} {form} field {k}", RATIOS)
        assert any(x.T.any() for x in res.values())
    print("worst so far:", {f: float(f"{v:.3g}") for f, v in RATIOS.items()})


def _tiles_in_reach(marks, slot, tag):
    """[tiles_y][tiles_x]: a tile_charge mark of the tile or of one of its eight neighbours carries the tag"""
    nx, ny, off = slot["nx"], slot["ny"], slot["offset"]
    m = marks[off:off + (nx + 1) * (ny + 1)].reshape(ny + 1, nx + 1)[::16, ::16] == tag
    p = np.pad(m, 1)
    return np.any([p[a:a + m.shape[0], b:b + m.shape[1]] for a in range(3) for b in range(3)], axis=0), m


@pytest.mark.parametrize("fold", [False, True], ids=["image_and_delta", "fold"])
def test_tagged_rounds_match_the_reference(torch_cuda, monkeypatch, fold):
    """two real rounds on one renderer: ims_accumulate deposits an object's charge with bf_tag = t and writes the tile marks, the test
    reads the delta array back and update_distortions(bf_tag = t) must give the reference applied to that charge -- round one in the
    last cells of tile (0, 0), moving points of the three tiles beyond its seams; round two with t + 1 elsewhere, over the stale
    marks and flags of round one.  The last tile column is out of reach in both.  fold: the deposits go to the delta image alone and
    the recalculation adds exactly the charge it consumes to the image."""
    c, scene = cases.round_case(2 if fold else 1)
    r = _renderer(monkeypatch, scene, FORMS["dpp"])
    arr = r.bound.sensor_arrays
    slot = cases.slots(c)[0]
    nx, ny = slot["nx"], slot["ny"]
    seen = []
    for k in range(2):
        tag = 7 + k
        pool = r.shoot_photons(cases.round_objects(k))
        r.accumulate(pool, bf_tag=tag)
        r.synchronize()
        before, d = _host(arr["boundary"]), _host(arr["delta"])
        image = r.image64_numpy().copy()
        reach, marked = _tiles_in_reach(arr["tile_charge"].cpu().numpy(), slot, tag)
        assert 3000 < d.sum() <= 6000 and marked.any() and not reach[:, -1].any() and not reach.all()
        r.update_distortions(0, 1, bf_tag=tag, fold=fold)
        r.synchronize()
        res = check_update(c, d, before, _host(arr["boundary"]), _host(arr["bounds"]), _host(arr["delta"]), None,
                           f"round {k} fold={fold}", RATIOS)[0]
        want = res.changed.reshape(ny + 1, nx + 1)
        got = ref.slot_cells(r._changed.cpu().numpy(), slot).reshape(ny + 1, nx + 1) != 0
        cell_reach = np.repeat(np.repeat(reach, 16, axis=0), 16, axis=1)[:ny + 1, :nx + 1]
        assert not (want & ~cell_reach).any(), "a tile the marks put out of reach holds a cell the charge reaches"
        assert np.array_equal(got[cell_reach], want[cell_reach]), "changed flags of the tiles the launch worked on"
        seen.append(want)
        if k == 0:
            assert marked[0, 0] and want[:, 16:32].any() and want[16:32, :].any(), "the reach crosses the seams of tile (0, 0)"
        if fold:
            gained = r.image64_numpy() - image
            assert np.array_equal(gained, d[:(nx + 1) * (ny + 1)].reshape(ny + 1, nx + 1)[:ny, :nx])
    assert (seen[0] & ~seen[1]).any() and (seen[1] & ~seen[0]).any(), "the two rounds move different tiles"
    print("worst so far:", {f: float(f"{v:.3g}") for f, v in RATIOS.items()})


def test_refusals(torch_cuda, monkeypatch):
    """qdist > 4, a qdist that reaches beyond the tabulated stamp and a null tile prefix are refused before anything is launched"""
    from imsim_amd import _abi
    c = cases.case("generic_e2v4_q2")
    r = _renderer(monkeypatch, cases.scene(c), {})
    prefix, prefix_t = r._tile_prefix(0)
    changed = torch_cuda.zeros(cases.offsets(c)[1], dtype=torch_cuda.uint8, device=r.device)
    before = _host(r.bound.sensor_arrays["boundary"])

    def call(host, pre):
        return r.lib.ims_sensor_update_distortions(r.bound.sensor_dev_ptr, C.byref(host), 0, 1, pre, int(prefix[1]), changed.data_ptr(), 0,
                                                   r._stream())
    far = _abi.Sensor.from_buffer_copy(bytes(r.bound.sensor_host))
    far.qdist = 5
    assert call(far, prefix_t.data_ptr()) != 0 and b"qdist" in r.lib.ims_last_error()
    small = _abi.Sensor.from_buffer_copy(bytes(r.bound.sensor_host))
    small.qdist, small.nx = 4, 7
    assert call(small, prefix_t.data_ptr()) != 0 and b"qdist" in r.lib.ims_last_error()
    assert call(r.bound.sensor_host, None) != 0
    r.synchronize()
    assert np.array_equal(_host(r.bound.sensor_arrays["boundary"]), before)
    with pytest.raises(AssertionError):
        ref.visits(cpu.model(c.model), 5)
