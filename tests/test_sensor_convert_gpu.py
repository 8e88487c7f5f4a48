"""The device's photon conversion (land_convert, through the converted pool of ims_shoot_ops_photons and through the fused
launch) and its initial tree-ring state (k_init_boundaries, k_init_tiles) against the independent reference of
tests/sensor_convert_ref.py, on the cases of tests/sensor_convert_cases.py.  The assertions are the ones tests/test_sensor_convert.py
holds the oracle to."""
import numpy as np
import pytest

import sensor_convert_cases as cases
import sensor_convert_ref as ref
from test_photon_variant import R, query
from test_sensor_convert import assert_exercised, check_initial_state, search_pixels

pytestmark = pytest.mark.gpu
CONVERT, RINGS = cases.CONVERT_NAMES, cases.RING_NAMES
RATIOS = {}
# the default chain runs in the kernel specialised for it, and in the descriptor-driven one with the switches off
RUNS = [(n, "1") for n in CONVERT] + [(n, "0") for n in cases.DEFAULT_CHAIN_NAMES[:2]]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _variant(r, objects, mode):
    from imsim_amd.engine import _seg_ptr
    rows, obj_t, prefix, pre_t = r._upload_objects(objects)
    prm = r.bound.params(obj_t.data_ptr(), len(rows), pre_t.data_ptr(), int(prefix[-1]), r.image.data_ptr(), None, _seg_ptr(pre_t))
    return query(r.lib, prm, mode)


def _renderer(monkeypatch, case, switch):
    from imsim_amd.engine import Renderer
    monkeypatch.setenv("IMS_CHAIN_KERNELS", switch)
    monkeypatch.setenv("IMS_LAYOUT_KERNELS", switch)
    r = Renderer(case.scene, lazy_static=False)
    want = (1, 1, R) if case.default_chain and switch == "1" else (0, 0, 0)
    assert _variant(r, case.objects, 2) == want
    return r


@pytest.mark.parametrize("name,switch", RUNS, ids=[f"{n}-switches_{'on' if s == '1' else 'off'}" for n, s in RUNS])
def test_converted_pool_matches_the_reference(torch_cuda, monkeypatch, name, switch):
    case = cases.convert_case(name)
    r = _renderer(monkeypatch, case, switch)
    pool = r.shoot_ops_photons(case.objects).to_host()
    got = r.shoot_ops_photons(case.objects, converted=True).to_host()
    r.synchronize()
    assert np.array_equal(pool["obj_index"], np.repeat(np.arange(len(case.objects)), case.objects["n_phot"]))
    conv = ref.convert_pool(case.ref_sensor(), case.scene.seed, case.objects, pool, case.has_angles)
    assert_exercised(case, conv)
    ref.assert_matches(conv, got, pool["flux"], f"{case.name} ({switch})", RATIOS)
    print("worst so far:", {f: float(f"{v:.3g}") for f, v in RATIOS.items()})


@pytest.mark.parametrize("name", [CONVERT[0], CONVERT[3]])
def test_fused_image_is_the_reference_conversion_and_search(torch_cuda, monkeypatch, name):
    """k_shoot_accumulate: the image equals np.add.at of the reference's conversion of the device's un-converted pool, searched by
    shapes_ref.pixel_search over the device's boundary array -- pixel by pixel, except the pixels an ambiguous photon could touch"""
    case = cases.convert_case(name)
    r = _renderer(monkeypatch, case, "1")
    pool = r.shoot_ops_photons(case.objects).to_host()
    r.render(case.objects)
    r.synchronize()
    conv = ref.convert_pool(case.ref_sensor(), case.scene.seed, case.objects, pool, case.has_angles)
    boundary = r.bound.sensor_arrays["boundary"].cpu().numpy().view(np.float64)
    want, amb = search_pixels(case, conv, boundary, pool["obj_index"], pool["flux"])
    assert amb.sum() <= ref.EDGE_SHARE_CAP * len(want)
    sc = case.scene
    img = np.zeros(sc.nx * sc.ny)
    on = want >= 0
    np.add.at(img, want[on], pool["flux"][on])
    got = r.image64_numpy().ravel()
    skip = np.zeros(sc.nx * sc.ny, dtype=bool)
    for k in np.flatnonzero(amb):                                # an ambiguous photon: its pixel and the eight around it
        c = int(np.floor(float(conv.y0[k]) + 0.5) - sc.ymin) * sc.nx + int(np.floor(float(conv.x0[k]) + 0.5) - sc.xmin)
        for d in (-sc.nx - 1, -sc.nx, -sc.nx + 1, -1, 0, 1, sc.nx - 1, sc.nx, sc.nx + 1):
            if 0 <= c + d < skip.size:
                skip[c + d] = True
    assert img.sum() > 1000 and skip.sum() <= 9 * amb.sum()
    bad = (got != img) & ~skip
    assert not bad.any(), f"{case.name}: {int(bad.sum())} pixels differ, first {np.flatnonzero(bad)[:5]}: device {got[bad][:5]} reference {img[bad][:5]}"


@pytest.mark.parametrize("tiles", ["1", "0"])
@pytest.mark.parametrize("name", RINGS)
def test_initial_state_matches_the_reference(torch_cuda, monkeypatch, name, tiles):
    """slot 0 and the private regions as the renderer makes them, with the tiled kernel (4 vertices per edge only) and the
    per-cell one: every owned point of every owner cell, the last row and column included, within the bound; the bounds lines
    exactly the rectangles of the device's own points; no point displaced by more than pristine_margin; no delta charge"""
    from imsim_amd.engine import Renderer
    case = cases.ring_case(name)
    monkeypatch.setenv("IMS_INIT_TILES", tiles)
    r = Renderer(case.scene, lazy_static=False)
    r.synchronize()
    arrays = {name: r.bound.sensor_arrays[name].cpu().numpy().view(np.float64) for name in ("boundary", "bounds", "delta")}
    moved = check_initial_state(case, arrays["boundary"], arrays["bounds"], f"{case.name} tiles={tiles}", RATIOS)
    margin = r.bound.sensor_struct.pristine_margin
    assert 0.0 <= moved <= margin < 0.5
    assert not arrays["delta"][:case.scene.sensor.total_cells()].any()
    print("worst so far:", {f: float(f"{v:.3g}") for f, v in RATIOS.items()})
