"""Renderer.apply_ops against the independent reference of tests/photon_ops_ref.py, on the planted pools of
tests/photon_ops_cases.py.

ims_apply_ops picks its kernel from params->optics_layout alone: k_apply_ops<IMS_LAYOUT_PERTURBED> for an
ims_optics_perturbed_t, the loop over the surface descriptors for everything else, whatever IMS_LAYOUT_KERNELS says.  Every
case asserts which of the two it is by the descriptor's type and the layout the renderer uploads.  The third form of the
trace, unrolled for IMS_LAYOUT_RUBIN_LIKE inside the kernels specialised for the default chain (run_ops<1>), only runs on a
converted pool or in the rendering kernels, which shoot their own photons and take no planted pool.  Nothing here runs it.  It is
tied to this reference only through the tests that hold it bit for bit to the descriptor loops pinned here:
tests/test_photon_variant.py (every specialised kernel against the loops, converted pools),
tests/test_sensor_convert_gpu.py::test_converted_pool_matches_the_reference (the converted pool against the unconverted one) and
tests/test_parity_gpu.py::test_shoot_ops_photons_one_launch_equals_shoot_then_ops, which already states that
ims_shoot_ops_photons equals shoot_photons followed by apply_ops bit for bit -- so no such test is repeated here."""
import numpy as np
import pytest

import photon_ops_cases as cases
import photon_ops_ref as ref
from imsim_amd import _abi
from test_photon_variant import R

pytestmark = pytest.mark.gpu
P = _abi.IMS_LAYOUT_PERTURBED
RATIOS = {}
CASES = cases.all_cases()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def planted_pool(torch, r, case):
    from imsim_amd.engine import PhotonPool, _seg_ptr
    rows, obj_t, prefix, pre_t = r._upload_objects(case.objects)
    prm = r.bound.params(obj_t.data_ptr(), len(rows), pre_t.data_ptr(), int(prefix[-1]), r.image.data_ptr(), None, _seg_ptr(pre_t))
    offs = np.concatenate([[0], np.cumsum(rows["n_phot"])]).astype(np.int64)
    off_t = torch.from_numpy(offs).to(r.device)
    pool = PhotonPool(torch, r.device, offs[-1], off_t, obj_t, len(rows), pre_t, int(prefix[-1]))
    for f in ref.FIELDS:
        pool.t[f][:pool.n].copy_(torch.from_numpy(case.pool[f]))
    pool.obj_index[:pool.n].copy_(torch.from_numpy(case.obj_index()))
    return pool, prm


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_apply_ops_matches_the_reference(torch_cuda, case):
    from imsim_amd.engine import Renderer
    perturbed = isinstance(case.scene.optics, _abi.OpticsPerturbed)
    res = case.reference()
    r = Renderer(case.scene)
    pool, prm = planted_pool(torch_cuda, r, case)
    if case.scene.optics is not None:
        assert prm.optics_layout == (P if perturbed else R)          # what ims_apply_ops chooses its instantiation by
    r.apply_ops(pool)
    r.synchronize()
    got = pool.to_host()
    assert np.array_equal(got["obj_index"], case.obj_index())
    ref.assert_matches(res, got, case.name, ratios=RATIOS)
    print("worst so far:", {f: float(f"{v:.3g}") for f, v in RATIOS.items()})
