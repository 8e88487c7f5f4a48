"""Renderer.shoot_photons against the independent reference of tests/photon_source_ref.py, on the cases of
tests/photon_source_cases.py; the kick array of the phase-screen pre-pass against the reference's gradients.

Every case asserts which kernel form it ran: ims_photon_kernel_variant on the very parameter block (ims_shoot_photons is
mode 0: the kernels that loop over the descriptors, whatever the PSF list), whether the 2 x 2 cell table was built
(screen_quads), whether the pre-pass was taken.  The kernels specialised for a PSF list run only in mode 2, whose photons have
been through the operator chain and the sensor's conversion; the last test holds those (Kolmogorov + Gaussian: variant 1; six
screens, second kick, Gaussian: variant 2 with the batched gathers) bit for bit to the descriptor-driven kernels on the same small
screens and large field angles, which the first test pins to the reference."""
import ctypes as C

import numpy as np
import pytest

import photon_source_cases as cases
import photon_source_ref as ref
from imsim_amd import _abi
from test_photon_variant import R, query

pytestmark = pytest.mark.gpu
CASES = cases.all_cases()
RATIOS = {}


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


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_shoot_photons_matches_the_reference(torch_cuda, monkeypatch, case):
    from imsim_amd.engine import Renderer
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    shot = ref.shoot(case.source(), case.objects)
    r = Renderer(case.scene)
    assert _variant(r, case.objects, 0) == (0, 0, 0)
    if case.scene.atm is not None:
        assert (r.bound.atm_struct.screen_quads is not None) == (case.env["IMS_SCREEN_QUADS"] == "1")
    objects, run, kick = case.objects, None, None
    if case.prepass is not None:
        objects, run = r.screen_prepass(case.objects)
        assert (run is not None) == case.prepass, "the pre-pass packs phot_first + j into 32 bits, and falls back when it does not fit"
    try:
        if run is not None:
            assert r.bound.base_params.screen_kick is not None
            run()
        pool = r.shoot_photons(objects)                      # (with a pre-pass: reads the gathered gradients)
        r.synchronize()
    finally:
        r.bound.base_params.screen_kick = None
    got = pool.to_host()
    assert np.array_equal(got["obj_index"], np.repeat(np.arange(len(objects)), objects["n_phot"]))
    if run is not None:
        n_phot = case.objects["n_phot"]
        entries = run.keep[2].cpu().numpy()
        oi, k = entries >> 32, entries & 0xFFFFFFFF
        assert len(entries) == n_phot.sum() and len(np.unique(entries)) == len(entries)        # every photon exactly once
        assert np.array_equal(np.bincount(oi, minlength=len(n_phot)), n_phot)
        first = case.objects["phot_first"][oi]
        assert np.all((k >= first) & (k < first + n_phot[oi]))
        kick = run.keep[3].cpu().numpy()                     # [pool offset of the object + j][2]
    ref.assert_matches(shot, got, case.name, kick=kick, ratios=RATIOS)
    print("worst so far:", {f: float(f"{v:.3g}") for f, v in RATIOS.items()})


@pytest.mark.parametrize("psf,width,triple", [("radial", 0, (1, 1, R)), ("screens", 64, (1, 2, R)), ("screens", 128, (1, 2, R))])
def test_specialised_kernels_equal_the_descriptor_loops_on_small_screens(torch_cuda, monkeypatch, psf, width, triple):
    """run_psf<1> and run_psf<2> (the batched gathers: six layers, quads, a power-of-two width) against the component loop, on
    screens that wrap about a hundred times under the objects' field angles: same converted pool, bit for bit"""
    import torch
    from imsim_amd import catalog, configs
    from imsim_amd.engine import PhotonPool, Renderer, _seg_ptr
    n = 128
    monkeypatch.setenv("IMS_SCREEN_QUADS", "1")
    monkeypatch.setenv("IMS_SCREEN_PREPASS", "0")
    if psf == "radial":
        scene = configs.scene_c3(nx=n, ny=n)
    else:
        scene = configs.scene_c3b(nx=n, ny=n, screen_size=width * 0.1, screen_scale=0.1)
        assert scene.atm.npix == width and len(scene.atm.altitudes) == 6
    scene.sensor.scratch_cells = 100_000
    cat = catalog.synthetic_catalog(24, nx=n, ny=n)
    phot = catalog.realize_fluxes(cat["nominal_flux"], 5)
    phot[:6] = cases.N_PHOT
    objects = (configs.c3b_objects if psf == "screens" else configs.c3_objects)(cat, phot, scene)[0]
    tan = np.array([0.031, -0.031, 0.0007, -0.0123, 0.0201, -0.0298, 0.0, 0.0155])
    objects["atm_tan_x"], objects["atm_tan_y"] = tan[np.arange(len(objects)) % 8], -tan[(np.arange(len(objects)) + 3) % 8]
    out = []
    for switch in ("1", "0"):
        monkeypatch.setenv("IMS_CHAIN_KERNELS", switch)
        monkeypatch.setenv("IMS_LAYOUT_KERNELS", switch)
        r = Renderer(scene)
        rows, obj_t, prefix, pre_t = r._upload_objects(objects)
        prm = r.bound.params(obj_t.data_ptr(), len(rows), pre_t.data_ptr(), int(prefix[-1]), r.image.data_ptr(), None, _seg_ptr(pre_t))
        assert query(r.lib, prm, 2) == (triple if switch == "1" else (0, 0, 0))
        if psf == "screens":
            assert r.bound.atm_struct.screen_quads is not None
        offs = np.concatenate([[0], np.cumsum(rows["n_phot"])]).astype(np.int64)
        off_t = torch.from_numpy(offs).to(r.device)
        pool = PhotonPool(torch, r.device, offs[-1], off_t, obj_t, len(rows), pre_t, int(prefix[-1]))
        for t in list(pool.t.values()) + [pool.obj_index]:
            t.zero_()
        ph = pool.struct()
        ph.converted = 1
        _abi.check(r.lib.ims_shoot_ops_photons(C.byref(prm), off_t.data_ptr(), C.byref(ph), r._stream()), "ims_shoot_ops_photons")
        r.synchronize()
        host = pool.to_host()
        out.append([host[f] for f in sorted(host)])
        assert np.count_nonzero(host["flux"]) > 1000
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
