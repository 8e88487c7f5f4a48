"""Which photon kernel a descriptor gets (ims_photon_kernel_variant): every kernel form computes the same bits, so a wrong choice
shows in no parity test -- only here.  The CPU test holds the selector against the rules written out below; the GPU test
launches every row of the table and compares with the kernels that loop over the descriptors."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from imsim_amd import _abi, tuning

G, RAD, SCR, OPT = _abi.IMS_PSF_GAUSSIAN, _abi.IMS_PSF_RADIAL, _abi.IMS_PSF_SCREENS, _abi.IMS_PSF_OPTICAL_SCREEN
R = 0x755556455333                         # IMS_LAYOUT_RUBIN_LIKE: the nibbles 3 3 3 5 5 4 6 5 5 5 5 7, first surface lowest
P = _abi.IMS_LAYOUT_PERTURBED
DEFAULT_CHAIN = [_abi.IMS_OP_TIME_SAMPLER, _abi.IMS_OP_PUPIL_ANNULUS_SAMPLER, _abi.IMS_OP_PHOTON_DCR,
                 _abi.IMS_OP_RUBIN_DIFFRACTION_OPTICS, _abi.IMS_OP_FOCUS_DEPTH, _abi.IMS_OP_REFRACTION]
CHAINS = {"default": DEFAULT_CHAIN, "five": DEFAULT_CHAIN[:5],
          "swapped": DEFAULT_CHAIN[:4] + [DEFAULT_CHAIN[5], DEFAULT_CHAIN[4]]}
PSFS = {"radial": ([RAD, G], False), "screens": ([SCR, RAD, G], True), "screens_no_atm": ([SCR, RAD, G], False),
        "doopt": ([SCR, RAD, OPT, G], True), "doopt_no_atm": ([SCR, RAD, OPT, G], False), "optical": ([OPT, G], True),
        "gaussian": ([G], False)}
TUNINGS = {"defaults": {}, "no_chain": {"chain_kernels": 0}, "no_layout": {"layout_kernels": 0}, "no_screens": {"psf_screens_kernel": 0}}

# mode 2 (the fused kernel and k_shoot_photons on a converted pool): the first row that matches, in the order of the
# launch ladders this table replaced.  (optical screen in the list, condition on (pv, lay, layout), (CHAIN, PSF, LAYOUT))
ROWS = [(True, lambda pv, lay, layout: layout == P, (0, 3, P)),
        (True, lambda pv, lay, layout: pv == 4 and lay, (1, 4, R)),
        (True, lambda pv, lay, layout: True, (0, 3, 0)),
        (False, lambda pv, lay, layout: layout == P, (0, 0, P)),
        (False, lambda pv, lay, layout: pv == 2 and lay, (1, 2, R)),
        (False, lambda pv, lay, layout: pv == 2, (1, 0, 0)),
        (False, lambda pv, lay, layout: pv == 1 and lay, (1, 1, R)),
        (False, lambda pv, lay, layout: pv == 0 and lay, (1, 0, R)),
        (False, lambda pv, lay, layout: pv == 1, (1, 1, 0)),
        (False, lambda pv, lay, layout: pv == 0, (1, 0, 0)),
        (False, lambda pv, lay, layout: True, (0, 0, 0))]


def expected(ops, kinds, atm, layout, mode, t):
    """the rules of the ladders: t = (chain_kernels, layout_kernels, psf_screens_kernel)"""
    chain_kernels, layout_kernels, screens_kernel = t
    optical = OPT in kinds
    if mode == 0:
        return (0, 3 if optical else 0, 0)
    if mode == 1:
        return (0, 3 if optical else 0, P if layout == P else 0)
    dc = ops == DEFAULT_CHAIN and chain_kernels
    if not dc:
        pv = -1
    elif optical:
        pv = 4 if chain_kernels and screens_kernel and kinds == [SCR, RAD, OPT, G] else 3
    elif not chain_kernels:
        pv = 0
    elif kinds == [RAD, G]:
        pv = 1
    elif screens_kernel and kinds == [SCR, RAD, G] and atm:
        pv = 2
    else:
        pv = 0
    lay = pv >= 0 and layout == R and bool(layout_kernels)
    return next(triple for has, cond, triple in ROWS if has == optical and cond(pv, lay, layout))


def descriptor(ops, kinds, atm, layout):
    """a parameter block with nothing but what the selector reads: no objects, no image"""
    prm = _abi.RenderParams()
    prm.n_ops, prm.n_psf, prm.optics_layout = len(ops), len(kinds), layout
    for k, kind in enumerate(ops):
        prm.ops[k].kind = kind
    for k, kind in enumerate(kinds):
        prm.psf[k].kind = kind
    dummy = (C.c_double * 1)()
    prm.atm = C.cast(dummy, C.c_void_p) if atm else None
    return prm, dummy


def query(lib, prm, mode):
    chain, psf, layout = C.c_int32(-7), C.c_int32(-7), C.c_uint64(7)
    assert lib.ims_photon_kernel_variant(C.byref(prm), mode, C.byref(chain), C.byref(psf), C.byref(layout)) == 0, lib.ims_last_error()
    return chain.value, psf.value, layout.value


def set_tuning(lib, **fields):
    t = tuning.Tuning()
    assert lib.ims_tuning_defaults(C.byref(t)) == 0
    for k, v in fields.items():
        setattr(t, k, v)
    assert lib.ims_set_tuning(C.byref(t)) == 0
    tuning._LAST[0] = None                                      # (the next tuning.sync_library hands its own block over again)
    return t.chain_kernels, t.layout_kernels, t.psf_screens_kernel


def test_selector_follows_the_table():
    lib = _abi.load()
    assert lib.ims_known_optics_layout(R) == 1
    seen, n = set(), 0
    try:
        for tname, fields in TUNINGS.items():
            t = set_tuning(lib, **fields)
            for (cname, ops), (pname, (kinds, atm)), layout, mode in itertools.product(CHAINS.items(), PSFS.items(), (0, R, P), (0, 1, 2)):
                prm, keep = descriptor(ops, kinds, atm, layout)
                want = expected(ops, kinds, atm, layout, mode, t)
                assert query(lib, prm, mode) == want, (tname, cname, pname, hex(layout), mode)
                seen.add((mode,) + want)
                n += 1
    finally:
        set_tuning(lib)
    assert n == 4 * 3 * 7 * 3 * 3
    # the cases reach every kernel the library holds: all ten triples in mode 2, four in mode 1, two in mode 0
    assert {s[1:] for s in seen if s[0] == 2} == {row[2] for row in ROWS} and len({row[2] for row in ROWS}) == 10
    assert {s[1:] for s in seen if s[0] == 1} == {(0, 0, 0), (0, 3, 0), (0, 0, P), (0, 3, P)}
    assert {s[1:] for s in seen if s[0] == 0} == {(0, 0, 0), (0, 3, 0)}


def test_selector_corner_cases():
    """the rules that no single ladder showed"""
    lib = _abi.load()
    try:
        set_tuning(lib)
        # variant 2 without a layout kernel runs the component loop on the default chain, not run_psf<2>
        assert query(lib, descriptor(DEFAULT_CHAIN, [SCR, RAD, G], True, 0)[0], 2) == (1, 0, 0)
        assert query(lib, descriptor(DEFAULT_CHAIN, [SCR, RAD, G], True, R)[0], 2) == (1, 2, R)
        # variant 2 asks for the atmosphere descriptor, variant 4 does not
        assert query(lib, descriptor(DEFAULT_CHAIN, [SCR, RAD, G], False, R)[0], 2) == (1, 0, R)
        assert query(lib, descriptor(DEFAULT_CHAIN, [SCR, RAD, OPT, G], False, R)[0], 2) == (1, 4, R)
        # a perturbed layout beats everything; modes 0 and 1 never take a specialised kernel
        assert query(lib, descriptor(DEFAULT_CHAIN, [SCR, RAD, OPT, G], True, P)[0], 2) == (0, 3, P)
        assert query(lib, descriptor(DEFAULT_CHAIN, [RAD, G], False, P)[0], 2) == (0, 0, P)
        assert query(lib, descriptor(DEFAULT_CHAIN, [RAD, G], False, R)[0], 1) == (0, 0, 0)
        assert query(lib, descriptor(DEFAULT_CHAIN, [SCR, RAD, OPT, G], True, P)[0], 1) == (0, 3, P)
        assert query(lib, descriptor(DEFAULT_CHAIN, [SCR, RAD, OPT, G], True, P)[0], 0) == (0, 3, 0)
        # without the chain kernels a list with an optical screen is variant 3, never 4 -- and never a kernel without it
        set_tuning(lib, chain_kernels=0)
        assert query(lib, descriptor(DEFAULT_CHAIN, [SCR, RAD, OPT, G], True, R)[0], 2) == (0, 3, 0)
        assert query(lib, descriptor(DEFAULT_CHAIN, [RAD, G], False, R)[0], 2) == (0, 0, 0)
    finally:
        set_tuning(lib)


def test_query_refuses_null_arguments_and_unknown_modes():
    lib = _abi.load()
    prm, keep = descriptor(DEFAULT_CHAIN, [RAD, G], False, R)
    a, b, c = C.c_int32(), C.c_int32(), C.c_uint64()
    for args in ((None, 2, C.byref(a), C.byref(b), C.byref(c)), (C.byref(prm), 2, None, C.byref(b), C.byref(c)),
                 (C.byref(prm), 2, C.byref(a), None, C.byref(c)), (C.byref(prm), 2, C.byref(a), C.byref(b), None)):
        assert lib.ims_photon_kernel_variant(*args) == -1 and b"NULL" in lib.ims_last_error()
    for mode in (3, -1):
        assert lib.ims_photon_kernel_variant(C.byref(prm), mode, C.byref(a), C.byref(b), C.byref(c)) == -1
        assert b"mode" in lib.ims_last_error()


# ---- on the GPU: every row launched, against the kernels that loop over the descriptors ----
N = 256
# (mode, (CHAIN, PSF, LAYOUT), PSF list of the scene, perturbed telescope, five operators instead of six, optics_layout left out)
GPU_ROWS = [(mode, triple) + how for mode in ("fused", 2) for triple, how in (
                ((0, 3, P), ("doopt", True, False, False)), ((1, 4, R), ("doopt", False, False, False)),
                ((0, 3, 0), ("doopt", False, True, False)), ((0, 0, P), ("radial", True, False, False)),
                ((1, 2, R), ("screens", False, False, False)), ((1, 0, 0), ("screens", False, False, True)),
                ((1, 1, R), ("radial", False, False, False)), ((1, 0, R), ("gaussian", False, False, False)),
                ((1, 1, 0), ("radial", False, False, True)), ((0, 0, 0), ("radial", False, True, False)))]
GPU_ROWS += [(1, (0, 0, 0), "radial", False, False, False), (1, (0, 3, 0), "doopt", False, False, False),
             (1, (0, 0, P), "radial", True, False, False), (1, (0, 3, P), "doopt", True, False, False),
             (0, (0, 0, 0), "radial", False, False, False), (0, (0, 3, 0), "doopt", False, False, False)]
_SCENES = {}


def _scene(psf, perturbed, five_ops):
    """256 x 256 Silicon scenes of the C3 family (as smoke()), built once per PSF list"""
    import copy
    import os
    from imsim_amd import configs, diffraction, optics
    if psf not in _SCENES:
        golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        if psf in ("radial", "gaussian"):
            sc = configs.scene_c3(nx=N, ny=N)
            if psf == "gaussian":
                sc.psf = sc.psf[1:]
        else:
            sc = configs.scene_c3b(nx=N, ny=N, screen_size=102.4, screen_scale=0.1,
                                   optical=dict(doOpt=True, data_dir=golden) if psf == "doopt" else None)
        sc.sensor.scratch_cells = 400_000
        _SCENES[psf] = sc
    sc = copy.copy(_SCENES[psf])
    if five_ops:
        sc.ops = sc.ops[:5]
    if perturbed:
        v = configs.VISIT
        tel = optics.apply_perturbations(optics.rubin_like_telescope(v["band"]), [{"M2": {"shift": [50e-6, 0.0, 0.0]}}])
        po = optics.make_optics(tel, (100.0, 0.0, (N - 1) / 2.0 + 0.5, 0.0, 100.0, (N - 1) / 2.0 + 0.5), math.radians(v["rottelpos"]))
        assert isinstance(po, _abi.OpticsPerturbed)
        po.img_wcs, po.icrf_to_field = sc.optics.img_wcs, sc.optics.icrf_to_field
        diffraction.fill_optics(po, math.radians(v["latitude"]), math.radians(v["azimuth"]), math.radians(v["altitude"]))
        sc.optics = po
    return sc


def _catalog_objects(scene):
    """60 objects; the shapes at which a wrong launch (not wrong arithmetic) shows: one live wavefront of four, two segments, a
    stamp across the image edge"""
    from imsim_amd import catalog, configs
    cat = catalog.synthetic_catalog(60, nx=N, ny=N)
    phot = catalog.realize_fluxes(cat["nominal_flux"], 7)
    phot[0], phot[1], phot[2] = 40, 700, 900
    cat["x"][2], cat["y"][2] = 2.3, 120.7
    objects = configs.c3b_objects(cat, phot, scene)[0]
    assert objects["n_phot"][0] < 64 and objects["n_phot"][1] > 256 and objects["stamp_xmin"][2] < 1 <= objects["stamp_xmax"][2]
    return objects


@pytest.mark.gpu
@pytest.mark.parametrize("mode,triple,psf,perturbed,five_ops,no_layout", GPU_ROWS,
                         ids=[f"{r[0]}-{r[1][0]}{r[1][1]}{'P' if r[1][2] == P else 'R' if r[1][2] else '0'}" for r in GPU_ROWS])
def test_every_row_launches_its_kernel_and_equals_the_loops(monkeypatch, mode, triple, psf, perturbed, five_ops, no_layout):
    """The query names the row's kernel for the very parameter block that is launched, and the launch gives the image (fused) or
    the photon pool (k_shoot_photons) of the same scene with chain_kernels = layout_kernels = 0, bit for bit."""
    import torch
    from imsim_amd.engine import PhotonPool, Renderer, _seg_ptr
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    scene = _scene(psf, perturbed, five_ops)
    objects = _catalog_objects(scene)
    out = []
    for switch in ("1", "0"):
        monkeypatch.setenv("IMS_CHAIN_KERNELS", switch)
        monkeypatch.setenv("IMS_LAYOUT_KERNELS", switch)
        r = Renderer(scene)                                              # (hands the switches to the library)
        lib = r.lib
        rows, obj_t, prefix, pre_t = r._upload_objects(objects)
        prm = r.bound.params(obj_t.data_ptr(), len(rows), pre_t.data_ptr(), int(prefix[-1]), r.image.data_ptr(), None, _seg_ptr(pre_t))
        if no_layout:
            prm.optics_layout = 0                                        # optional: the trace loops over the surfaces
        if switch == "1":
            assert query(lib, prm, 2 if mode == "fused" else mode) == triple
        if mode == "fused":
            _abi.check(lib.ims_shoot_accumulate(C.byref(prm), r._stream()), "ims_shoot_accumulate")
            r.synchronize()
            out.append([r.image64_numpy()])
            assert out[-1][0].sum() > 0
            continue
        offs = np.concatenate([[0], np.cumsum(rows["n_phot"])]).astype(np.int64)
        off_t = torch.from_numpy(offs).to(r.device)
        pool = PhotonPool(torch, r.device, offs[-1], off_t, obj_t, len(rows), pre_t, int(prefix[-1]))
        for t in list(pool.t.values()) + [pool.obj_index]:
            t.zero_()                                                    # (a converted pool leaves some fields unwritten)
        ph = pool.struct()
        ph.converted = 1 if mode == 2 else 0
        entry = lib.ims_shoot_photons if mode == 0 else lib.ims_shoot_ops_photons
        _abi.check(entry(C.byref(prm), off_t.data_ptr(), C.byref(ph), r._stream()), "ims_shoot_photons / ims_shoot_ops_photons")
        r.synchronize()
        host = pool.to_host()
        out.append([host[f] for f in sorted(host)])
        assert np.count_nonzero(host["flux"]) > 1000
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
