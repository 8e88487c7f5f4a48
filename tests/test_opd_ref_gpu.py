"""ims_opd / ims_opd_perturbed against tests/opd_ref.py (long double, bounds derived there) on every case of tests/opd_cases.py:
the finite mask, the map, A^T A and A^T w of the direct call, and the header's AZ_jjj; the all-NaN field and the rank-deficient
grid return the documented minimum-norm coefficients without raising."""
import ctypes as C

import numpy as np
import pytest

from imsim_amd import _abi, opd
import opd_cases
import opd_ref

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _direct(torch, case, ref):
    """ims_opd called the way opd._run calls it, with the reference's own directions rounded to binary64:
    (maps, ata [n, J, J], atw [n, J])"""
    tel, R, eps = opd_cases.parameters(case)
    lib = _abi.load()
    dev = torch.device("cuda:0")
    opt = opd_cases.descriptor(tel)
    _abi.check(lib.ims_fill_derived_medium(int(opt.in_medium_kind), opt.in_medium_c), "ims_fill_derived_medium")
    for k in range(opt.n_surfaces):
        _abi.check(lib.ims_fill_derived_medium(int(opt.surf[k].medium_kind), opt.surf[k].medium_c), "ims_fill_derived_medium")
    _abi.check(lib.ims_fill_derived_optics(C.byref(opt)), "ims_fill_derived_optics")
    opt_dev = torch.from_numpy(np.frombuffer(bytes(opt), dtype=np.uint8).copy()).to(dev)
    n, nx, J = len(case["fields"]), case["nx"], case["jmax"]
    P = _abi.Opd()
    P.n_fields, P.nx, P.reference, P.jmax = n, nx, opd.REFERENCES[case["reference"]], J
    P.dx, P.wavelength, P.sphere_radius = 2.0 * tel.pupil_outer / nx, opd_cases.WAVE, R
    P.r_outer, P.eps = tel.pupil_outer, eps
    poly, ms = opd.zernike_table(J, eps)
    dirs = torch.from_numpy(np.array([d.astype(np.float64) for d in ref.dirs])).to(dev)
    poly_d, ms_d = torch.from_numpy(poly).to(dev), torch.from_numpy(ms).to(dev)
    maps = torch.empty((n, nx, nx), dtype=torch.float64, device=dev)
    scratch = torch.empty(_abi.opd_scratch_bytes(n, nx, J), dtype=torch.uint8, device=dev)
    ata = torch.empty((n, J * (J + 1) // 2), dtype=torch.float64, device=dev)
    atw = torch.empty((n, J), dtype=torch.float64, device=dev)
    P.dirs, P.opd, P.scratch = dirs.data_ptr(), maps.data_ptr(), scratch.data_ptr()
    P.zk_poly, P.zk_m, P.zk_ata, P.zk_atw = poly_d.data_ptr(), ms_d.data_ptr(), ata.data_ptr(), atw.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    assert C.sizeof(opt) == C.sizeof(_abi.Optics)                   # the direct case is a coaxial telescope
    _abi.check(lib.ims_opd(C.byref(P), opt_dev.data_ptr(), stream), "ims_opd")
    torch.cuda.synchronize()
    packed = ata.cpu().numpy()
    full = np.zeros((n, J, J))
    iu = np.triu_indices(J)
    for f in range(n):
        full[f][iu] = packed[f]
        full[f] = full[f] + np.triu(full[f], 1).T
    return maps.cpu().numpy(), full, atw.cpu().numpy()


def _note(worst, what, value):
    worst[what] = max(worst.get(what, 0.0), value)


@pytest.mark.parametrize("case", opd_cases.CASES, ids=[c["name"] for c in opd_cases.CASES])
def test_against_the_long_double_reference(torch_cuda, case):
    ref = opd_cases.reference(case)
    tel, R, eps = opd_cases.parameters(case)
    J, nx = case["jmax"], case["nx"]
    worst = {}
    if case["direct"]:
        maps, ata, atw = _direct(torch_cuda, case, ref)
        zks = [opd.solve_normal(ata[f], atw[f]) for f in range(len(maps))]
        for f, ft in enumerate(ref.fits):
            _note(worst, "zk_ata", opd_ref.ratio(ata[f], ft.ata, ft.d_ata))
            _note(worst, "zk_atw", opd_ref.ratio(atw[f], ft.atw, ft.d_atw))
    else:
        out = opd.compute(tel, case["fields"], opd_cases.WAVE, nx=nx, projection=case["projection"],
                          sphere_radius=case["sphere_radius"], reference=case["reference"], jmax=J)     # must not raise
        maps = [m for m, _ in out]
        zks = [np.array([h[f"AZ_{j:03d}"][0] for j in range(1, J + 1)]) for _, h in out]
        assert all(h["sph_rad"][0] == R and h["eps"][0] == eps for _, h in out)
    for fld, m, zk, F, ft in zip(case["fields"], maps, zks, ref.fields, ref.fits):
        keep = ~F.flagged
        assert m.shape == (nx, nx)
        assert np.array_equal(np.isfinite(m)[keep], np.isfinite(F.opd)[keep]), f"{case['name']} {fld}: finite mask differs"
        both = keep & np.isfinite(F.opd)
        _note(worst, "map", opd_ref.ratio(m[both], F.opd[both], F.bound[both]))
        assert np.all(np.isfinite(zk))
        _note(worst, "AZ", opd_ref.ratio(zk, ft.zk, ft.zk_bound))
        if fld == opd_cases.OUT:
            assert not np.isfinite(m).any() and not np.any(zk)          # the minimum-norm fit of no pixel at all: zeros
    print(f"{case['name']}: error / bound " + " ".join(f"{q}={v:.3g}" for q, v in worst.items()))
    for q, v in worst.items():
        _note(WORST, q, v)
    bad = {q: v for q, v in worst.items() if not v <= 1.0}
    assert not bad, f"{case['name']}: error exceeds the bound: {bad}"


def test_worst_ratios_are_printed(torch_cuda):
    """the table of tests/opd_ref.py's docstring (records, not thresholds)"""
    print("worst error / bound over the cases run: " + " ".join(f"{q}={v:.3g}" for q, v in sorted(WORST.items())))
