"""ims_fft_reshoot on the device against tests/fft_reshoot_ref.py, on the hand-made batch of tests/fft_reshoot_cases.py (grids of 32
and 64), then through FftDrawer and through config.Process (stamp.fft_reshoot).

What is exact is compared exactly: the counts, the photons as made (positions, fluxes, rows, ordinals), the binning -- the output
image equals the fixed-point binning of the device's OWN dumped photons bit for bit, so no photon near a pixel edge needs excusing.
What the operators compute is held to photon_ops_ref's own tolerances and its own cap on the flagged share."""
import ctypes as C

import numpy as np
import pytest

import fft_reshoot_cases as cases
import fft_reshoot_ref as ref
import photon_ops_ref as ops_ref
import photon_source_ref as src_ref
from imsim_amd import _abi, fft_draw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def launch(torch, chain, pool_stage=0, raw=0, grid=0):
    """one call of the entry point on the batch -> (out [n_pix], pool fields or None, land or None)"""
    from imsim_amd.engine import Renderer
    fft, po, v, sc, _, made, _ = cases.reference(chain)
    r = Renderer(sc)
    R = fft_draw.Reshoot(r)
    dev = r.device
    buf = np.array(v, copy=True)
    if raw:
        for o in fft:                                                            # pre-multiplied: the kernel's 1 / nfft^2 undoes it exactly
            n = int(o["nfft"])
            buf[int(o["r_offset"]):int(o["r_offset"]) + n * n] *= float(n * n)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fft_t, po_t = up(fft.view(np.uint8).reshape(-1)), up(po.view(np.uint8).reshape(-1))
    rpre = np.concatenate([[0], np.cumsum(fft["nfft"].astype(np.int64) ** 2)]).astype(np.int64)
    n_pix = int(rpre[-1])
    rpre_t, buf_t = up(rpre), up(buf)
    work = torch.empty(int(r.lib.ims_fft_reshoot_work_bytes(n_pix)), dtype=torch.uint8, device=dev)
    out = torch.full((n_pix,), 7.0, dtype=torch.float64, device=dev)             # (the call zeroes it)
    n = int(made["offset"][-1])
    pool = pool_t = off_t = land_t = None
    if pool_stage:
        pool_t = {q: torch.full((n,), np.nan, dtype=torch.float64, device=dev) for q in ops_ref.FIELDS}
        pool_t["obj_index"] = torch.full((n,), -5, dtype=torch.int32, device=dev)
        land_t = torch.full((n,), -7, dtype=torch.int32, device=dev)
        off_t = up(made["offset"])
        pool = _abi.Photons()
        pool.n = n
        for q in ops_ref.FIELDS:
            setattr(pool, q, pool_t[q].data_ptr())
        pool.obj_index = pool_t["obj_index"].data_ptr()
    FP = _abi.FftParams()
    FP.seed = sc.seed
    _abi.check(r.lib.ims_fft_reshoot(C.byref(FP), C.byref(R.P), fft_t.data_ptr(), fft.ctypes.data, po_t.data_ptr(), len(fft), rpre_t.data_ptr(),
                                     n_pix, buf_t.data_ptr(), raw, 1.0, work.data_ptr(), out.data_ptr(),
                                     C.byref(pool) if pool is not None else None, off_t.data_ptr() if off_t is not None else None,
                                     land_t.data_ptr() if land_t is not None else None, pool_stage, grid, r._stream()), "ims_fft_reshoot")
    r.synchronize()
    total = int(work.view(torch.int64)[-1].item())
    assert total == n, f"photon total on the device {total}, restatement {n}"
    got = {q: t.cpu().numpy() for q, t in pool_t.items()} if pool_t is not None else None
    return out.cpu().numpy(), got, (land_t.cpu().numpy() if land_t is not None else None)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {np.flatnonzero(bad)[:5]}: {a[bad][:3]} vs {b[bad][:3]}"


def test_a_chain_that_moves_nothing_gives_the_restatement_bit_for_bit(torch_cuda):
    fft, po, v, sc, want, made, _ = cases.reference("time")
    assert made["n_per_pixel"][0].max() > 3 * cases.RUN                          # one pixel spans more than three of the kernel's runs
    out, _, _ = launch(torch_cuda, "time")
    same_bits(out, want, "output")
    same_bits(launch(torch_cuda, "time", raw=1)[0], out, "raw = 1 on a pre-multiplied buffer")
    for grid in (1, 3, 500):
        same_bits(launch(torch_cuda, "time", grid=grid)[0], out, f"grid of {grid} workgroups")
    # outside the stamps: zero, whatever the input held there
    for o in fft:
        n = int(o["nfft"])
        ok, _, _ = ref.in_stamp(o)
        g = out[int(o["r_offset"]):int(o["r_offset"]) + n * n].reshape(n, n)
        assert np.all(g[~ok] == 0.0) and np.any(v[int(o["r_offset"]):int(o["r_offset"]) + n * n].reshape(n, n)[~ok] != 0.0)


def test_photons_as_made_equal_the_restatement(torch_cuda):
    _, _, _, _, _, made, _ = cases.reference("time")
    _, got, _ = launch(torch_cuda, "time", pool_stage=1)
    for q in ("x", "y", "flux", "dxdz", "dydz", "pupil_u", "pupil_v", "time"):
        same_bits(got[q], made["fields"][q], q)
    assert np.array_equal(got["obj_index"], made["obj_index"])                   # the FFT row; the place in the pool is offset + ordinal
    err = np.abs(got["wavelength"].astype(src_ref.LD) - made["fields"]["wavelength"].astype(src_ref.LD))
    assert np.all(err <= made["wl_bound"] + src_ref.EPS * 1100.0), f"wavelength: worst {float(err.max())}"
    assert np.ptp(got["wavelength"][made["obj_index"] == 1]) > 50.0 and np.all(got["wavelength"][made["obj_index"] == 0] == 620.0)


@pytest.mark.parametrize("chain", ["default", "descriptor"])
def test_photons_after_the_operators_and_their_binning(torch_cuda, chain):
    from imsim_amd.engine import Renderer
    fft, po, v, sc, _, made, res = cases.reference(chain)
    # which kernel runs: the straight-line chain for the default six, the descriptor loop otherwise
    r = Renderer(sc)
    R = fft_draw.Reshoot(r)
    ch, psf, lay = C.c_int32(), C.c_int32(), C.c_uint64()
    _abi.check(r.lib.ims_photon_kernel_variant(C.byref(R.P), 2, C.byref(ch), C.byref(psf), C.byref(lay)))
    assert ch.value == (1 if chain == "default" else 0)
    out, got, land = launch(torch_cuda, chain, pool_stage=2)
    ops_ref.assert_matches(res, got, f"re-shot photons, {chain} chain")
    assert np.array_equal(got["obj_index"], made["obj_index"])
    want, _, want_land = ref.bin_photons(fft, got["x"], got["y"], got["flux"], got["obj_index"])
    same_bits(out, want, "output against the binning of the device's own photons")
    assert np.array_equal(land, want_land)
    lost = float((land < 0).mean())
    print(f"{chain}: {len(land)} photons, {lost:.3f} lost")
    assert lost < 0.5 and (lost > 0.0 or chain == "descriptor")                  # the optics vignette some; most arrive
    same_bits(launch(torch_cuda, chain, grid=5)[0], out, "grid of 5 workgroups")


def _bright_point(chain_ops, reshoot):
    """one point source of 5e4 e- on a 64 grid through a Gaussian PSF, no noise -> (stamp values without the stage, CCD image, realized)"""
    import torch
    import photon_ops_cases as pc
    from imsim_amd.engine import Renderer, Scene
    sc = Scene(nx=128, ny=128, seed=pc.SEED, psf=[], ops=chain_ops)
    po = pc.rows(1)
    po["obj_id"], po["x0"], po["y0"] = 77, 60.3, 70.6
    po["stamp_xmin"], po["stamp_xmax"], po["stamp_ymin"], po["stamp_ymax"] = 35, 86, 44, 97              # 52 x 54: a 64 grid
    rows, order = fft_draw.build_fft_objects(po, np.array([5.0e4]), np.array([_abi.IMS_PROF_POINT]))
    assert list(rows["nfft"]) == [64]
    r = Renderer(sc)
    drawer = fft_draw.FftDrawer(r, [(_abi.IMS_KPSF_GAUSSIAN, 0, 0.35)], add_noise=False, reshoot=fft_draw.Reshoot(r) if reshoot else None)
    real = torch.zeros(1, dtype=torch.float64, device=r.device)
    _, rbuf = drawer.draw(rows, realized=real, photon_objects=po[order])
    r.synchronize()
    stamp = rbuf.cpu().numpy() if reshoot else fft_draw.image_from_rbuf(rows, rbuf.cpu().numpy())
    return rows, stamp, r.image64_numpy(), float(real.item())


def test_drawer_with_a_chain_that_moves_nothing_keeps_the_image(torch_cuda):
    rows, v, plain, real0 = _bright_point([cases.TIME_OP], False)
    _, _, shot, real1 = _bright_point([cases.TIME_OP], True)
    o = rows[0]
    ok, px, py = ref.in_stamp(o)
    grid = v.reshape(64, 64)
    n = np.where(ok, ref.counts(grid), 0)
    bound = n * 2.0 ** -33 + np.abs(grid) * 2.0 ** -52                            # one rounding of the deposit per photon, one of v / N
    assert n.sum() > 4.0e4 and n.max() > 1000
    on = np.zeros((128, 128))
    on[py[ok] - 1, px[ok] - 1] = bound[ok]
    diff = np.abs(shot - plain)
    print(f"worst difference {diff.max():.3e}, its bound {on[diff == diff.max()].max():.3e}; realized {real1 - real0:.3e}, bound {bound[ok].sum():.3e}")
    assert np.any(shot != plain) and np.all(diff <= on)
    assert abs(real1 - real0) <= bound[ok].sum()


def _process(**over):
    import os
    from imsim_amd import config
    here = os.path.dirname(os.path.abspath(__file__))
    o = {"input.instance_catalog.file_name": os.path.join(here, "golden", "example_instcat_subset.txt")}
    o.update(over)
    return config.Process(os.path.join(here, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(here, "data")], overrides=o)


# the default chain of tests/data/test-config-base.yaml's stamp.photon_ops, as stamp.fft_photon_ops
DEFAULT_CHAIN = [
    {"type": "TimeSampler", "t0": 0.0, "exptime": "$exptime"},
    {"type": "PupilAnnulusSampler", "R_outer": "$pupil_R_outer", "R_inner": "$pupil_R_inner"},
    {"type": "PhotonDCR", "base_wavelength": "$bandpass.effective_wavelength", "latitude": "-30.24463 degrees"},
    {"type": "RubinDiffractionOptics", "det_name": "$det_name", "boresight": [0, 0], "camera": "LsstCamSim", "altitude": "$altitude",
     "azimuth": "$azimuth"},
    {"type": "FocusDepth", "depth": 0},
    {"type": "Refraction", "index_ratio": 3.9},
]


def test_config_switch_runs_the_stage(torch_cuda):
    """stamp.fft_reshoot: true with the default chain as fft_photon_ops: the brightest star above the threshold is FFT-drawn and
    re-shot -- it loses the share the optics vignette and the stamp clips, no more than tests/test_parity_gpu.py accepts for
    photon-shot objects (test_config_phot_full_chain_and_pooling_agree: above 0.85)"""
    from imsim_amd.lsst_image import GalSimConfigError
    over = {"image.nobjects": 40, "stamp.fft_sb_thresh": 2.0e3, "image.sensor": ""}
    base = _process(**over)
    with pytest.raises(GalSimConfigError, match="fft_photon_ops"):
        _process(**dict(over, **{"stamp.fft_photon_ops": DEFAULT_CHAIN}))
    res = _process(**dict(over, **{"stamp.fft_photon_ops": DEFAULT_CHAIN, "stamp.fft_reshoot": True}))
    assert not any("fft_reshoot" in s or "fft_photon_ops" in s for s in res.ignored)
    t0, t1 = base.truth[0], res.truth[0]
    assert list(t0["mode"]) == list(t1["mode"])
    fft = np.flatnonzero(np.asarray(t1["mode"]) == "fft")
    assert len(fft) > 0
    inside = (t1["x"][fft] > 200) & (t1["x"][fft] < 3896) & (t1["y"][fft] > 200) & (t1["y"][fft] < 3800)
    assert inside.any()
    star = fft[inside][np.argmax(np.asarray(t1["nominal_flux"])[fft][inside])]
    f0, f1 = float(t0["realized_flux"][star]), float(t1["realized_flux"][star])
    print(f"realized flux of the star ({float(t1['nominal_flux'][star]):.3g} e-): {f0:.1f} without fft_photon_ops, {f1:.1f} re-shot ({f1 / f0:.4f})")
    assert 0.85 * f0 < f1 < f0
