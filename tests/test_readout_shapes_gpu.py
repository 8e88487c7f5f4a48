"""The readout kernels (k_readout_span_init .. k_readout_finish) on ragged, odd and toy amplifier geometries.  The parity tests
run the chain at the one real geometry only: raw segments of 576 x 2048 (9 x 64 by 512 x 4: no tile guard fires, no partial
x-block of staged serial weights), 16 amplifiers, 21 taps, an even number of pixels per segment (the single-pixel finish
kernel never runs).  Here: the geometry table of tests/readout_ref.py through CcdReadout.build_amp_images, the stages one at
a time through the C-ABI with hand-made descriptors, and the bleed-trail vectors generated from the reference.  Everything
is compared bit for bit, with the oracle and with the plain numpy statements of readout_ref.py (which
tests/test_readout_shapes.py proves equal to the oracle on the same inputs without a device)."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import assert_bits_equal
from imsim_amd import _abi, readout
from oracle import orc_loader
import readout_ref as ref

pytestmark = pytest.mark.gpu

SEED = 20261017
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readout_golden.npz"))
ODD_PER = {"E2V-71x37", "ITL-21x27", "E2V-131x11"}          # the rows whose chain ends in the single-pixel finish kernel


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def case_id(c):
    return f"{c[0]}amps-{c[2][0]}x{c[2][1]}"


def single_pixel_finish(ro, seg_ptr, out_ptr):
    """the choice of ims_readout_finish: pairs of pixels need an even number per segment and 8-byte aligned arrays"""
    return (ro.raw_w * ro.raw_h) % 2 == 1 or (seg_ptr | out_ptr) % 8 != 0


# ---------------------------------------------------------------------------------------------
# bleed trails
# ---------------------------------------------------------------------------------------------
def gpu_bleed(torch, img, full_well, midline):
    lib = _abi.load()
    t = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float64)).cuda()
    ny, nx = t.shape
    flags = torch.empty((nx * ny + 15) // 16 * 16 + 16 * nx, dtype=torch.uint8, device="cuda")   # IMS_READOUT_SCRATCH_BYTES
    _abi.check(lib.ims_readout_bleed(t.data_ptr(), flags.data_ptr(), nx, ny, float(full_well), int(midline), None))
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("case", ref.BLEED_CASES)
def test_bleed_shape_cases_match_reference_and_oracle(torch_cuda, case):
    """odd ny (halves of 48 and 49 rows), channels shorter than the eight rows of flags fetched at a time, more than 256
    channels (the half = t / nx boundary inside a workgroup), nothing and everything saturated, a pixel exactly at full well,
    a negative pixel beside a run"""
    fw = float(GOLD["full_well"])
    src = GOLD[f"{case}_in"]
    for key, mid in (("midline", True), ("nomidline", False)):
        got = gpu_bleed(torch_cuda, src, fw, mid)
        assert_bits_equal(got, GOLD[f"{case}_{key}"], f"{case}, {key}: reference")
        assert_bits_equal(got, orc_loader.bleed_eimage(src, fw, mid), f"{case}, {key}: oracle")
        if case == "unsat":
            assert (src == fw).any() and not (src > fw).any()
            assert_bits_equal(got, src, "an image without a saturated pixel is left alone")
        else:
            assert (got != src).any()


# ---------------------------------------------------------------------------------------------
# the whole chain on toy cameras
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(ref.CONFIGS))
@pytest.mark.parametrize("row", ref.SHAPES, ids=ref.shape_id)
def test_chain_on_toy_cameras_is_bit_exact(torch_cuda, row, cfg):
    kw = dict(ref.CONFIGS[cfg])
    ccd, ro = ref.toy_readout(row, **kw)
    e, xs = ref.toy_eimage(ccd, SEED)
    ro.eimage.array = torch_cuda.from_numpy(e.copy()).cuda()
    got = ro.build_amp_images(SEED)
    torch_cuda.cuda.synchronize()
    d = ro.descriptor()
    st = ref.oracle_stages(e, ro, d, SEED)
    ny = e.shape[0]
    assert (st["bled"] != e).any(), "the e-image must bleed"
    if row[0] == "E2V":
        assert ro.midline_stop() and (e[ny // 2 - 2:ny // 2 + 2, xs] > ro.full_well).all(), "a run must straddle the midline"
        assert not np.array_equal(st["bled"], orc_loader.bleed_eimage(e, ro.full_well, False)), "the midline stop must matter"
    else:
        assert not ro.midline_stop()
    assert_bits_equal(ro.eimage.array.cpu().numpy(), st["dark"], "e-image after bleed trails and dark current")
    assert got.shape == (16, d.raw_h, d.raw_w) and got.dtype == torch_cuda.int32
    out = got.cpu().numpy()
    assert_bits_equal(out, st["out"], "raw segments: oracle")
    seg, p, s, mine = ref.statement_chain(st["dark"], ro, d, SEED)
    assert_bits_equal(out, mine, "raw segments: numpy statements")
    # which finish kernel ran: the output tensor is a fresh allocation, so the parity of the segment size decides
    assert got.data_ptr() % 8 == 0
    assert single_pixel_finish(d, 0, got.data_ptr()) == (ref.shape_id(row) in ODD_PER)
    if kw["pcti"]:
        assert (s[:, d.data_y0 + d.seg_h:, :] > 0).any(), "deferred charge must reach the parallel overscan"
    if kw["scti"]:
        assert (s[:, :, d.data_x0 + d.seg_w:] > 0).any(), "deferred charge must reach the serial overscan"
    if kw["xtalk"]:
        plain = _abi.Readout.from_buffer_copy(bytes(d))
        plain.has_xtalk = 0
        assert (ref.segments(st["dark"], plain) != seg).any(), "a crosstalk term must be non-zero"
    if kw.get("read_noise") == 0.0:
        assert (s == 0).any() and (out[s == 0] == -300).all()                  # -300.5 truncates towards zero


# ---------------------------------------------------------------------------------------------
# the stages through the C-ABI, hand-made descriptors
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xtalk", [True, False], ids=["xtalk", "plain"])
@pytest.mark.parametrize("case", ref.SEGMENT_CASES, ids=case_id)
def test_segments_kernel_with_1_3_and_16_amplifiers(torch_cuda, case, xtalk):
    """k_readout_segments loops to IMS_MAX_AMPS under a < n_amps guards and has only ever run with 16: here 1, 3 and 16
    amplifiers, all four flip patterns, crosstalk rows with exact zeros, an imaging section offset in x and y, a raw_w that is
    no multiple of 64 and a raw_h that is no multiple of 4"""
    lib = _abi.load()
    ro, e = ref.descriptor(*case, seed=5, xtalk=xtalk)
    assert ro.raw_w % 64 and ro.raw_h % 4 and ro.data_x0 > 0 and ro.data_y0 > 0
    shape = (ro.n_amps, ro.raw_h, ro.raw_w)
    img = torch_cuda.from_numpy(e).cuda()
    n, pad = int(np.prod(shape)), 64
    buf = torch_cuda.full((n + 2 * pad,), -7.0, dtype=torch_cuda.float32, device="cuda")   # prescan and overscan must be written
    seg = buf[pad:pad + n]
    _abi.check(lib.ims_readout_segments(img.data_ptr(), e.shape[1], e.shape[0], C.byref(ro), seg.data_ptr(), None))
    torch_cuda.cuda.synchronize()
    got = seg.cpu().numpy().reshape(shape)
    want = ref.segments(e, ro)
    assert_bits_equal(got, want, "segments")
    mask = np.ones(shape[1:], bool)
    mask[ro.data_y0:ro.data_y0 + ro.seg_h, ro.data_x0:ro.data_x0 + ro.seg_w] = False
    assert (got[:, mask] == 0).all() and (got[:, ~mask] > 0).all()
    assert (buf[:pad] == -7.0).all() and (buf[pad + n:] == -7.0).all(), "nothing is written outside the segments"
    assert_bits_equal(img.cpu().numpy(), e, "the e-image is read only")
    if xtalk and ro.n_amps > 1:
        plain = _abi.Readout.from_buffer_copy(bytes(ro))
        plain.has_xtalk = 0
        assert (ref.segments(e, plain) != want).any()


@pytest.mark.parametrize("n_band", ref.CTE_BANDS)
@pytest.mark.parametrize("case", [ref.CTE_CASE, ref.SEGMENT_CASES[2]], ids=case_id)
def test_cte_kernel_band_widths_and_both_axes(torch_cuda, case, n_band):
    """k_readout_cte<21> on a partial x-block (the tail of the staged serial weights) and k_readout_cte<0>, the generic band
    width, which the chain never selects: 1, 6 and 40 taps (40 exceeds raw_h = 27, and every band but the first exceeds
    raw_h = 7 of the second geometry, where the short-tap branch is the whole image)"""
    lib = _abi.load()
    ro, e = ref.descriptor(*case, seed=5)
    shape = (ro.n_amps, ro.raw_h, ro.raw_w)
    src_h = ref.cte_input(ref.segments(e, ro), ro.n_amps)
    src = torch_cuda.from_numpy(src_h).cuda()
    for axis, cti in ((0, 2e-3), (1, 1e-3)):
        band_h = readout.cte_band(shape[1 + axis], cti, n_band - 1)
        assert band_h.shape == (shape[1 + axis], n_band)
        band = torch_cuda.from_numpy(band_h).cuda()
        dst = torch_cuda.full(shape, -7.0, dtype=torch_cuda.float32, device="cuda")
        _abi.check(lib.ims_readout_cte(src.data_ptr(), dst.data_ptr(), C.byref(ro), band.data_ptr(), n_band, axis, None))
        torch_cuda.cuda.synchronize()
        got = dst.cpu().numpy()
        assert_bits_equal(got, ref.cte(src_h, band_h, axis), f"{n_band} taps, axis {axis}: numpy statement")
        want = np.zeros(shape, dtype=np.float32)
        orc_loader.load().orc_readout_cte(src_h.ctypes.data, want.ctypes.data, C.byref(ro), band_h.ctypes.data, n_band, axis)
        assert_bits_equal(got, want, f"{n_band} taps, axis {axis}: oracle")
        assert np.allclose(got, ref.cte_dense(src_h, cti, axis, n_band - 1).astype(np.float32), rtol=ref.CTE_RTOL, atol=ref.CTE_ATOL)
        assert (got[:, -1, -1] != src_h[:, -1, -1]).all(), "the last row and column must be transferred"
        assert_bits_equal(src.cpu().numpy(), src_h, "the source is read only")


def _finish(torch, lib, ro, seg_h, seed, offset):
    """ims_readout_finish on tensors that start `offset` elements into a larger allocation; returns (result, single-pixel
    kernel?, the elements around the output)"""
    n = seg_h.size
    seg_buf = torch.full((n + 4,), 1.0e6, dtype=torch.float32, device="cuda")
    out_buf = torch.full((n + 4,), -99, dtype=torch.int32, device="cuda")
    seg, out = seg_buf[offset:offset + n], out_buf[offset:offset + n]
    seg.copy_(torch.from_numpy(seg_h.reshape(-1)))
    _abi.check(lib.ims_readout_finish(seg.data_ptr(), C.byref(ro), seed, out.data_ptr(), None))
    torch.cuda.synchronize()
    all_out = out_buf.cpu().numpy()
    around = np.concatenate([all_out[:offset], all_out[offset + n:]])
    return all_out[offset:offset + n].reshape(seg_h.shape), single_pixel_finish(ro, seg.data_ptr(), out.data_ptr()), around


def test_finish_kernels_agree_and_match_the_statement(torch_cuda):
    """k_readout_finish, the one-pixel-per-thread kernel, claims the bits of k_readout_finish_pairs and has never run: the same
    even-sized segments through the pairs kernel (8-byte aligned) and, as views one element into a larger tensor (4-byte
    aligned only), through the single-pixel kernel; then an odd segment size with three amplifiers"""
    lib = _abi.load()
    ro, e = ref.descriptor(*ref.FINISH_EVEN, seed=5)
    assert (ro.raw_w * ro.raw_h) % 2 == 0 and ro.n_amps == 16
    seg_h = (ref.cte_input(ref.segments(e, ro), 3) - np.float32(2000.0)).astype(np.float32)
    want = ref.finish(seg_h, ro, 99)
    assert (want < 0).any() and (want > 0).any()
    pairs, single0, around0 = _finish(torch_cuda, lib, ro, seg_h, 99, 0)
    ones, single1, around1 = _finish(torch_cuda, lib, ro, seg_h, 99, 1)
    assert not single0 and single1, "aligned tensors take the pairs kernel, the shifted views the single-pixel kernel"
    assert_bits_equal(pairs, ones, "pairs kernel vs single-pixel kernel")
    assert_bits_equal(pairs, want, "pairs kernel vs numpy statement")
    assert_bits_equal(ones, want, "single-pixel kernel vs numpy statement")
    assert (around0 == -99).all() and (around1 == -99).all(), "nothing is written outside the segments"
    orc = np.zeros(want.shape, dtype=np.int32)
    orc_loader.load().orc_readout_finish(seg_h.ctypes.data, C.byref(ro), 99, orc.ctypes.data)
    assert_bits_equal(pairs, orc, "oracle")

    ro, e = ref.descriptor(*ref.FINISH_ODD, seed=6)
    assert (ro.raw_w * ro.raw_h) % 2 == 1 and ro.n_amps == 3
    seg_h = (ref.cte_input(ref.segments(e, ro), 4) - np.float32(2000.0)).astype(np.float32)
    want = ref.finish(seg_h, ro, 7)
    for offset in (0, 1):
        got, single, around = _finish(torch_cuda, lib, ro, seg_h, 7, offset)
        assert single
        assert_bits_equal(got, want, f"odd segment size, offset {offset}")
        assert (around == -99).all()
    assert not np.array_equal(want, ref.finish(seg_h, ro, 8))                 # the seed matters: read noise is on
