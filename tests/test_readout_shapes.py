"""The readout stages on ragged, odd and toy amplifier geometries, CPU side: the plain numpy statements of
tests/readout_ref.py against the oracle, stage by stage and bit for bit, on every geometry and every hand-made descriptor the
GPU tests (test_readout_shapes_gpu.py) use -- the proof that the statements and the inputs are sound -- and the argument
checks of the C-ABI entry points, which run before any launch and need no device."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal
from imsim_amd import _abi, readout
from oracle import orc_loader
import readout_ref as ref

SEED = 20261017


def test_shape_table_has_the_rows_it_promises():
    rows = [dict(vendor=v, seg_w=s[0], seg_h=s[1], raw_w=r[0], raw_h=r[1], prescan=p, per=r[0] * r[1]) for v, s, r, p in ref.SHAPES]
    for g in rows:
        assert g["prescan"] + g["seg_w"] < g["raw_w"] and g["seg_h"] < g["raw_h"]        # a serial and a parallel overscan
    r1, r2, r3, r4, r5, r6 = rows[:6]
    assert r1["vendor"] == "E2V" and 64 < r1["raw_w"] < 128 and r1["raw_h"] % 4 == 1 and r1["per"] % 2 == 1
    assert r1["raw_w"] > 21 and r1["raw_h"] > 21
    assert r2["vendor"] == "ITL" and r2["raw_w"] == readout.NTRANSFERS + 1 and r2["per"] % 2 == 1
    assert r3["raw_h"] < 21 and r3["raw_w"] == 2 * 64 + 3
    assert r4["raw_w"] < 21 and r4["per"] % 2 == 0 and (r4["seg_w"], r4["seg_h"]) == (12, 20)
    assert r5["raw_w"] % 64 == 0 and r5["raw_h"] % 4 == 0 and r5["per"] % 2 == 0
    assert r6["vendor"] == "E2V" and r6["seg_h"] % 2 == 1 and r6["seg_h"] < 8
    # the toy of test_readout.py keeps its defaults
    ccd = ref.small_ccd()
    assert ccd.bounds.numpyShape() == (40, 96) and ccd["C10"].raw_bounds.numpyShape() == (26, 20) and ccd.serial.startswith("E2V")


@pytest.mark.parametrize("cfg", list(ref.CONFIGS))
@pytest.mark.parametrize("row", ref.SHAPES, ids=ref.shape_id)
def test_statements_equal_the_oracle_stage_by_stage(row, cfg):
    kw = dict(ref.CONFIGS[cfg])
    ccd, ro = ref.toy_readout(row, **kw)
    e, xs = ref.toy_eimage(ccd, SEED)
    d = ro.descriptor()
    st = ref.oracle_stages(e, ro, d, SEED)
    ny = e.shape[0]
    assert (st["bled"] != e).any(), "the e-image must bleed"
    assert (e[ny // 2 - 2:ny // 2 + 2, xs] > ro.full_well).all(), "a run must straddle the midline"
    if ro.midline_stop():
        assert not np.array_equal(st["bled"], orc_loader.bleed_eimage(e, ro.full_well, False)), "the midline stop must matter"

    seg, p, s, out = ref.statement_chain(st["dark"], ro, d, SEED)
    assert_bits_equal(seg, st["segments"], "segments")
    mask = np.ones(seg.shape[1:], bool)
    mask[d.data_y0:d.data_y0 + d.seg_h, d.data_x0:d.data_x0 + d.seg_w] = False
    assert mask.any() and (seg[:, mask] == 0).all() and (seg[:, ~mask] > 0).all()
    if kw["xtalk"]:
        plain = _abi.Readout.from_buffer_copy(bytes(d))
        plain.has_xtalk = 0
        assert (ref.segments(st["dark"], plain) != seg).any(), "a crosstalk term must be non-zero"
    else:
        assert d.has_xtalk == 0

    assert_bits_equal(p, st["pcte"], "after the parallel transfer")
    assert_bits_equal(s, st["cte"], "after the serial transfer")
    x = seg.astype(np.float64)
    if kw["pcti"]:
        x = ref.cte_dense(x, kw["pcti"], 0).astype(np.float32).astype(np.float64)
        assert (s[:, d.data_y0 + d.seg_h:, :] > 0).any(), "deferred charge must reach the parallel overscan"
    else:
        assert (s[:, d.data_y0 + d.seg_h:, :] == 0).all()
    if kw["scti"]:
        x = ref.cte_dense(x, kw["scti"], 1)
        assert (s[:, :, d.data_x0 + d.seg_w:] > 0).any(), "deferred charge must reach the serial overscan"
    assert np.allclose(s, x.astype(np.float32), rtol=ref.CTE_RTOL, atol=ref.CTE_ATOL)

    assert_bits_equal(out, st["out"], "int32 segments")
    assert np.abs(out.astype(np.int64)).max() < 2 ** 24                 # far inside the int32 range
    if kw.get("read_noise") == 0.0:
        # nothing but the bias where no charge arrived: -300.5 becomes -300 (towards zero), not -301
        assert kw["bias_level"] == -300.5 and (s == 0).any() and (out[s == 0] == -300).all() and (out < 0).any()
    else:
        assert (out != (s + np.float32(d.amps[0].bias_level)).astype(np.int32)).any(), "read noise must show"


@pytest.mark.parametrize("case", ref.SEGMENT_CASES + [ref.CTE_CASE, ref.FINISH_EVEN], ids=lambda c: f"{c[0]}amps-{c[2][0]}x{c[2][1]}")
@pytest.mark.parametrize("xtalk", [True, False])
def test_hand_made_descriptors_statements_equal_the_oracle(case, xtalk):
    """the stages one at a time, as the GPU tests call them through the C-ABI: n_amps of 1, 3 and 16, all flip patterns, an
    imaging section offset in x and y, crosstalk rows with exact zeros; band widths of 1, 6, 21 and 40 taps on both axes"""
    lib = orc_loader.load()
    ro, e = ref.descriptor(*case, seed=5, xtalk=xtalk)
    n, shape = ro.n_amps, (ro.n_amps, ro.raw_h, ro.raw_w)
    want = np.zeros(shape, dtype=np.float32)
    scratch = np.zeros(n * ro.seg_w * ro.seg_h, dtype=np.float32)
    lib.orc_readout_segments(e.ctypes.data, e.shape[1], e.shape[0], C.byref(ro), want.ctypes.data, scratch.ctypes.data)
    seg = ref.segments(e, ro)
    assert_bits_equal(seg, want, "segments")
    flips = {(ro.amps[a].flip_x, ro.amps[a].flip_y) for a in range(n)}
    assert len(flips) == min(n, 4) and ro.data_x0 > 0 and ro.data_y0 > 0 and ro.raw_w % 64 and ro.raw_h % 4
    if xtalk and n > 1:
        coef = np.array([ro.xtalk[i * 16 + j] for i in range(n) for j in range(n) if i != j])
        assert (coef == 0).any() and (coef != 0).any()
    if not xtalk:
        return
    src = ref.cte_input(seg, n)
    for n_band in ref.CTE_BANDS:
        for axis, cti in ((0, 2e-3), (1, 1e-3)):
            band = readout.cte_band(shape[1 + axis], cti, n_band - 1)
            dst = np.zeros(shape, dtype=np.float32)
            lib.orc_readout_cte(src.ctypes.data, dst.ctypes.data, C.byref(ro), band.ctypes.data, n_band, axis)
            got = ref.cte(src, band, axis)
            assert_bits_equal(got, dst, f"cte, {n_band} taps, axis {axis}")
            assert (got[:, -1, -1] != src[:, -1, -1]).all()
            assert np.allclose(got, ref.cte_dense(src, cti, axis, n_band - 1).astype(np.float32), rtol=ref.CTE_RTOL, atol=ref.CTE_ATOL)
    fin = (src - np.float32(2000.0)).astype(np.float32)
    out = np.zeros(shape, dtype=np.int32)
    lib.orc_readout_finish(fin.ctypes.data, C.byref(ro), 99, out.ctypes.data)
    mine = ref.finish(fin, ro, 99)
    assert_bits_equal(mine, out, "finish")
    assert (mine < 0).any() and (mine > 0).any()


# ---------------------------------------------------------------------------------------------
# refusals: the entry points check their arguments before the first HIP call
# ---------------------------------------------------------------------------------------------
class _Buffers:
    """valid, large enough memory for every pointer of a call: device memory where there is a device (a check that went missing
    would then launch on buffers of the documented sizes), host memory otherwise (nothing can launch)"""

    def __init__(self):
        import torch
        self.keep = []
        self.torch = torch if torch.cuda.is_available() else None

    def __call__(self, nbytes):
        if self.torch is not None:
            t = self.torch.zeros(nbytes, dtype=self.torch.uint8, device="cuda")
            self.keep.append(t)
            return t.data_ptr()
        a = np.zeros(nbytes, dtype=np.uint8)
        self.keep.append(a)
        return a.ctypes.data


def test_readout_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _abi.load()
    buf = _Buffers()
    good, e = ref.descriptor(*ref.SEGMENT_CASES[1], seed=1)
    ny, nx = e.shape
    n = good.n_amps * good.raw_w * good.raw_h
    img, seg, dst, out = buf(8 * nx * ny), buf(4 * n), buf(4 * n), buf(4 * n)
    band = buf(8 * 21 * max(good.raw_w, good.raw_h))

    def bad(**kw):
        ro = _abi.Readout.from_buffer_copy(bytes(good))
        for k, v in kw.items():
            setattr(ro, k, v)
        return ro

    def refused(code, word):
        assert code < 0 and word in lib.ims_last_error(), (code, lib.ims_last_error())

    def all_three(ro, word):
        refused(lib.ims_readout_segments(img, nx, ny, C.byref(ro), seg, None), word)
        refused(lib.ims_readout_cte(seg, dst, C.byref(ro), band, 21, 0, None), word)
        refused(lib.ims_readout_finish(seg, C.byref(ro), 1, out, None), word)

    all_three(bad(n_amps=0), b"n_amps")
    all_three(bad(n_amps=17), b"n_amps")
    all_three(bad(data_x0=good.raw_w - good.seg_w + 1), b"does not fit")
    all_three(bad(data_y0=good.raw_h - good.seg_h + 1), b"does not fit")
    all_three(bad(seg_w=0), b"does not fit")
    zero_gain = bad()
    zero_gain.amps[2].gain = 0.0
    all_three(zero_gain, b"gain")
    refused(lib.ims_readout_cte(seg, seg, C.byref(good), band, 21, 0, None), b"out of place")
    refused(lib.ims_readout_cte(seg, dst, C.byref(good), band, 0, 0, None), b"n_band")
    refused(lib.ims_readout_cte(seg, dst, C.byref(good), band, 21, 2, None), b"axis")
    refused(lib.ims_readout_cte(seg, dst, C.byref(good), None, 21, 0, None), b"NULL")
    outside = bad()
    outside.amps[2].x0 = nx - good.seg_w + 1
    refused(lib.ims_readout_segments(img, nx, ny, C.byref(outside), seg, None), b"outside the e-image")
    refused(lib.ims_readout_segments(img, nx, good.seg_h - 1, C.byref(good), seg, None), b"outside the e-image")
    flags = buf((nx * ny + 15) // 16 * 16 + 16 * nx)
    refused(lib.ims_readout_bleed(img, flags, 0, ny, 1e5, 1, None), b"empty image")
    refused(lib.ims_readout_bleed(img, flags, nx, 0, 1e5, 0, None), b"empty image")
    refused(lib.ims_readout_bleed(None, flags, nx, ny, 1e5, 0, None), b"NULL")
