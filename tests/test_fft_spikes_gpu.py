"""The spike step of the FFT branch (k_fft_bbox, k_fft_spike_table, k_fft_spikes, k_fft_spikes_stream, k_fft_spikes_arms) driven
straight through the C ABI on the planted cases of tests/spike_cases.py: arms along the axes, along the diagonals and in between,
sin0 == 0.0 exactly, a negative and a wide swept angle, a cutoff far above the grid, boxes of one pixel, on the last column, wider
than the stencil and as large as the stamp, objects without a box next to objects with one.  Every form of the step -- {compressed
table, stencil in place} x {one launch, listed} -- gives the same bits, the oracle's bits, and lies within the bounds of the
long-double statement of the operation (tests/spike_ref.py, which shares nothing with the kernels or the oracle and has no table);
the table itself is checked entry by entry against the reference's stencil."""
import ctypes as C
import math

import numpy as np
import pytest

import spike_cases as sc
import spike_ref as sr
from helpers import assert_bits_equal
from imsim_amd import _abi
from oracle import orc_loader

pytestmark = pytest.mark.gpu
LD = np.longdouble
_REF, _TABLES = {}, {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def reference(shape, geom):
    if (shape, geom) not in _REF:
        c = sc.case(shape, geom)
        _REF[shape, geom] = sr.apply(c.S, c.rows, c.rbuf)
    return _REF[shape, geom]


def oracle(S):
    from imsim_amd.engine import Scene
    orc = orc_loader.OracleFft(Scene(nx=64, ny=64, seed=1), [], add_noise=False)
    orc.P.spikes = S
    return orc


def build_table(torch, S, slack=8):
    """ims_fft_spike_table's two calls: (counts, row_ptr, col, val) as numpy arrays; col / val carry `slack` sentinel entries past
    the end that the second call must leave alone"""
    lib = _abi.load()
    rows = 2 * int(S.cutoff) + 1
    count = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    _abi.check(lib.ims_fft_spike_table(C.byref(S), None, count.data_ptr(), None, None, None), "ims_fft_spike_table")
    torch.cuda.synchronize()
    ptr = torch.zeros(rows + 1, dtype=torch.int32, device="cuda")
    ptr[1:] = torch.cumsum(count, 0).to(torch.int32)
    n = int(ptr[-1].item())
    col = torch.full((n + slack,), 99999, dtype=torch.int32, device="cuda")
    val = torch.full((n + slack,), -1.0, dtype=torch.float64, device="cuda")
    _abi.check(lib.ims_fft_spike_table(C.byref(S), ptr.data_ptr(), None, col.data_ptr(), val.data_ptr(), None), "ims_fft_spike_table")
    torch.cuda.synchronize()
    return count, ptr, col, val, n


def device_table(torch, geom, cutoff):
    """the table of a geometry on the device, made once (the tensors are kept alive here)"""
    if (geom, cutoff) not in _TABLES:
        _TABLES[geom, cutoff] = build_table(torch, sc.spikes(geom, cutoff))
    return _TABLES[geom, cutoff]


def run_step(torch, c, table, listed, rbuf=None, raw=0, list_cap=None):
    """one spike step through the C ABI: (image, bbox [n][4], listed count or None)"""
    lib = _abi.load()
    P = _abi.FftParams()
    P.spikes = c.S
    P.rbuf_raw = raw
    if table:
        _, ptr, col, val, _ = device_table(torch, c.geom, int(c.S.cutoff))
        P.spikes.tab_row, P.spikes.tab_col, P.spikes.tab_val = ptr.data_ptr(), col.data_ptr(), val.data_ptr()
    else:
        P.spikes.tab_row = P.spikes.tab_col = P.spikes.tab_val = None
    rows_t = torch.from_numpy(np.frombuffer(c.rows.tobytes(), dtype=np.uint8).copy()).cuda()
    pre_t = torch.from_numpy(c.prefix.copy()).cuda()
    rin = torch.from_numpy(np.array(c.rbuf if rbuf is None else rbuf, dtype=np.float64)).cuda()
    rout = torch.full_like(rin, -12345.0)
    n, n_pix = len(c.rows), int(c.prefix[-1])
    bbox = torch.full((4 * n,), 77, dtype=torch.int32, device="cuda")
    count = None
    if listed:
        cap = n_pix if list_cap is None else int(list_cap)
        lst = torch.zeros(cap, dtype=torch.int64, device="cuda")
        cnt = torch.full((1,), 1234567, dtype=torch.int32, device="cuda")
        _abi.check(lib.ims_fft_spikes_listed(C.byref(P), rows_t.data_ptr(), n, pre_t.data_ptr(), n_pix, rin.data_ptr(), rout.data_ptr(),
                                             bbox.data_ptr(), lst.data_ptr(), cap, cnt.data_ptr(), None), "ims_fft_spikes_listed")
        torch.cuda.synchronize()
        count = int(cnt.item())
    else:
        _abi.check(lib.ims_fft_spikes(C.byref(P), rows_t.data_ptr(), n, pre_t.data_ptr(), n_pix, rin.data_ptr(), rout.data_ptr(),
                                      bbox.data_ptr(), None), "ims_fft_spikes")
        torch.cuda.synchronize()
    assert_bits_equal(rin.cpu().numpy(), np.asarray(c.rbuf if rbuf is None else rbuf), "the step leaves its input alone")
    return rout.cpu().numpy(), bbox.cpu().numpy().reshape(n, 4).astype(np.int64), count


@pytest.mark.parametrize("cutoff", [20, 200])
@pytest.mark.parametrize("geom", list(sc.GEOMETRIES))
def test_spike_table_is_the_reference_stencil(torch_cuda, geom, cutoff):
    """ims_fft_spike_table, both calls: the counts are those of the stored rows, columns strictly descending inside [-cutoff,
    cutoff], the stored offsets are the reference's non-zero offsets (offsets within rounding of the cross's edge, or near a
    wedge decision, may be on either side), every value within the stencil bound of S / norm, nothing written past the end, a
    second build gives the same bits"""
    S = sc.spikes(geom, cutoff)
    count, ptr, col, val, n = (t.cpu().numpy() if hasattr(t, "cpu") else t for t in device_table(torch_cuda, geom, cutoff))
    assert count.shape == (2 * cutoff + 1,) and (count >= 0).all() and (count <= 2 * cutoff + 1).all()
    assert ptr[0] == 0 and (np.diff(ptr) >= 0).all() and ptr[-1] == n == count.sum()
    assert (col[n:] == 99999).all() and (val[n:] == -1.0).all(), "the second call wrote past row_ptr[2 cutoff + 1]"
    st = sr.stencil(sr.Geometry(S))
    stored = np.zeros((2 * cutoff + 1, 2 * cutoff + 1), dtype=bool)
    worst = 0.0
    for row in range(2 * cutoff + 1):
        b, v = col[ptr[row]:ptr[row + 1]].astype(np.int64), val[ptr[row]:ptr[row + 1]]
        assert (np.abs(b) <= cutoff).all() and (np.diff(b) < 0).all(), f"row {row - cutoff}: columns {b}"
        assert (v > 0).all()
        stored[row, b + cutoff] = True
        err, bound = np.abs(v.astype(LD) - st.Sn[row, b + cutoff]), st.bound[row, b + cutoff]
        assert (err <= bound).all(), f"row {row - cutoff}: values off by up to {float(np.max(err / bound))} bounds"
        if b.size:
            worst = max(worst, float(np.max(err / bound)))
    loose = st.edge | st.near
    assert np.array_equal(stored | loose, (st.S != 0) | loose), "the table's offsets are not the reference's non-zero offsets"
    assert n >= 4 * cutoff + 1
    if geom == "axis_exact":
        assert count[cutoff] == 2 * cutoff + 1 and (count[np.arange(2 * cutoff + 1) != cutoff] == 1).all()
    print(f"{geom}, cutoff {cutoff}: {n} entries, longest row {count.max()}, worst value error / bound {worst:.3g}")
    again = build_table(torch_cuda, S)
    for name, a, b in (("counts", count, again[0]), ("row_ptr", ptr, again[1]), ("columns", col, again[2]), ("values", val, again[3])):
        assert_bits_equal(a, b.cpu().numpy(), f"second build, {name}")


@pytest.mark.parametrize("shape,geom", sc.CASES, ids=[f"{s}/{g}" for s, g in sc.CASES])
def test_spike_step_in_every_form(torch_cuda, shape, geom):
    """{table, in place} x {one launch, listed}: the same bits, the oracle's bits, within the reference's bounds; pixels outside
    the stamp (and objects without a box) are the clipped input exactly (their bound is 0); the bbox scratch is the planted box"""
    c = sc.case(shape, geom)
    want, bound, boxes = reference(shape, geom)
    assert np.array_equal(boxes, c.boxes)
    if geom == "axis_exact":
        assert c.S.sin0 == 0.0
    oimage = oracle(c.S).spikes(c.rows, c.rbuf)
    first = None
    for table in (True, False):
        for listed in (False, True):
            what = f"{c.name}, {'table' if table else 'in place'}, {'listed' if listed else 'one launch'}"
            got, bbox, count = run_step(torch_cuda, c, table, listed)
            assert np.array_equal(bbox, c.boxes), f"{what}: bbox {bbox.tolist()}"
            if listed:
                assert 0 <= count <= int(c.prefix[-1]) and (count > 0) == bool((c.boxes[:, 1] >= c.boxes[:, 0]).any())
            if first is None:
                first = got
                ratio = sr.worst_ratio(got, want, bound)
                print(f"{c.name}: MI355X worst error / bound {ratio:.3g} (oracle {sr.worst_ratio(oimage, want, bound):.3g})")
                assert ratio <= 1.0
            assert_bits_equal(got, first, f"{what} vs table, one launch")
            assert_bits_equal(got, oimage, f"{what} vs the oracle")
    # (bound 0 outside the stamp: worst_ratio has compared those pixels exactly; said once more in plain words)
    outside = bound == 0
    assert_bits_equal(first[outside], np.clip(c.rbuf, 0, None)[outside], f"{c.name}: pixels the step may only clip")
    assert (first != np.clip(c.rbuf, 0, None)).any()


def test_listed_form_at_the_boundaries_of_its_list(torch_cuda):
    """count == cap (the list just holds: the arms kernel does the sums), count == cap + 1 and a list of 64 (it runs over: entries
    beyond the cap are not written, the arms kernel returns, the one-launch kernel does the whole step): the same bits every time"""
    c = sc.case("clip64", "generic")
    want, _, count = run_step(torch_cuda, c, True, True)
    assert count > 65
    for table in (True, False):
        for cap in (count, count - 1, 64):
            got, bbox, n = run_step(torch_cuda, c, table, True, list_cap=cap)
            assert n == count, "the counter counts every arm pixel, whatever the list holds"
            assert (n <= cap) == (cap == count)
            assert_bits_equal(got, want, f"list of {cap} entries for {count} arm pixels, {'table' if table else 'in place'}")
            assert np.array_equal(bbox, c.boxes)


def test_raw_buffer_is_scaled_as_promised(torch_cuda):
    """rbuf_raw = 1 on five objects of grids 32, 64, 32, 96, 32 (1 / 96^2 is no power of two): within the bounds of the reference
    fed the raw buffer, and the bits of the oracle fed fl64(raw fl64(1 / n^2))"""
    c = sc.case("batch", "generic")
    raw, image = sc.raw_buffer(c)
    assert not np.array_equal(image, c.rbuf)
    want, bound, boxes = sr.apply(c.S, c.rows, raw, raw=True)
    assert np.array_equal(boxes, c.boxes)
    oimage = oracle(c.S).spikes(c.rows, image)
    for table in (True, False):
        for listed in (False, True):
            got, bbox, _ = run_step(torch_cuda, c, table, listed, rbuf=raw, raw=1)
            ratio = sr.worst_ratio(got, want, bound)
            print(f"raw {c.name}, table {table}, listed {listed}: worst error / bound {ratio:.3g}")
            assert ratio <= 1.0
            assert_bits_equal(got, oimage, "raw buffer vs the oracle on the scaled image")
            assert np.array_equal(bbox, c.boxes)


def _drawn_rows():
    """four bright objects on a 256 x 256 CCD (the rows of the parity tests' FFT case)"""
    from imsim_amd import configs, catalog, fft_draw
    scene = configs.scene_c2(nx=256, ny=256)
    cat = dict(x=np.array([100.3, 60.0, 180.6, 128.5]), y=np.array([120.7, 200.2, 70.1, 40.9]), mag=np.zeros(4),
               nominal_flux=np.array([2.0e6, 5.0e6, 1.5e6, 3.0e6]), kind=np.array([0, 1, 2, 0]),
               hlr=np.array([0.0, 0.4, 0.8, 0.0]), q=np.array([1.0, 0.5, 0.8, 1.0]), pa=np.array([0.0, 30.0, 110.0, 0.0]),
               obj_id=np.arange(4))
    objects, _ = catalog.build_object_table(cat, cat["nominal_flux"].astype(np.int64), stamp_size=np.array([64, 128, 96, 48]))
    fwhm_atm, fwhm_sys = catalog.kolmogorov_gaussian_fwhm()
    rows, _ = fft_draw.build_fft_objects(objects, cat["nominal_flux"], objects["prof_table"])
    rows = rows.copy()
    rows["flux"] *= 20.0                                   # peaks well above the 1e5 threshold
    return scene, rows, fft_draw.kolmogorov_gaussian_kpsf(fwhm_atm, fwhm_sys)


def test_driver_path_with_arms_along_the_axes(torch_cuda, monkeypatch):
    """FftDrawer.draw at rotTelPos = pi/4 (alpha = 0: arms along rows and columns, table rows of 2 cutoff + 1 entries), exptime
    30 s, in both forms of the spike step: the oracle's bits on the GPU's own transforms"""
    from imsim_amd import fft_draw, diffraction_fft as dfft
    from imsim_amd.engine import Renderer
    scene, rows, kpsf = _drawn_rows()
    cfg = dfft.DiffractionFFT(exptime=30.0, azimuth=math.radians(114.39), altitude=math.radians(53.16), rotTelPos=math.pi / 4,
                              spike_length_cutoff=60)
    images = []
    for listed in ("1", "0"):
        monkeypatch.setenv("IMS_FFT_SPIKE_LIST", listed)
        r = Renderer(scene)
        drawer = fft_draw.FftDrawer(r, kpsf, add_noise=False, diffraction_fft=cfg, wavelength=622.2)
        _, rbuf = drawer.draw(rows)
        r.synchronize()
        assert (drawer._last[7] is not None) == (listed == "1")
        final = drawer._last[2].cpu().numpy().copy()
        image = fft_draw.image_from_rbuf(rows, rbuf.cpu().numpy())
        orc = orc_loader.OracleFft(scene, kpsf, add_noise=False, diffraction_fft=cfg, wavelength=622.2)
        assert_bits_equal(final, orc.spikes(rows, image), f"spiked images at rotTelPos = pi/4, IMS_FFT_SPIKE_LIST={listed}")
        assert np.abs(final - np.clip(image, 0, None)).max() > 1.0
        images.append(final)
    assert_bits_equal(images[0], images[1], "listed vs one launch")
