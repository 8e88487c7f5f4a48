"""The Poisson deviate on the GPU, through the entry points that consume it, against tests/noise_deviate_ref.py (plain numpy,
np.longdouble, mpmath's log Gamma): draw for draw apart from the reference's own near ties, and against the exact law.  Also
the bits of the log Gamma probe and the law of the read-noise Gaussian.  The CPU half is tests/test_noise_deviates.py."""
import numpy as np
import pytest

import noise_deviate_cases as K
import noise_deviate_ref as R
from imsim_amd import _abi
from helpers import assert_bits_equal

pytestmark = pytest.mark.gpu

ITERATION = 5
START = 1000.0                                   # the image is added to: it starts from a non-zero integer image


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _start_image(ny, nx):
    return START + (np.arange(ny * nx, dtype=np.float64) % 7.0).reshape(ny, nx)


def _flat_add(torch, base, level, iteration, nx, ny, area=None, inv_mean_area=1.0, with_delta=False, seed=K.SEED):
    """ims_flat_add on a fresh image; returns (image - start, delta or None) as numpy"""
    lib = _abi.load()
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a, dtype=np.float64)).cuda()       # a copy: inputs stay as they are
    start = _start_image(ny, nx)
    img, b, ar = dev(start), dev(base), dev(area)
    delta = torch.full(((ny + 1) * (nx + 1),), -3.0, dtype=torch.float64, device="cuda") if with_delta else None
    _abi.check(lib.ims_flat_add(ar.data_ptr() if ar is not None else None, b.data_ptr() if b is not None else None, float(level),
                                float(inv_mean_area), int(seed), int(iteration), nx, ny, img.data_ptr(),
                                delta.data_ptr() if delta is not None else None, None), "ims_flat_add")
    torch.cuda.synchronize()
    return img.cpu().numpy() - start, (delta.cpu().numpy().reshape(ny + 1, nx + 1) if delta is not None else None)


@pytest.fixture(scope="module")
def flat_case():
    """the mean map of the 1000 x 1049 image and the reference's draws of it, computed once and left unchanged"""
    base, bands = K.flat_base()
    mean = np.float64(K.FLAT_LEVEL) * base
    ref = R.poisson_ref(mean, K.SEED, K.FLAT_ID_BASE + ITERATION, np.arange(mean.size).reshape(mean.shape))
    for a in (base, mean) + ref:
        a.setflags(write=False)
    return base, bands, mean, ref


def test_flat_add_equals_the_restatement_and_follows_the_law(torch_cuda, flat_case):
    base, bands, mean, ref = flat_case
    nx, ny = K.FLAT_NX, K.FLAT_NY
    assert (nx * ny) % 256 != 0                                    # the last workgroup is partial
    got, _ = _flat_add(torch_cuda, base, K.FLAT_LEVEL, ITERATION, nx, ny)
    # equality, band by band (the share of near ties is capped per case), then the rows below the bands
    rows = dict(bands)
    rows["ramp, edge row and the rest"] = slice(len(K.LAW_MEANS) * K.BAND, ny)
    for name, sl in rows.items():
        share = R.assert_equal_apart_from_ties(got[sl], None, None, None, None, f"flat band {name}", ref=(ref[0][sl], ref[1][sl]))
        print(f"near-tie share, band {name}: {share:.3g}")
    # the edge row: the values the spec gives whatever the uniforms are
    edge_row = got[len(K.LAW_MEANS) * K.BAND + K.BAND]
    for j, (m, want) in enumerate(K.EDGE_MEANS):
        if want is not None:
            assert np.all(edge_row[j::len(K.EDGE_MEANS)] == want), f"edge mean {m}"
    # the law on the bands' own counts
    for m, sl in bands.items():
        p = R.law_pvalue(got[sl], mean[sl][0, 0])
        print(f"law p-value of the band at mean {m}: {p:.3g}")
        assert p >= R.P_PASS


def test_flat_add_fills_delta_with_its_own_stride(torch_cuda, flat_case):
    base, _, _, ref = flat_case
    nx, ny = K.FLAT_NX, K.FLAT_NY
    got, delta = _flat_add(torch_cuda, base, K.FLAT_LEVEL, ITERATION, nx, ny, with_delta=True)
    assert np.all(delta[:, nx] == -3.0) and np.all(delta[ny, :] == -3.0)          # last column and last row untouched
    assert np.array_equal(delta[:ny, :nx] + 3.0, got)
    R.assert_equal_apart_from_ties(got, None, None, None, None, "flat with delta", ref=ref)


def test_flat_add_with_pixel_areas(torch_cuda):
    """mean = level * base[p] * (area[p] * inv_mean_area), in that order; 301 x 41 = 48 workgroups + 53 pixels"""
    nx, ny = 301, 41
    n = nx * ny
    base = K.ramp(n).reshape(ny, nx) / K.FLAT_LEVEL
    area = 1.0 + 0.01 * np.sin(np.arange(n, dtype=np.float64)).reshape(ny, nx)
    inv = 1.0 / 1.003
    mean = (np.float64(K.FLAT_LEVEL) * base) * (area * np.float64(inv))
    got, _ = _flat_add(torch_cuda, base, K.FLAT_LEVEL, 2, nx, ny, area=area, inv_mean_area=inv)
    R.assert_equal_apart_from_ties(got, mean, K.SEED, K.FLAT_ID_BASE + 2, np.arange(n).reshape(ny, nx), "flat with areas")


@pytest.mark.parametrize("stream_id", (0, 3))
def test_add_noise_draws_from_its_mean_map(torch_cuda, stream_id):
    """LsstImage.add_noise with a gradient and a multiplier map on 255 x 142, against the mean map restated from the inputs"""
    from imsim_amd import configs, lsst_image
    from imsim_amd.engine import Renderer
    nx, ny = 255, 142
    r = Renderer(configs.scene_c2(nx=nx, ny=ny))
    grad = (0.95, 0.0005, -0.0002)
    mult = 1.0 + 0.1 * np.cos(np.arange(ny)[:, None] / 20.0) * np.ones((ny, nx))
    sky = 900.0
    lsst_image.LSST_ImageBuilder().add_noise(r, sky_level=sky, sky_gradient=grad, multiplier=mult, seed=99, stream_id=stream_id)
    r.synchronize()
    got = r.image.cpu().numpy().astype(np.float64).reshape(ny, nx)
    xx, yy = np.arange(nx, dtype=np.float64)[None, :], np.arange(ny, dtype=np.float64)[:, None]
    base = (1.0 * (grad[0] + grad[1] * xx + grad[2] * yy)) * mult
    mean = np.float64(sky * 0.2 * 0.2) * base
    R.assert_equal_apart_from_ties(got, mean, 99, K.FLAT_ID_BASE + lsst_image.NOISE_STREAM + stream_id,
                                   np.arange(nx * ny).reshape(ny, nx), f"sky noise, stream {stream_id}")


def _dev_math(torch, which, x, n=None, seed=0, obj=0, slot=0):
    lib = _abi.load()
    xin = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    n = xin.numel() if n is None else n
    out = torch.empty(n * (2 if which == 6 else 1), dtype=torch.float64, device="cuda")
    _abi.check(lib.ims_test_math(which, xin.data_ptr(), out.data_ptr(), n, seed, obj, slot, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_lgamma_probe_has_the_oracles_bits(torch_cuda):
    from oracle import orc_loader
    from test_noise_deviates import _lgamma_points, lgamma_worst_ratio
    x = _lgamma_points()
    got = _dev_math(torch_cuda, 13, x)
    assert_bits_equal(got, orc_loader.math_probe(13, x), "lgamma")
    ratio = lgamma_worst_ratio(got)
    print(f"lgamma on the device: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_read_noise_gaussian_follows_the_normal_law(torch_cuda):
    from oracle import orc_loader
    n = K.N_LAW // 2
    g = _dev_math(torch_cuda, 6, np.zeros(1), n=n, seed=K.SEED, obj=K.READOUT_ID_BASE + 3, slot=0)
    p = R.normal_pvalue(g)
    print(f"read noise on the device: p-value of 2^20 deviates over 64 equiprobable bins {p:.3g}")
    assert p >= R.P_PASS
    assert_bits_equal(g, orc_loader.gauss_probe(K.SEED, K.READOUT_ID_BASE + 3, n, 0), "gaussian pairs")


# ---------------------------------------------------------------------------------------------
# the other consumers, each against a mean map restated in numpy from the inputs alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dark_current", (0.02, 1.0), ids=["multiplication", "ptrs"])
def test_readout_dark_current(torch_cuda, dark_current):
    """CcdReadout on the first toy geometry of readout_ref (e-image 536 x 62, not a multiple of 256): the e-image after
    build_amp_images is the bled image plus a deviate of dark_current * (exptime + readout_time) per pixel, stream DARK_STREAM,
    under the CCD's seed.  The bled image is the oracle's bleed_eimage, which tests/golden/readout_golden.npz pins to the
    reference; the dark step is the restatement's.  Means 0.64 and 32: one per branch of the deviate."""
    from imsim_amd import readout
    from oracle import orc_loader
    import readout_ref as ref
    seed = 20261017
    ccd, ro = ref.toy_readout(ref.SHAPES[0], dark_current=dark_current)
    e, _ = ref.toy_eimage(ccd, seed)
    ny, nx = e.shape
    assert (nx * ny) % 256 != 0
    ro.eimage.array = torch_cuda.from_numpy(e.copy()).cuda()
    ro.build_amp_images(seed)
    torch_cuda.cuda.synchronize()
    bled = orc_loader.bleed_eimage(e, ro.full_well, ro.midline_stop())
    assert (bled != e).any()
    level = dark_current * (30.0 + 2.0)                            # eimage_header(det, 30.0), readout_time 2.0
    assert level == ro.dark_level()
    got = ro.eimage.array.cpu().numpy() - bled                     # integers below 2^53: the difference is exact
    R.assert_equal_apart_from_ties(got, np.float64(level), seed, K.FLAT_ID_BASE + (1 << 20) + 7,
                                   np.arange(nx * ny).reshape(ny, nx), f"dark current {dark_current}")
    assert readout.DARK_STREAM == (1 << 20) + 7
    p = R.law_pvalue(got, level)
    print(f"dark current, mean {level}: law p-value {p:.3g}")
    assert p >= R.P_PASS


def test_device_table_realises_photon_counts(torch_cuda):
    """DeviceTable(..., phot_flux=None) on the edge catalog: n_phot is the deviate of the nominal flux at (seed, obj_id, pixel
    IMS_FLUX_PIXEL = -7), truncated to an integer; every third object id lies above 2^32"""
    from imsim_amd.device_table import DeviceTable
    from imsim_amd.engine import Renderer
    from test_device_table import _edge_catalog, VISIT
    scene, cat = _edge_catalog()
    ids = np.asarray(cat["obj_id"], dtype=np.int64).copy()
    ids[::3] += K.CATALOG_ID_HIGH
    cat["obj_id"] = ids
    t = DeviceTable(Renderer(scene), cat, VISIT, phot_flux=None)
    torch_cuda.cuda.synchronize()
    assert _abi.IMS_FLUX_PIXEL == -7
    nominal = np.asarray(cat["nominal_flux"], dtype=np.float64)
    ref = R.poisson_ref(nominal, scene.seed, ids, np.full(len(ids), -7, dtype=np.int64))
    assert not ref[1].any()                                        # 400 draws: one near tie would be 25 times the cap
    R.assert_equal_apart_from_ties(np.asarray(t.n_phot, dtype=np.float64), None, None, None, None, "n_phot", ref=ref)
    assert np.array_equal(t.meta["n_phot"], ref[0].astype(np.int64)) and t.n_phot[0] == 0 and t.n_phot[17] > 9e8
    # the ids matter: the same catalog with the low ids draws other counts for the objects that moved
    moved = R.poisson_ref(nominal, scene.seed, np.asarray(ids) & 0xFFFFFFFF, np.full(len(ids), -7, dtype=np.int64))[0]
    assert (moved[::3] != ref[0][::3]).sum() > len(ids) // 6 and np.array_equal(moved[1::3], ref[0][1::3])


def test_fft_drawn_object_noise_step(torch_cuda):
    """One point source through a Gaussian PSF on a 32 x 32 grid (sixteen wavefronts; a wavefront holds two rows), wholly on
    a 64 x 48 CCD.  add_noise off: the CCD holds the clipped stamp.  On: every pixel is the deviate of the clipped noise-free
    pixel at (obj_id, local pixel iy * 32 + ix), and the realised flux is the noise-free sum."""
    import fft_closed_forms as cf
    from imsim_amd import configs, fft_draw
    from test_fft_edges_gpu import draw, gaussian_kpsf
    nx, ny, n, x0, y0 = 64, 48, 32, 11, 9
    obj_id = K.CATALOG_ID_HIGH + 12
    rows = cf.make_rows([dict(nfft=n, x0=x0, y0=y0, cx=15.3, cy=16.4, flux=3.0e4, obj_id=obj_id)])
    out = {}
    for noise in (False, True):
        scene = configs.scene_c2(nx=nx, ny=ny)
        r, drawer, _, image, real = draw(torch_cuda, scene, gaussian_kpsf(0.3), rows, add_noise=noise)
        out[noise] = (r.image64_numpy(), np.where(image < 0.0, 0.0, image).reshape(n, n), real, scene)
    ccd, clipped, real, scene = out[False]
    cx, cy = x0 - scene.xmin, y0 - scene.ymin
    want = np.zeros((ny, nx))
    want[cy:cy + n, cx:cx + n] = clipped
    assert_bits_equal(ccd, want, "CCD image without noise")
    noisy, clipped_on, real_on, scene = out[True]
    assert_bits_equal(clipped_on, clipped, "the noise-free stamp does not depend on the noise switch")
    assert clipped.max() > 1000.0 and 0.0 < clipped[clipped > 0].min() < 10.0     # both branches of the deviate, and zeros' neighbours
    stamp = noisy[cy:cy + n, cx:cx + n]
    R.assert_equal_apart_from_ties(stamp, clipped, scene.seed, obj_id, np.arange(n * n).reshape(n, n), "FFT noise step")
    outside = noisy.copy()
    outside[cy:cy + n, cx:cx + n] = 0.0
    assert not outside.any()
    np.testing.assert_allclose(real_on, [clipped.sum()], rtol=1.0e-12)
    np.testing.assert_allclose(real, [clipped.sum()], rtol=1.0e-12)
