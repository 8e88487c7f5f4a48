"""FFT-drawn RandomKnots on the GPU (stamp.fft_knots): ims_knot_positions against the photon path's knots, ims_fft_knots_factor against
the extended-precision sum of tests/knots_closed_forms.py, the drawn images against the erf closed form, and the bits of every other
object of a batch.  Pixel scale 0.2", no noise, no spikes, n_alias 0.  Grids of 32 and 64; knot counts 1, 2, 7, 65 and 257 (one knot,
a pair, less than a chunk of the kernel, and across its chunk and wavefront boundaries).

Measured on an MI355X (every test prints its figures before it asserts, pytest -s; EXPERIMENTS.md, "FFT-drawn RandomKnots"):
    structure factor against the longdouble sum: 9.2e-16 on 32 (bound 1.8e-13), 1.5e-15 on 64 (bound 3.6e-13)
    images against the erf form, per unit flux: N = 2 7.3e-17, N = 7 3.9e-17, N = 65 2.4e-17 (allowed 1.0e-13)
    N = 1 against the moved point: 2.9e-11 at a peak of 4.9e4 (allowed 8.9e-9)"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from helpers import assert_bits_equal
from imsim_amd import _abi, configs, fft_draw
import fft_closed_forms as cf
import knots_closed_forms as kc
import photon_source_cases as cases
import streak_closed_forms as sf
from test_fft_closed_forms import ROUNDING

pytestmark = pytest.mark.gpu

PS = cf.PIXEL_SCALE
SIGMA_PSF = cf.POINT_SIGMAS[0]                       # 0.5": n_alias 0, the Gaussian-PSF point case of tests/test_fft_closed_forms.py
KPSF = [(_abi.IMS_KPSF_GAUSSIAN, 0, SIGMA_PSF)]
COUNTS = (1, 2, 7, 65, 257)
JACS = ((0.9, 0.3, -0.2, 0.7), (0.5, 0.8, 0.7, -0.4))        # anisotropic; the second has a negative determinant
SEED = cases.SEED


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _side(rows, n_knots, sigma):
    n_knots = np.asarray(n_knots, dtype=np.int32)
    return n_knots, np.where(n_knots > 0, sigma, 0.0).astype(np.float64), np.concatenate([[0], np.cumsum(n_knots, dtype=np.int64)])[:-1]


def _positions(torch, rows, knots, seed=SEED):
    """ims_knot_positions alone -> [total knots][2] on the host"""
    lib = _abi.load()
    dev = "cuda"
    obj_t = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()).to(dev)
    n_t, s_t, o_t = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in knots)
    xy = torch.full((2 * int(knots[0].sum()),), float("nan"), dtype=torch.float64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _abi.check(lib.ims_knot_positions(int(seed), obj_t.data_ptr(), len(rows), n_t.data_ptr(), s_t.data_ptr(), o_t.data_ptr(),
                                      xy.data_ptr(), st), "ims_knot_positions")
    torch.cuda.synchronize()
    return xy.cpu().numpy().reshape(-1, 2)


def _draw(torch, rows, knots=None, scene=None):
    """one noiseless draw -> (renderer, drawer, [half spectrum per row], [image per row])"""
    from imsim_amd.engine import Renderer
    sc = scene or configs.scene_c2(nx=256, ny=256)
    sc.seed = SEED
    r = Renderer(sc)
    drawer = fft_draw.FftDrawer(r, KPSF, add_noise=False)
    assert drawer.P.n_alias == 0 and not drawer.P.spikes.enabled
    drawer.keep_kspace = True
    kbuf, rbuf = drawer.draw(rows, knots=knots)
    r.synchronize()
    k = kbuf.cpu().numpy()
    spectra = [k[int(o["k_offset"]):int(o["k_offset"]) + int(o["nfft"]) * (int(o["nfft"]) // 2 + 1)].reshape(int(o["nfft"]), -1)
               for o in rows]
    return r, drawer, spectra, cf.grids(rows, fft_draw.image_from_rbuf(rows, rbuf.cpu().numpy()))


@pytest.mark.parametrize("n", [7, 37])
def test_knot_positions_are_the_photon_paths(torch_cuda, n):
    """photons of a knots object without a PSF, jac and winv the identity, the object at the origin: every photon sits ON a knot, in
    pixels; ims_knot_positions with the identity for jac' gives the same numbers, bit for bit.  4000 photons per knot: the chance
    that one of 37 knots is never picked is 37 exp(-4000)."""
    from imsim_amd.engine import Renderer
    o = cases.rows(1, first=[0], ids=[2 ** 32 + 5], n_phot=[4000 * n])
    o["prof_table"], o["prof_aux"], o["prof_scale"] = _abi.IMS_PROF_KNOTS, n, 0.45
    o["jac"][0] = o["winv"][0] = (1.0, 0.0, 0.0, 1.0)
    o["x0"] = o["y0"] = 0.0
    r = Renderer(cases._scene([]))
    pool = r.shoot_photons(o)
    r.synchronize()
    got = pool.to_host()
    seen = np.unique(np.stack([got["x"], got["y"]], axis=1).view(np.uint64), axis=0)
    rows = cf.make_rows([dict(nfft=32, x0=0, y0=0, cx=16.0, cy=16.0, flux=1.0, obj_id=2 ** 32 + 5)])
    d = _positions(torch_cuda, rows, _side(rows, [n], 0.45))
    want = np.unique(d.view(np.uint64), axis=0)
    assert len(want) == n, "two knots at one place?"
    assert len(seen) == n, f"{len(seen)} distinct photon positions for {n} knots"
    assert_bits_equal(seen, want, "knot positions")
    assert np.isfinite(d).all() and 0.5 * 0.45 < d.std() < 2.0 * 0.45


def _factor_rows():
    """every knot count on both grids with both affines; a point row in between that the pass must not touch"""
    specs, n_knots = [], []
    for nfft in (32, 64):
        for k, n in enumerate(COUNTS):
            specs.append(dict(nfft=nfft, x0=0, y0=0, cx=nfft / 2.0, cy=nfft / 2.0, flux=1.0, obj_id=100 * nfft + n, jac=JACS[k % 2]))
            n_knots.append(n)
        specs.append(dict(nfft=nfft, x0=0, y0=0, cx=3.0, cy=4.0, flux=1.0, obj_id=nfft))
        n_knots.append(0)
    return cf.make_rows(specs), n_knots


@pytest.fixture(scope="module")
def factors(torch_cuda):
    """the pass over a buffer of ones: (1 + 0 i) S is S, bit for bit -> (rows, n_knots, positions, [S per row])"""
    torch = torch_cuda
    lib = _abi.load()
    rows, n_knots = _factor_rows()
    sigma = 0.3                      # |d| <= 4.5 sigma (|j0| + |j1|) = 1.76" < 3.2" = half the smaller grid
    knots = _side(rows, n_knots, sigma)
    d = _positions(torch, rows, knots)
    dev = "cuda"
    obj_t = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()).to(dev)
    n_t, _, o_t = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in knots)
    which = np.flatnonzero(knots[0] > 0).astype(np.int32)
    w_t = torch.from_numpy(which).to(dev)
    xy = torch.from_numpy(d.reshape(-1).copy()).to(dev)
    total = int(sum(int(o["nfft"]) * (int(o["nfft"]) // 2 + 1) for o in rows))
    kbuf = torch.ones(total, dtype=torch.complex128, device=dev)
    P = _abi.FftParams()
    P.pixel_scale, P.n_alias = PS, 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _abi.check(lib.ims_fft_knots_factor(C.byref(P), obj_t.data_ptr(), w_t.data_ptr(), len(which), int(rows["nfft"].max()), n_t.data_ptr(),
                                        o_t.data_ptr(), xy.data_ptr(), kbuf.data_ptr(), st), "ims_fft_knots_factor")
    torch.cuda.synchronize()
    k = kbuf.cpu().numpy()
    S = [k[int(o["k_offset"]):int(o["k_offset"]) + int(o["nfft"]) * (int(o["nfft"]) // 2 + 1)].reshape(int(o["nfft"]), -1) for o in rows]
    return rows, knots, d, S


def test_structure_factor_is_the_extended_precision_sum(factors):
    rows, knots, d, S = factors
    worst = {}
    for o, n, at, got in zip(rows, knots[0], knots[2], S):
        nfft = int(o["nfft"])
        if n == 0:
            assert_bits_equal(got.view(np.float64), np.ones_like(got).view(np.float64), "a row without knots")
            continue
        dm = d[at:at + n]
        assert np.abs(dm).max() <= 0.5 * nfft * PS, "a knot outside the grid: the bound's premise"
        re, im = kc.S_ref(dm, nfft, PS)
        err = float(max(np.abs(got.real.astype(np.longdouble) - re).max(), np.abs(got.imag.astype(np.longdouble) - im).max()))
        print(f"grid {nfft} N {n} det {'-' if o['jac'][0] * o['jac'][3] < o['jac'][1] * o['jac'][2] else '+'}: "
              f"S misses the longdouble sum by {err:.3e}, allowed {kc.factor_bound(nfft):.3e}")
        assert err <= kc.factor_bound(nfft)
        worst[nfft] = max(worst.get(nfft, 0.0), err)
    print("largest deviation per grid:", {n: f"{v:.3e}" for n, v in worst.items()})
    assert sorted(worst) == [32, 64] and min(worst.values()) > 0.0
    assert any(o["jac"][0] * o["jac"][3] < o["jac"][1] * o["jac"][2] for o in rows)


def test_exact_anchors(torch_cuda, factors):
    rows, knots, d, S = factors
    for n, got in zip(knots[0], S):
        if n == 0:
            continue
        dc = got[0, 0]
        if n & (n - 1) == 0:
            assert dc == 1.0 + 0.0j, f"S(0, 0) for N = {n}"
        else:
            assert abs(dc.real - 1.0) <= kc.EPS and dc.imag == 0.0, f"S(0, 0) for N = {n}"
    # the DC term of a knots object is the point's
    spec = dict(nfft=32, x0=20, y0=30, cx=15.3, cy=16.6, flux=2.0e6, obj_id=77, jac=JACS[0])
    rows1 = cf.make_rows([spec])
    for n in (1, 2, 7):
        _, drawer, sk, _ = _draw(torch_cuda, rows1, _side(rows1, [n], 0.3))
        _, plain, sp, _ = _draw(torch_cuda, rows1)
        assert drawer.knot_launches == 1 and plain.knot_launches == 0
        assert abs(sk[0][0, 0] - sp[0][0, 0]) <= kc.EPS * abs(sp[0][0, 0])
    # N = 1: the point branch with its centre moved by d_0 / pixel_scale
    k1 = _side(rows1, [1], 0.3)
    d0 = _positions(torch_cuda, rows1, k1)[0]
    _, _, _, ik = _draw(torch_cuda, rows1, k1)
    moved = cf.make_rows([dict(spec, cx=spec["cx"] + d0[0] / PS, cy=spec["cy"] + d0[1] / PS)])
    _, _, _, ip = _draw(torch_cuda, moved)
    err, peak = float(np.abs(ik[0] - ip[0]).max()), float(ip[0].max())
    print(f"N = 1 against the moved point: {err:.3e}, peak {peak:.3e}, allowed {kc.factor_bound(32) * peak:.3e}")
    assert abs(d0).max() > 0.01 and err <= kc.factor_bound(32) * peak


@pytest.mark.parametrize("n", [2, 7, 65])
def test_image_is_the_erf_closed_form(torch_cuda, n):
    """one Gaussian PSF (sigma 0.5"), a sheared jac'; the Gaussian-PSF point case's tolerance (tests/test_fft_closed_forms.py): the
    bound on the aliases left out plus ROUNDING, per unit flux.  The numpy restatement of the branch meets it with three decades to
    spare (tests/test_fft_knots.py prints 1.0e-16 against 1.0e-13), so it is not widened.  Knots at least 8 PSF sigmas inside the grid
    (the issue's 4 and more): the closed form is not periodic, and beyond 8 sigma a Gaussian holds 6e-16 of its flux."""
    flux, nfft, cx, cy = 3.0e6, 64, 31.4, 30.7
    rows = cf.make_rows([dict(nfft=nfft, x0=40, y0=50, cx=cx, cy=cy, flux=flux, obj_id=900 + n, jac=JACS[0])])
    knots = _side(rows, [n], 0.3)
    d = _positions(torch_cuda, rows, knots)
    margin = kc.margin_in_sigmas(nfft, cx, cy, d, SIGMA_PSF, PS)
    assert margin >= 8.0 >= 4.0, margin
    _, _, _, images = _draw(torch_cuda, rows, knots)
    want = kc.image_ref(nfft, cx, cy, d, SIGMA_PSF, PS, flux)
    tol = (cf.omitted_alias_bound(SIGMA_PSF, nfft, 0, PS) + ROUNDING) * flux
    err = float(np.abs(images[0] - want).max())
    print(f"N {n}: image misses the erf form by {err / flux:.3e} per unit flux, allowed {tol / flux:.3e}; margin {margin:.1f} sigma")
    assert err <= tol
    # and it is not the point's image: the knots are resolved
    assert float(np.abs(kc.image_ref(nfft, cx, cy, [[0.0, 0.0]], SIGMA_PSF, PS, flux) - want).max()) > (1.0e3 * tol if n > 1 else 0.0)


def _mixed(with_knots):
    """The box sits in FRONT of the knots rows: k_fft_kspace_fill forms a box from its LDS tables only in workgroups whose span lies
    inside the one object, so a box's own bits depend on where its half spectrum starts in the buffer -- with or without this pass."""
    specs = [dict(nfft=32, cx=15.37, cy=16.81, flux=2.0e6, x0=10, y0=12, obj_id=1),
             dict(nfft=32, cx=15.9, cy=16.3, flux=2.5e6, x0=150, y0=150, obj_id=4, prof_ktable=-2, jac=sf.box_jac(3.0, 0.6, 90.0)),
             dict(nfft=64, cx=31.4, cy=30.7, flux=3.0e6, x0=60, y0=70, obj_id=2, prof_ktable=0, prof_scale=0.3, jac=sf.box_jac(1.0, 0.5, 37.0))]
    n_knots = [0, 0, 0]
    if with_knots:
        specs.insert(2, dict(nfft=32, cx=16.2, cy=15.1, flux=1.5e6, x0=150, y0=20, obj_id=3, jac=JACS[0]))
        specs.append(dict(nfft=64, cx=32.2, cy=31.1, flux=1.0e6, x0=100, y0=20, obj_id=5, jac=JACS[1]))
        n_knots = [0, 0, 7, 0, 65]
    rows = cf.make_rows(specs)
    return rows, _side(rows, n_knots, 0.3)


def test_knots_in_the_batch_leave_the_other_objects_bits_alone(torch_cuda):
    """a point, a box, knots, a Sersic and knots on grids of 32, 32, 32, 64, 64 -- and the same batch without the knots rows"""
    (both, kb), (plain, kp) = _mixed(True), _mixed(False)
    assert list(both["obj_id"]) == [1, 4, 3, 2, 5] and list(plain["obj_id"]) == [1, 4, 2]
    _, drawer, s2, i2 = _draw(torch_cuda, both, kb)
    assert drawer.knot_launches == 1
    r0, none, s1, i1 = _draw(torch_cuda, plain, kp)
    assert none.knot_launches == 0 and none._last[8] is None                     # no knots object: nothing is launched
    r1, bare, s0, i0 = _draw(torch_cuda, plain)                                   # ... and the draw is the one without side arrays
    assert bare.knot_launches == 0
    assert_bits_equal(r0.image64_numpy(), r1.image64_numpy(), "CCD image of the batch without knots")
    for a, b in ((0, 0), (1, 1), (3, 2)):
        assert_bits_equal(s2[a].view(np.float64), s1[b].view(np.float64), f"half spectrum of object {int(both['obj_id'][a])}")
        assert_bits_equal(i2[a], i1[b], f"image of object {int(both['obj_id'][a])}")
        assert_bits_equal(s1[b].view(np.float64), s0[b].view(np.float64), f"half spectrum of object {int(both['obj_id'][a])}, no side arrays")
    # the knots rows of the mixed batch are what they are alone
    for a in (2, 4):
        alone = cf.make_rows([{f: both[a][f] for f in ("nfft", "x0", "y0", "cx", "cy", "flux", "obj_id", "jac")}])
        _, _, sa, ia = _draw(torch_cuda, alone, _side(alone, [kb[0][a]], 0.3))
        assert_bits_equal(s2[a].view(np.float64), sa[0].view(np.float64), f"half spectrum of knots object {int(both['obj_id'][a])}")


def test_a_knots_stamp_clipped_by_the_ccd_edge(torch_cuda):
    """the grid hangs over the corner (1, 1) of the CCD by 28 and 14 pixels, the object's centre is 2.6 pixels inside the chip: the CCD
    holds the part of the image that is on it"""
    flux, nfft, cx, cy = 2.0e6, 64, 30.6, 31.3
    rows = cf.make_rows([dict(nfft=nfft, x0=-27, y0=-13, cx=cx, cy=cy, flux=flux, obj_id=31, jac=JACS[0])])
    knots = _side(rows, [7], 0.3)
    d = _positions(torch_cuda, rows, knots)
    assert kc.margin_in_sigmas(nfft, cx, cy, d, SIGMA_PSF, PS) >= 8.0
    r, _, _, images = _draw(torch_cuda, rows, knots, configs.scene_c2(nx=96, ny=80))
    got = r.image64_numpy()
    v = np.where(images[0] < 0.0, 0.0, images[0])
    on_chip = np.zeros((80, 96))
    on_chip[:nfft - 14, :nfft - 28] = v[14:, 28:]                # grid index 28 along x is CCD pixel 1, column 0
    assert_bits_equal(got, on_chip, "CCD image of the clipped knots stamp")
    want = kc.image_ref(nfft, cx, cy, d, SIGMA_PSF, PS, flux)[14:, 28:]
    tol = (cf.omitted_alias_bound(SIGMA_PSF, nfft, 0, PS) + ROUNDING) * flux * want.size
    print(f"flux on the chip {got.sum():.6f}, closed form {want.sum():.6f}, allowed {tol:.3e}")
    assert abs(got.sum() - want.sum()) <= tol
    assert 0.3 * flux < got.sum() < 0.999 * flux                 # a visible part of the object is off the chip


# two knots objects and a star near the boresight of a 256^2 CCD: 2.0e6 e- in 12 knots (hlr 0.3"), 1.5e4 e- in 12 knots, a star of 1.5e5
KNOTS = ("object 9001 60.4890 -38.1650 16.5909 flatSED/sed_flat.txt.gz 0 0 0 0 0 0 knots 0.3 0.3 0.0 12 none none\n"
         "object 9002 60.4925 -38.1630 21.9032 flatSED/sed_flat.txt.gz 0 0 0 0 0 0 knots 0.3 0.3 0.0 12 none none\n"
         "object 9003 60.4860 -38.1620 19.4032 flatSED/sed_flat.txt.gz 0 0 0 0 0 0 point none none\n")


def test_lsst_image_config_draws_the_bright_knots_object_by_fft(torch_cuda, tmp_path):
    """The path a user takes: instance-catalog `knots` lines -> config.Process with image.type LSST_Image on a 256^2 CCD, the Silicon
    sensor, stamp.fft_sb_thresh, input.vignetting and stamp.fft_knots.  PSF: a Gaussian of FWHM 0.7" (peak 1 / 0.555 arcsec^-2):
    2e6 / 0.555 / 2 x 0.04 = 7.2e4 per pixel > 1e4 for the bright object; the faint one is below 1e6 e-.  Without the key the render is
    the one of before: bit for bit the image of draw_method phot, in which nothing is FFT-drawn."""
    from imsim_amd import config, truth as truthmod
    from imsim_amd.vignetting import Vignetting
    here = os.path.dirname(os.path.abspath(__file__))
    fn = tmp_path / "knots.txt"
    with open(os.path.join(here, "golden", "example_instcat_subset.txt")) as f:
        header = "".join(line for line in f if not line.startswith("object"))          # the visit of the golden catalog
    fn.write_text(header + KNOTS)
    columns = {"object_id": "@object_id", "x": "$image_pos.x", "y": "$image_pos.y", "nominal_flux": "@nominal_flux",
               "phot_flux": "@phot_flux", "fft_flux": "@fft_flux", "realized_flux": "@realized_flux"}
    res = {}
    for name, extra in (("on", {"stamp.fft_knots": True}), ("off", {}), ("phot", {"stamp.draw_method": "phot"})):
        out = tmp_path / name
        over = {"input.instance_catalog.file_name": str(fn), "input.instance_catalog.sort_mag": False, "image.xsize": 256, "image.ysize": 256,
                "stamp.fft_sb_thresh": 1.0e4, "psf": {"type": "Gaussian", "fwhm": 0.7}, "input.vignetting": {"file_name": "LSSTCam_vignetting_data.json"},
                "output.dir": str(out), "output.truth": {"dir": str(out), "file_name": "centroid.txt", "columns": columns}}
        over.update(extra)
        res[name] = config.Process(os.path.join(here, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(here, "data")],
                                   overrides=over)
    a = res["on"]
    assert a.det_names == ["R22_S11"] and a.images[0].shape == (256, 256)
    t = a.truth[0]
    assert [str(s) for s in t["object_id"]] == ["9001", "9002", "9003"]
    assert list(t["mode"]) == ["fft", "phot", "phot"]
    np.testing.assert_allclose(t["nominal_flux"][0], 2.0e6, rtol=1e-3)
    factor = float(Vignetting("LSSTCam_vignetting_data.json").at_pixel("R22_S11", t["x"][:1], t["y"][:1], 256, 256)[0])
    assert 0.9 < factor <= 1.0
    assert t["fft_flux"][0] == t["nominal_flux"][0] * factor and t["fft_flux"][1] == 0.0 and t["fft_flux"][2] == 0.0
    assert t["phot_flux"][0] == 0.0 and t["phot_flux"][1] > 0.0 and t["phot_flux"][2] > 0.0
    F = float(t["fft_flux"][0])
    print(f"fft_flux {F:.1f}, realized {t['realized_flux'][0]:.1f}, 5 sigma {5.0 * math.sqrt(F):.1f}")
    assert abs(t["realized_flux"][0] - F) <= 5.0 * math.sqrt(F)
    # the flux of the image inside the bright object's stamp (the other two objects are more than 40 pixels away)
    x, y = int(round(float(t["x"][0]))) - 1, int(round(float(t["y"][0]))) - 1
    box = a.images[0][max(y - 16, 0):y + 17, max(x - 16, 0):x + 17].astype(np.float64).sum()
    print(f"flux in the bright object's stamp {box:.1f}")
    assert abs(box - F) <= 5.0 * math.sqrt(F)
    rows = truthmod.read(str(tmp_path / "on" / "centroid.txt"))
    np.testing.assert_allclose(rows["fft_flux"], t["fft_flux"], rtol=2e-8)
    # without the key: knots stay with the photons, and the image is draw_method phot's bit for bit
    off, phot = res["off"], res["phot"]
    assert list(off.truth[0]["mode"]) == ["phot", "phot", "phot"] and not np.asarray(off.truth[0]["fft_flux"]).any()
    assert_bits_equal(off.images[0], phot.images[0], "image without stamp.fft_knots")
    assert not np.array_equal(a.images[0], off.images[0])
