"""FFT-drawn FITS stamps on the GPU (stamp.fft_stamps): ims_fft_image_factor against the extended-precision sum of
tests/stamp_closed_forms.py, the drawn images against the pixel integrals of (quintic kernel) x (Gaussian), linearity in the stamp's
pixels, the FFT branch against photon shooting, the bits of every other object of a batch, and the path through a config.  Pixel
scale 0.2", no spikes, n_alias 0.  Grids of 32, 64 (two row tiles) and 128 (65 columns: a second column tile of one column).

Every test prints its figures before it asserts (pytest -s).  Measured on an MI355X:
    factor against the longdouble sum: 1.6e-14 on 32 (bound 1.8e-13), 1.8e-14 on 64 (3.6e-13), 2.3e-14 on 128 (7.2e-13); nearest 4.6e-16
    image against the pixel integrals, per unit flux: 1.2e-16 at sigma 0.5" (allowed 1.0e-13), 2.1e-6 at 0.25" (allowed 1.0e-5)
    linearity 2.9e-16 of the peak; chi-square per degree of freedom against photons 1.127 over 384 pixels (allowed 1 +- 0.361)"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from helpers import assert_bits_equal
from imsim_amd import _abi, catalog, configs, fft_draw
import fft_closed_forms as cf
import photon_source_cases as cases
import stamp_closed_forms as sc
from test_fft_stamps import PHOTON_CASE, SIGMAS_PSF, centre_pixel_stamp, image_tolerance, photon_case_stamp

pytestmark = pytest.mark.gpu

PS = sc.PIXEL_SCALE
SEED = cases.SEED
GRIDS = (32, 64, 128)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _factor_rows():
    """every stamp with both affines on every grid; a point row in the middle of every grid's rows, between two stamp rows with
    different stamps, that the pass must not touch"""
    stamps = sc.factor_stamps()
    specs, row_image = [], []
    for nfft in GRIDS:
        k = 0
        for j, jac in enumerate(sc.JACS):
            for s, (name, img, p) in enumerate(stamps):
                specs.append(dict(nfft=nfft, x0=0, y0=0, cx=nfft / 2.0, cy=nfft / 2.0, flux=1.0, obj_id=1000 * nfft + 10 * s + j, jac=jac,
                                  prof_scale=p))
                row_image.append(s)
                k += 1
                if k == 3:
                    specs.append(dict(nfft=nfft, x0=0, y0=0, cx=3.0, cy=4.0, flux=1.0, obj_id=nfft))
                    row_image.append(-1)
    return cf.make_rows(specs), np.asarray(row_image, dtype=np.int32), stamps


def _run_factor(torch, rows, row_image, images, interpolant=1, n_alias=0, fill=None):
    """ims_fft_image_factor over a buffer of ones (or `fill`): (1 + 0 i) F is F, bit for bit -> (return code, buffer on the host)"""
    lib = _abi.load()
    dev = "cuda"
    size, offset, ab, w = fft_draw.image_pixel_lists(images)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to(dev)
    obj_t = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()).to(dev)
    which = np.flatnonzero(row_image >= 0).astype(np.int32)
    keep = [up(which), up(row_image), up(size), up(offset), up(ab), up(w)]
    total = int(sum(int(o["nfft"]) * (int(o["nfft"]) // 2 + 1) for o in rows))
    kbuf = torch.ones(total, dtype=torch.complex128, device=dev) if fill is None else torch.from_numpy(fill.copy()).to(dev)
    P = _abi.FftParams()
    P.pixel_scale, P.n_alias = PS, n_alias
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.ims_fft_image_factor(C.byref(P), obj_t.data_ptr(), keep[0].data_ptr(), len(which), int(rows["nfft"][which].max()),
                                  keep[1].data_ptr(), len(size), keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(),
                                  keep[5].data_ptr(), interpolant, kbuf.data_ptr(), st)
    torch.cuda.synchronize()
    return rc, kbuf.cpu().numpy()


def _split(rows, k):
    return [k[int(o["k_offset"]):int(o["k_offset"]) + int(o["nfft"]) * (int(o["nfft"]) // 2 + 1)].reshape(int(o["nfft"]), -1) for o in rows]


@pytest.fixture(scope="module")
def factors(torch_cuda):
    rows, row_image, stamps = _factor_rows()
    images = [img for _, img, _ in stamps]
    rc, k = _run_factor(torch_cuda, rows, row_image, images)
    assert rc == 0, _abi.load().ims_last_error()
    return rows, row_image, stamps, k


@pytest.mark.parametrize("nfft", GRIDS)
def test_factor_is_the_extended_precision_sum(factors, nfft):
    rows, row_image, stamps, k = factors
    worst, seen = 0.0, 0
    for o, s, got in zip(rows, row_image, _split(rows, k)):
        if int(o["nfft"]) != nfft:
            continue
        if s < 0:
            assert_bits_equal(got.view(np.float64), np.ones_like(got).view(np.float64), "a row without a stamp")
            continue
        name, img, p = stamps[s]
        jac = tuple(float(v) for v in o["jac"])
        assert sc.extent(img, p, jac) <= 0.5 * nfft * PS, "a pixel outside half the grid: the bound's premise"
        re, im = sc.F_ref(img, p, jac, nfft, PS)
        err = float(max(np.abs(got.real.astype(np.longdouble) - re).max(), np.abs(got.imag.astype(np.longdouble) - im).max()))
        print(f"grid {nfft} stamp {name} det {jac[0] * jac[3] - jac[1] * jac[2]:.3f}: F misses the longdouble sum by {err:.3e}, "
              f"allowed {sc.factor_bound(nfft):.3e}")
        assert err <= sc.factor_bound(nfft)
        assert got[0, 0].imag == 0.0 and abs(got[0, 0].real - 1.0) <= 4.0 * sc.EPS                   # F(0) = sum w = 1
        worst, seen = max(worst, err), seen + 1
    print(f"grid {nfft}: largest deviation {worst:.3e} over {seen} rows, bound {sc.factor_bound(nfft):.3e}, ratio {worst / sc.factor_bound(nfft):.3f}")
    assert seen == 8 and worst > 0.0


def test_nearest_interpolant_takes_the_sinc(torch_cuda):
    name, img, p = sc.factor_stamps()[1]
    rows = cf.make_rows([dict(nfft=64, x0=0, y0=0, cx=32.0, cy=32.0, flux=1.0, obj_id=5, jac=sc.JACS[1], prof_scale=p)])
    rc, k = _run_factor(torch_cuda, rows, np.array([0], dtype=np.int32), [img], interpolant=0)
    assert rc == 0
    re, im = sc.F_ref(img, p, sc.JACS[1], 64, PS, "nearest")
    got = _split(rows, k)[0]
    err = float(max(np.abs(got.real.astype(np.longdouble) - re).max(), np.abs(got.imag.astype(np.longdouble) - im).max()))
    print(f"nearest interpolant, grid 64: {err:.3e}, allowed {sc.factor_bound(64):.3e}")
    assert err <= sc.factor_bound(64)
    qre, _ = sc.F_ref(img, p, sc.JACS[1], 64, PS, "quintic")
    assert float(np.abs(qre - re).max()) > 1.0e-3                                                     # and it is not the quintic's


def test_two_calls_give_the_same_bits_and_aliases_are_refused(torch_cuda, factors):
    rows, row_image, stamps, k = factors
    images = [img for _, img, _ in stamps]
    rc, again = _run_factor(torch_cuda, rows, row_image, images)
    assert rc == 0
    assert_bits_equal(again.view(np.float64), k.view(np.float64), "second call")
    fill = (np.random.default_rng(3).standard_normal(len(k)) + 1j * np.random.default_rng(4).standard_normal(len(k))).astype(np.complex128)
    rc, out = _run_factor(torch_cuda, rows, row_image, images, n_alias=1, fill=fill)
    assert rc == -4                                                                                   # IMS_ERR_UNSUPPORTED
    assert b"n_alias" in _abi.load().ims_last_error()
    assert_bits_equal(out.view(np.float64), fill.view(np.float64), "kbuf after the refused call")


def _draw(torch, rows, images=None, profiles=None, sigma=0.5, interpolant="quintic", force_base_band=False, scene=None):
    """one noiseless draw -> (renderer, drawer, [half spectrum per row], [image per row])"""
    from imsim_amd.engine import Renderer
    s = scene or configs.scene_c2(nx=256, ny=256)
    s.seed = SEED
    s.image_profiles = profiles
    s.image_interpolant = interpolant
    r = Renderer(s)
    drawer = fft_draw.FftDrawer(r, [(_abi.IMS_KPSF_GAUSSIAN, 0, sigma)], add_noise=False)
    if force_base_band:
        drawer.P.n_alias = 0                 # the fill leaves the aliases out; the tolerance carries their bound (omitted_alias_bound)
    assert drawer.P.n_alias == 0 and not drawer.P.spikes.enabled
    drawer.keep_kspace = True
    kbuf, rbuf = drawer.draw(rows, images=images)
    r.synchronize()
    return r, drawer, _split(rows, kbuf.cpu().numpy()), cf.grids(rows, fft_draw.image_from_rbuf(rows, rbuf.cpu().numpy()))


@pytest.mark.parametrize("sigma", SIGMAS_PSF)
def test_image_is_the_pixel_integral_of_kernel_and_gaussian(torch_cuda, sigma):
    """a 5 x 5 stamp whose only positive pixel is the centre one, p = 0.2", J' the identity, grid 64: pixel (i, j) is F I(i) I(j).
    With the Gaussian of 0.25" the PSF's alias order is 1: the draw is made in the base band (n_alias forced to 0, what the pass
    supports) and the aliases left out are inside the tolerance, as the Gaussian-PSF point case has them; 0.5" needs none."""
    flux, nfft, cx, cy, p = 3.0e6, 64, 31.4, 32.7, 0.2
    img = centre_pixel_stamp()
    rows = cf.make_rows([dict(nfft=nfft, x0=40, y0=50, cx=cx, cy=cy, flux=flux, obj_id=77, prof_scale=p)])
    _, drawer, _, images = _draw(torch_cuda, rows, np.array([0], dtype=np.int32), [img], sigma=sigma, force_base_band=True)
    assert drawer.image_launches == 1
    want = sc.image_ref(nfft, cx, cy, img, p, sigma, PS, flux).astype(np.float64)
    tol = image_tolerance(sigma, nfft, cx, cy, img, p) * flux
    err = float(np.abs(images[0] - want).max())
    print(f"sigma {sigma}: image misses the pixel integrals by {err / flux:.3e} per unit flux, allowed {tol / flux:.3e}")
    assert err <= tol
    assert abs(images[0].sum() - flux) <= 1.0e-10 * flux


def test_image_is_linear_in_the_stamps_pixels(torch_cuda):
    """a 4 x 6 stamp of random weights under a rotated J' is the weighted sum of its 24 single-pixel renders (each the same 4 x 6
    stamp with one positive pixel), to 1e-12 of the peak; the image total is F to 1e-10; a point row between the stamp rows comes
    back with the bits it has alone."""
    flux, nfft, p = 2.0e6, 64, 0.3
    t = math.radians(25.0)
    jac = (1.1 * math.cos(t), -1.1 * math.sin(t), 1.1 * math.sin(t), 1.1 * math.cos(t))
    full = np.random.default_rng(12).uniform(0.1, 2.0, size=(4, 6))
    singles = []
    for b in range(4):
        for a in range(6):
            one = np.zeros((4, 6))
            one[b, a] = 1.0
            singles.append(one)
    spec = dict(nfft=nfft, x0=30, y0=40, cx=31.7, cy=32.2, flux=flux, jac=jac, prof_scale=p)
    point = dict(nfft=nfft, x0=120, y0=130, cx=30.5, cy=33.1, flux=1.5e6, obj_id=500)
    specs = [dict(spec, obj_id=100)] + [point] + [dict(spec, obj_id=200 + m) for m in range(24)]
    rows = cf.make_rows(specs)
    row_image = np.array([0, -1] + list(range(1, 25)), dtype=np.int32)
    _, drawer, spectra, images = _draw(torch_cuda, rows, row_image, [full] + singles, sigma=0.5)
    assert drawer.image_launches == 1
    w = full.reshape(-1) / full.sum()
    want = sum(w[m] * images[2 + m] for m in range(24))
    peak = float(images[0].max())
    err = float(np.abs(images[0] - want).max())
    print(f"linearity: {err:.3e} at a peak of {peak:.3e} ({err / peak:.3e} of it); total {images[0].sum():.6f} for {flux}")
    assert err <= 1.0e-12 * peak
    assert abs(images[0].sum() - flux) <= 1.0e-10 * flux
    # the point row: the bits of the same row drawn alone, without side arrays
    alone = cf.make_rows([point])
    _, plain, s1, i1 = _draw(torch_cuda, alone, sigma=0.5)
    assert plain.image_launches == 0 and plain._last[9] is None
    assert_bits_equal(spectra[1].view(np.float64), s1[0].view(np.float64), "half spectrum of the point row")
    assert_bits_equal(images[1], i1[0], "image of the point row")
    # a batch whose side array names no stamp launches nothing
    _, none, _, _ = _draw(torch_cuda, alone, np.array([-1], dtype=np.int32), [full], sigma=0.5)
    assert none.image_launches == 0


def test_fft_against_photons(torch_cuda):
    """The same 8 x 8 random stamp (sheared J', Gaussian PSF of 0.3", 2e6 e-) FFT-drawn without noise and photon-shot without sensor
    on the same CCD.  Nearest interpolant: its photons carry unit flux, so a pixel's count is Poisson about the expectation and
    Pearson's chi-square applies (the quintic's photons carry +-1.58: its placement is held to the same pixel centres by the factor
    and image tests above).  tests/test_fft_stamps.py settles on the host that the pixels of at least 25 e- cover the footprint."""
    from imsim_amd.engine import Renderer
    c = PHOTON_CASE
    img = photon_case_stamp()
    n_phot = int(c["flux"])
    cat = dict(x=np.array([100.6]), y=np.array([90.3]), mag=np.zeros(1), nominal_flux=np.array([c["flux"]]),
               kind=np.array([catalog.KIND_IMAGE], dtype=np.int32), hlr=np.zeros(1), q=np.ones(1), pa=np.zeros(1),
               obj_id=np.array([41], dtype=np.int64), n_knots=np.zeros(1), box_length=np.zeros(1), box_width=np.zeros(1),
               image_index=np.zeros(1, dtype=np.int64), image_scale=np.array([c["p"]]), image_extent=np.array([8 * c["p"]]))
    objects, _ = catalog.build_object_table(cat, np.array([n_phot]), stamp_size=np.array([64]))
    objects["jac"][0] = c["jac"]

    def scene():
        s = configs.scene_c2(nx=192, ny=192)
        s.seed = SEED
        s.psf = [(_abi.IMS_PSF_GAUSSIAN, 0, c["sigma"], 0.0, 1.0)]
        s.image_profiles, s.image_interpolant = [img], "nearest"
        return s
    # photons: the simple-accumulate path
    r = Renderer(scene())
    r.render(objects)
    r.synchronize()
    shot = r.image64_numpy()
    # FFT: the same row through build_fft_objects, onto a CCD of its own
    rows, order = fft_draw.build_fft_objects(objects, np.array([c["flux"]]), fft_draw.profile_ktable_ids(None, objects["prof_table"]))
    assert list(rows["prof_ktable"]) == [-1] and rows["nfft"][0] == 64
    r2, drawer, _, _ = _draw(torch_cuda, rows, fft_draw.image_side_arrays(objects, order), [img], sigma=c["sigma"],
                             interpolant="nearest", scene=scene())
    assert drawer.image_launches == 1
    want = r2.image64_numpy()
    sel = want >= c["floor"]
    dof = int(sel.sum())
    foot = sc.footprint_pixels(img, c["p"], c["jac"], PS)
    chi2 = float((((shot - want) ** 2)[sel] / want[sel]).sum()) / dof
    print(f"{dof} pixels of at least {c['floor']} e- (footprint {foot:.1f}): chi-square per degree of freedom {chi2:.4f}, "
          f"allowed 1 +- {5.0 * math.sqrt(2.0 / dof):.4f}; totals {shot.sum():.1f} photon-shot, {want.sum():.1f} FFT")
    assert dof >= 0.25 * foot
    assert abs(chi2 - 1.0) <= 5.0 * math.sqrt(2.0 / dof)
    assert abs(shot.sum() - want.sum()) <= 5.0 * math.sqrt(c["flux"])


# a star, a bright FITS-stamp object (5.0e6 e-) and a faint one (1.5e4 e-) near the boresight of a 256^2 CCD
STAMPS = ("object 9001 60.4890 -38.1650 15.5960 flatSED/sed_flat.txt.gz 0 0 0 0 0 0 stamp.fits 0.2 30.0 none none\n"
          "object 9002 60.4925 -38.1630 21.9032 flatSED/sed_flat.txt.gz 0 0 0 0 0 0 stamp.fits 0.2 0.0 none none\n"
          "object 9003 60.4860 -38.1620 19.4032 flatSED/sed_flat.txt.gz 0 0 0 0 0 0 point none none\n")


def _process(tmp_path, itype, runs):
    """config.Process on a 256^2 CCD for every (name, overrides) of `runs` -> ({name: result}, flux key of the truth record)"""
    from imsim_amd import config, fits_io
    here = os.path.dirname(os.path.abspath(__file__))
    fits_io.write_fits(str(tmp_path / "stamp.fits"), [({}, photon_case_stamp().astype(np.float32))])
    fn = tmp_path / "stamps.txt"
    with open(os.path.join(here, "golden", "example_instcat_subset.txt")) as f:
        header = "".join(line for line in f if not line.startswith("object"))          # the visit of the golden catalog
    fn.write_text(header + STAMPS)
    pooling = itype == "LSST_PhotonPoolingImage"
    flux_key = "incident_flux" if pooling else "realized_flux"
    columns = {"object_id": "@object_id", "x": "$image_pos.x", "y": "$image_pos.y", "nominal_flux": "@nominal_flux",
               "phot_flux": "@phot_flux", "fft_flux": "@fft_flux", flux_key: "@" + flux_key}
    res = {}
    for name, extra in runs:
        out = tmp_path / name
        over = {"input.instance_catalog.file_name": str(fn), "input.instance_catalog.sort_mag": False, "image.xsize": 256, "image.ysize": 256,
                "stamp.fft_sb_thresh": 1.0e4, "psf": {"type": "Gaussian", "fwhm": 0.7},
                "input.vignetting": {"file_name": "LSSTCam_vignetting_data.json"}, "output.dir": str(out)}
        if pooling:
            over.update({"image.type": itype, "stamp.type": "LSST_Photons", "input.checkpoint": "", "output.truth": "",
                         "output.photon_pooling_truth": {"dir": str(out), "file_name": "centroid.txt", "columns": columns}})
        else:
            over["output.truth"] = {"dir": str(out), "file_name": "centroid.txt", "columns": columns}
        over.update(extra)
        res[name] = config.Process(os.path.join(here, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(here, "data")],
                                   overrides=over)
    return res, flux_key


def _check_bright_is_fft(res, flux_key, itype):
    from imsim_amd.vignetting import Vignetting
    t = res.truth[0]
    assert [str(s) for s in t["object_id"]] == ["9001", "9002", "9003"]
    assert list(t["mode"]) == ["fft", "phot", "phot"]
    np.testing.assert_allclose(t["nominal_flux"][0], 5.0e6, rtol=1e-3)
    factor = float(Vignetting("LSSTCam_vignetting_data.json").at_pixel("R22_S11", t["x"][:1], t["y"][:1], 256, 256)[0])
    assert 0.9 < factor <= 1.0
    assert t["fft_flux"][0] == t["nominal_flux"][0] * factor and t["fft_flux"][1] == 0.0 and t["fft_flux"][2] == 0.0
    assert t["phot_flux"][0] == 0.0 and t["phot_flux"][1] > 0.0 and t["phot_flux"][2] > 0.0
    F = float(t["fft_flux"][0])
    print(f"{itype}: fft_flux {F:.1f}, {flux_key} {t[flux_key][0]:.1f}, 5 sigma {5.0 * math.sqrt(F):.1f}")
    assert abs(t[flux_key][0] - F) <= 5.0 * math.sqrt(F)


@pytest.mark.parametrize("itype", ["LSST_Image", "LSST_PhotonPoolingImage"])
def test_config_draws_the_bright_stamp_by_fft(torch_cuda, tmp_path, itype):
    """The path a user takes: instance-catalog FITS-stamp lines -> config.Process on a 256^2 CCD with stamp.fft_sb_thresh,
    input.vignetting and stamp.fft_stamps.  PSF: a Gaussian of FWHM 0.7" (1 / peak 0.555 arcsec^2); the 8 x 8 stamp of 0.2" has
    max w of some 0.03, 1 / peak some 1.4 arcsec^2: 5e6 / 1.9 / 2 x 0.04 = 5e4 per pixel > 1e4; the faint one is below 1e6 e-."""
    runs = [("on", {"stamp.fft_stamps": True})]
    if itype == "LSST_Image":
        runs.append(("sharp", {"stamp.fft_stamps": True, "psf": {"type": "Gaussian", "fwhm": 0.28}}))
    res, flux_key = _process(tmp_path, itype, runs)
    _check_bright_is_fft(res["on"], flux_key, itype)
    if itype == "LSST_Image":
        # a PSF whose aliases the fill folds (sigma 0.119": alias order 1): the bright stamp stays with the photons, key or not
        assert list(res["sharp"].truth[0]["mode"])[:2] == ["phot", "phot"]


@pytest.mark.parametrize("itype", ["LSST_Image", "LSST_PhotonPoolingImage"])
def test_config_without_the_key_is_the_render_of_false(torch_cuda, tmp_path, monkeypatch, itype):
    """Without the key both stamps say `phot`, and the image is the one of `stamp.fft_stamps: false`, bit for bit.
    These runs take the nearest interpolant: the photons of a quintic stamp carry +-1.584 e-, the f64 image is accumulated with
    atomic additions, and the last bit of a pixel then depends on the order in which its photons arrive (two runs of one and the
    same config differed in one pixel, 0 against -4.4e-16, on an MI355X); with unit photons every partial sum is an integer and
    the image does not depend on the order."""
    from imsim_amd import engine
    scene_init = engine.Scene.__init__

    def nearest_scene(self, *args, **kw):
        scene_init(self, *args, **kw)
        self.image_interpolant = "nearest"
    monkeypatch.setattr(engine.Scene, "__init__", nearest_scene)
    res, flux_key = _process(tmp_path, itype, [("absent", {}), ("false", {"stamp.fft_stamps": False})])
    absent, false = res["absent"], res["false"]
    for r in (absent, false):
        assert list(r.truth[0]["mode"]) == ["phot", "phot", "phot"] and not np.asarray(r.truth[0]["fft_flux"]).any()
    assert_bits_equal(absent.images[0], false.images[0], "image without stamp.fft_stamps")
    assert float(absent.images[0].sum()) > 4.0e6                                                     # the bright stamp is there, photon-shot
