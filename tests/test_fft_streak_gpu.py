"""FFT-drawn streaks on the GPU: the box branch of the k-space fill (kspace_pair for the mirrored rows 0 < i < n / 2, kspace_at
through kspace_value for rows 0 and n / 2), the library's inverse transform and the finish, against tests/streak_closed_forms.py.
Gaussian PSF of sigma 0.4", pixel scale 0.2", no noise, no spikes, n_alias 0.

Tolerances.  Against restatement (a): what the EXISTING delta and Sersic branches (bit-exact to the oracle) show against the same
numpy restatement at the same grids, centres and fluxes -- numpy's sine, cosine and exponential against the library's -- times four.
Measured on an MI355X, per unit flux, worst element (the constants below):
    half spectra:  delta 1.688e-15, Sersic 1.491e-15   -> the box may miss by 6.75e-15; it misses by 1.42e-15
    images:        delta 3.638e-17, Sersic 2.728e-17   -> the box may miss by 1.46e-16; it misses by 2.5e-17
Against (b) and (c): the host residuals recorded in tests/streak_closed_forms.py, times four.
Every test prints its figures before it asserts (pytest -s)."""
import math

import numpy as np
import pytest

from helpers import assert_bits_equal
from imsim_amd import _abi, configs, fft_draw, tables
import fft_closed_forms as cf
import streak_closed_forms as sf

pytestmark = pytest.mark.gpu

# measured deviation of the existing branches from restatement (a), per unit flux (test_existing_branches_against_the_restatement
# prints them); the box is allowed 4 x the larger of each pair
MEASURED_SPEC_DELTA, MEASURED_SPEC_SERSIC = 1.688e-15, 1.491e-15
MEASURED_IMG_DELTA, MEASURED_IMG_SERSIC = 3.638e-17, 2.728e-17
TOL_SPEC = 4.0 * max(MEASURED_SPEC_DELTA, MEASURED_SPEC_SERSIC)
TOL_IMG = 4.0 * max(MEASURED_IMG_DELTA, MEASURED_IMG_SERSIC)

KPSF = [(_abi.IMS_KPSF_GAUSSIAN, 0, sf.SIGMA)]
SERSIC_SCALE = 0.3            # arcsec: half-light radius of the n = 1 comparison profile


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _draw(torch, rows, scene=None):
    """one noiseless draw -> (renderer, drawer, [half spectrum per row], [image per row])"""
    from imsim_amd.engine import Renderer
    r = Renderer(scene or configs.scene_c2(nx=256, ny=256))
    drawer = fft_draw.FftDrawer(r, KPSF, add_noise=False)
    assert drawer.P.n_alias == 0 and not drawer.P.spikes.enabled
    drawer.keep_kspace = True
    kbuf, rbuf = drawer.draw(rows)
    r.synchronize()
    k = kbuf.cpu().numpy()
    spectra = [k[int(o["k_offset"]):int(o["k_offset"]) + int(o["nfft"]) * (int(o["nfft"]) // 2 + 1)].reshape(int(o["nfft"]), -1)
               for o in rows]
    return r, drawer, spectra, cf.grids(rows, fft_draw.image_from_rbuf(rows, rbuf.cpu().numpy()))


def _ktables():
    q, t1 = tables.sersic_ktable(1.0)
    return [t1, tables.sersic_ktable(4.0)[1]], float(q[1] - q[0])


def _deviations(rows, spectra, images):
    """worst (spectrum, image) deviation from (a) per unit flux over the rows; the Nyquist column and row carry imaginary parts the
    real transform ignores: they count like every other element"""
    kt, q_step = _ktables()
    ds = di = 0.0
    for o, spec, img in zip(rows, spectra, images):
        want = sf.half_spectrum(o, ktables=kt, q_step=q_step)
        ds = max(ds, float(np.abs(spec - want).max()) / float(o["flux"]))
        di = max(di, float(np.abs(img - sf.image_a(o, ktables=kt, q_step=q_step)).max()) / float(o["flux"]))
    return ds, di


@pytest.fixture(scope="module")
def boxes(torch_cuda):
    """the eight boxes of streak_closed_forms.CASES in one batch (grids of 32 and 64), drawn once"""
    rows = sf.box_rows()
    r, drawer, spectra, images = _draw(torch_cuda, rows)
    return rows, spectra, images


def _like(prof_ktable):
    """the cases' grids, centres and fluxes with another profile: a point, or the n = 1 Sersic sheared by the box's affine"""
    rows = sf.box_rows()
    rows["prof_ktable"] = prof_ktable
    if prof_ktable == -1:
        rows["jac"] = (1.0, 0.0, 0.0, 1.0)
    else:
        rows["jac"] = [sf.box_jac(1.0, 0.5, c[3]) for c in sf.CASES]
        rows["prof_scale"] = SERSIC_SCALE
    return rows


def test_existing_branches_against_the_restatement(torch_cuda):
    """the yardstick of TOL_SPEC / TOL_IMG, measured again: it must not have moved past what the module states"""
    got = {}
    for name, t in (("delta", -1), ("sersic", 0)):
        rows = _like(t)
        _, _, spectra, images = _draw(torch_cuda, rows)
        got[name] = _deviations(rows, spectra, images)
        print(f"{name}: half spectra {got[name][0]:.3e}, images {got[name][1]:.3e} per unit flux")
    assert got["delta"][0] <= 2.0 * MEASURED_SPEC_DELTA and got["sersic"][0] <= 2.0 * MEASURED_SPEC_SERSIC
    assert got["delta"][1] <= 2.0 * MEASURED_IMG_DELTA and got["sersic"][1] <= 2.0 * MEASURED_IMG_SERSIC


def test_half_spectra_and_images_are_the_restatement(boxes):
    rows, spectra, images = boxes
    assert list(rows["prof_ktable"]) == [-2] * 8 and list(rows["nfft"]) == [32] * 4 + [64] * 4
    ds, di = _deviations(rows, spectra, images)
    print(f"box: half spectra {ds:.3e} (allowed {TOL_SPEC:.3e}), images {di:.3e} (allowed {TOL_IMG:.3e}) per unit flux")
    # rows 0 and n / 2 come from kspace_at, the others from kspace_pair: both are in the comparison
    assert ds <= TOL_SPEC
    assert di <= TOL_IMG


def test_axis_aligned_boxes_are_the_separable_closed_form(boxes):
    rows, _, images = boxes
    seen = 0
    for case, img in zip(sf.CASES, images):
        if case[3] not in (0.0, 90.0):
            continue
        err = float(np.abs(img - sf.image_b_of(case)).max()) / case[6]
        print(f"grid {case[0]} L {case[1]} W {case[2]} pa {case[3]}: (b) misses by {err:.3e} per unit flux, allowed {4.0 * sf.RESIDUAL_B:.3e}")
        assert err <= 4.0 * sf.RESIDUAL_B
        seen += 1
    assert seen == 5


def test_moments_are_exact_at_every_angle(boxes):
    rows, _, images = boxes
    for case, img in zip(sf.CASES, images):
        n = case[0]
        total, mx, my, cov = sf.moments(img, case[4], case[5])
        es = abs(math.fsum(img.ravel()) / case[6] - 1.0)
        ec = max(abs(mx - case[4]), abs(my - case[5]))
        ev = float(np.abs(cov - sf.exact_moments(case[1], case[2], case[3])).max())
        print(f"grid {n} L {case[1]} W {case[2]} pa {case[3]}: sum {es:.3e} ({4 * sf.RESIDUAL_SUM:.1e}), centroid {ec:.3e} "
              f"({4 * sf.RESIDUAL_CENTROID[n]:.1e}), covariance {ev:.3e} ({4 * sf.RESIDUAL_COV[n]:.1e})")
        assert es <= 4.0 * sf.RESIDUAL_SUM
        assert ec <= 4.0 * sf.RESIDUAL_CENTROID[n]
        assert ev <= 4.0 * sf.RESIDUAL_COV[n]


# the delta and Sersic branches against (a) on the grids of LARGE_CASES, per unit flux (larger grids, larger phases): half spectra
# delta 9.136e-15 / Sersic 6.783e-15 on 256, 1.718e-14 / 1.290e-14 on 512; images 1.358e-16 / 8.731e-17 on 256, 2.561e-16 / 1.607e-16
# on 512 -- the oracle's figures, whose half spectra are the kernels' bit for bit (tests/test_parity_gpu.py); the test prints the
# kernels' own and holds them to these
MEASURED_LARGE = {256: (9.136e-15, 1.358e-16), 512: (1.718e-14, 2.561e-16)}


def test_boxes_on_grids_wider_than_one_level_of_the_column_tables(torch_cuda):
    """grids of 256 and 512 (129 and 257 columns: the second level of the fill's column tables, jh = 0 .. 4; workgroups of 256
    elements, each inside one row or two): half spectra and images against (a), the quarter-turned box against (b), moments against (c)"""
    got = {}
    for name, t in (("delta", -1), ("sersic", 0)):
        rows = sf.box_rows(sf.LARGE_CASES)
        rows["prof_ktable"] = t
        if t == -1:
            rows["jac"] = (1.0, 0.0, 0.0, 1.0)
        else:
            rows["jac"] = [sf.box_jac(1.0, 0.5, c[3]) for c in sf.LARGE_CASES]
            rows["prof_scale"] = SERSIC_SCALE
        _, _, spectra, images = _draw(torch_cuda, rows)
        for k, o in enumerate(rows):
            d = _deviations(rows[k:k + 1], spectra[k:k + 1], images[k:k + 1])
            n = int(o["nfft"])
            got[n] = tuple(max(a, b) for a, b in zip(got.get(n, (0.0, 0.0)), d))
            print(f"{name}, grid {n}: half spectra {d[0]:.3e}, images {d[1]:.3e} per unit flux")
    for n in (256, 512):
        assert got[n][0] <= 2.0 * MEASURED_LARGE[n][0] and got[n][1] <= 2.0 * MEASURED_LARGE[n][1]
    rows = sf.box_rows(sf.LARGE_CASES)
    _, _, spectra, images = _draw(torch_cuda, rows)
    for k, (case, o) in enumerate(zip(sf.LARGE_CASES, rows)):
        n = case[0]
        ds, di = _deviations(rows[k:k + 1], spectra[k:k + 1], images[k:k + 1])
        print(f"box, grid {n} L {case[1]} pa {case[3]}: half spectra {ds:.3e} (allowed {4 * MEASURED_LARGE[n][0]:.3e}), "
              f"images {di:.3e} (allowed {4 * MEASURED_LARGE[n][1]:.3e}) per unit flux")
        assert ds <= 4.0 * MEASURED_LARGE[n][0] and di <= 4.0 * MEASURED_LARGE[n][1]
        img = images[k]
        if case[3] == 90.0:
            err = float(np.abs(img - sf.image_b_of(case)).max()) / case[6]
            print(f"   (b) misses by {err:.3e}, allowed {4 * sf.RESIDUAL_B_LARGE:.3e}")
            assert err <= 4.0 * sf.RESIDUAL_B_LARGE
        total, mx, my, cov = sf.moments(img, case[4], case[5])
        es = abs(math.fsum(img.ravel()) / case[6] - 1.0)
        ec = max(abs(mx - case[4]), abs(my - case[5]))
        ev = float(np.abs(cov - sf.exact_moments(case[1], case[2], case[3])).max())
        print(f"   sum {es:.3e} ({4 * sf.RESIDUAL_SUM:.1e}), centroid {ec:.3e} ({4 * sf.RESIDUAL_CENTROID[n]:.1e}), "
              f"covariance {ev:.3e} ({4 * sf.RESIDUAL_COV[n]:.1e})")
        assert es <= 4.0 * sf.RESIDUAL_SUM and ec <= 4.0 * sf.RESIDUAL_CENTROID[n] and ev <= 4.0 * sf.RESIDUAL_COV[n]


def test_a_saturating_streak_grows_spikes(torch_cuda):
    """4e7 e- in 3 x 0.6": 2.9e5 per pixel at the peak, over DiffractionFFT's 1e5 -- the spike step between clip and noise acts on a
    box as on a star: it changes the image, moves light out of the trail's core into the arms of the cross and keeps the flux"""
    from imsim_amd.diffraction_fft import DiffractionFFT
    from imsim_amd.engine import Renderer
    rows = cf.make_rows([dict(nfft=128, x0=60, y0=50, cx=63.4, cy=64.7, flux=4.0e7, prof_ktable=-2, jac=sf.box_jac(3.0, 0.6, 37.0))])
    cfg = DiffractionFFT(exptime=30.0, azimuth=math.radians(114.39), altitude=math.radians(53.16), rotTelPos=math.radians(40.04),
                         spike_length_cutoff=60)
    out = {}
    for name, d in (("plain", None), ("spikes", cfg)):
        r = Renderer(configs.scene_c2(nx=256, ny=256))
        drawer = fft_draw.FftDrawer(r, KPSF, add_noise=False, diffraction_fft=d, wavelength=622.2)
        assert bool(drawer.P.spikes.enabled) == (d is not None)
        real = torch_cuda.zeros(1, dtype=torch_cuda.float64, device="cuda")
        drawer.draw(rows, realized=real)
        r.synchronize()
        out[name] = (r.image64_numpy(), float(real.item()))
    plain, spiked = out["plain"][0], out["spikes"][0]
    assert plain.max() > cfg.brightness_threshold
    change = np.abs(spiked - plain)
    print(f"peak {plain.max():.3e}; the spike step moves {0.5 * change.sum():.3e} e-; realized {out['plain'][1]:.1f} -> {out['spikes'][1]:.1f}")
    assert change.max() > 1.0e3
    far = np.ones_like(plain, dtype=bool)
    far[49 + 42:49 + 88, 59 + 41:59 + 86] = False                       # 22 pixels and more from the centre: the wings of box and PSF are < 1
    assert plain[far].max() < 1.0 and spiked[far].max() > 10.0          # light where only an arm of the cross can have put it
    assert abs(out["spikes"][1] / out["plain"][1] - 1.0) < 0.05


def _mixed(with_boxes):
    specs = [dict(nfft=32, cx=15.37, cy=16.81, flux=2.0e6, x0=10, y0=12, obj_id=1),
             dict(nfft=64, cx=31.4, cy=30.7, flux=3.0e6, x0=60, y0=70, obj_id=2, prof_ktable=0, prof_scale=SERSIC_SCALE,
                  jac=sf.box_jac(1.0, 0.5, 37.0))]
    if with_boxes:
        specs.insert(1, dict(nfft=32, cx=16.2, cy=15.1, flux=1.5e6, x0=150, y0=20, obj_id=3, prof_ktable=-2, jac=sf.box_jac(3.0, 0.6, 37.0)))
        specs.append(dict(nfft=64, cx=30.9, cy=33.3, flux=2.5e6, x0=150, y0=150, obj_id=4, prof_ktable=-2, jac=sf.box_jac(3.0, 0.6, 90.0)))
    return cf.make_rows(specs)


def test_a_box_in_the_batch_leaves_the_other_objects_bits_alone(torch_cuda):
    """a delta, a box, a Sersic and another box on grids of 32, 32, 64, 64: workgroups of the fill whose span crosses from one object
    into the next take the per-lane lookup, the others branch on their one object's profile"""
    both, plain = _mixed(True), _mixed(False)
    assert list(both["obj_id"]) == [1, 3, 2, 4] and list(plain["obj_id"]) == [1, 2]
    _, _, s2, i2 = _draw(torch_cuda, both)
    _, _, s1, i1 = _draw(torch_cuda, plain)
    for a, b in ((0, 0), (2, 1)):
        assert_bits_equal(s2[a].view(np.float64), s1[b].view(np.float64), f"half spectrum of object {int(both['obj_id'][a])}")
        assert_bits_equal(i2[a], i1[b], f"image of object {int(both['obj_id'][a])}")
    ds, di = _deviations(both[[1, 3]], [s2[1], s2[3]], [i2[1], i2[3]])
    print(f"boxes of the mixed batch: half spectra {ds:.3e}, images {di:.3e} per unit flux")
    assert ds <= TOL_SPEC and di <= TOL_IMG


def test_a_box_clipped_by_the_ccd_edge(torch_cuda):
    """the stamp hangs over the corner (1, 1) of the CCD by 10 and 5 pixels: the CCD holds the clipped-at-zero image of the part on it"""
    rows = cf.make_rows([dict(nfft=32, x0=-9, y0=-4, cx=14.6, cy=15.3, flux=2.0e6, prof_ktable=-2, jac=sf.box_jac(3.0, 0.6, 37.0))])
    scene = configs.scene_c2(nx=96, ny=80)
    r, _, spectra, images = _draw(torch_cuda, rows, scene)
    ds, di = _deviations(rows, spectra, images)
    assert ds <= TOL_SPEC and di <= TOL_IMG
    v = np.where(images[0] < 0.0, 0.0, images[0])
    want = np.zeros((80, 96))
    want[:32 - 5, :32 - 10] = v[5:, 10:]                    # grid index 10 along x is CCD pixel 1, column 0
    got = r.image64_numpy()
    assert_bits_equal(got, want, "CCD image of the clipped box")
    assert 0.5 * 2.0e6 < got.sum() < 0.999 * 2.0e6          # most of the trail is on the chip, a visible part is not


# two trails near the boresight (pixels (104, 192) and (129, 136) of a 256^2 CCD): 2.0e6 e- in 1.0 x 0.3" and 1.5e6 e- in 20 x 1"
STREAKS = ("object 9001 60.4890 -38.1650 16.5909 flatSED/sed_flat.txt.gz 0 0 0 0 0 0 streak 1.0 0.3 37.0 none none\n"
           "object 9002 60.4925 -38.1630 16.9032 flatSED/sed_flat.txt.gz 0 0 0 0 0 0 streak 20.0 1.0 110.0 none none\n")


def test_lsst_image_config_draws_the_bright_streak_by_fft(torch_cuda, tmp_path):
    """The path a user takes: instance-catalog `streak` lines -> config.Process with image.type LSST_Image on a 256^2 CCD, the Silicon
    sensor, stamp.fft_sb_thresh, input.vignetting and stamp.diffraction_fft (the template's) -> truth record and centroid file.
    PSF: a Gaussian of FWHM 0.7" (peak 1 / 0.555 arcsec^-2): 2e6 / (0.3 + 0.555) / 2 x 0.04 = 4.7e4 per pixel > 1e4 for the short trail,
    1.5e6 / 20.6 / 2 x 0.04 = 1.5e3 for the long one.  The short trail's brightest pixel is 8.9e4, under DiffractionFFT's 1e5: no pixel
    grows spikes, and its 20-pixel stamp holds all but 2e-7 of the Gaussian-convolved trail, so that realized_flux differs from
    fft_flux by the Poisson noise alone.  (With the template's Kolmogorov PSF the stamp, sized as for every extended object from the
    box and the proxy PSF, leaves 1.8 % of the trail in the wings outside it -- 1 963 809 of 2 000 004 e- on an MI355X: the stamp-size
    rule's doing, not noise, and nothing a Poisson bound can hold.)"""
    import os
    from imsim_amd import config, truth as truthmod
    from imsim_amd.vignetting import Vignetting
    here = os.path.dirname(os.path.abspath(__file__))
    fn = tmp_path / "streaks.txt"
    with open(os.path.join(here, "golden", "example_instcat_subset.txt")) as f:
        header = "".join(line for line in f if not line.startswith("object"))          # the visit of the golden catalog
    fn.write_text(header + STREAKS)
    columns = {"object_id": "@object_id", "x": "$image_pos.x", "y": "$image_pos.y", "nominal_flux": "@nominal_flux",
               "phot_flux": "@phot_flux", "fft_flux": "@fft_flux", "realized_flux": "@realized_flux"}
    res = {}
    for method in ("auto", "phot"):
        out = tmp_path / method
        over = {"input.instance_catalog.file_name": str(fn), "input.instance_catalog.sort_mag": False, "image.xsize": 256, "image.ysize": 256,
                "stamp.fft_sb_thresh": 1.0e4, "stamp.draw_method": method, "psf": {"type": "Gaussian", "fwhm": 0.7}, "input.vignetting": {"file_name": "LSSTCam_vignetting_data.json"},
                "output.dir": str(out), "output.truth": {"dir": str(out), "file_name": "centroid.txt", "columns": columns}}
        res[method] = config.Process(os.path.join(here, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(here, "data")],
                                     overrides=over)
    a = res["auto"]
    assert a.det_names == ["R22_S11"] and a.images[0].shape == (256, 256)
    t = a.truth[0]
    assert [str(s) for s in t["object_id"]] == ["9001", "9002"]
    assert list(t["mode"]) == ["fft", "phot"]
    np.testing.assert_allclose(t["nominal_flux"], [2.0e6, 1.5e6], rtol=1e-3)
    factor = float(Vignetting("LSSTCam_vignetting_data.json").at_pixel("R22_S11", t["x"][:1], t["y"][:1], 256, 256)[0])
    assert 0.9 < factor <= 1.0
    assert t["fft_flux"][0] == t["nominal_flux"][0] * factor and t["fft_flux"][1] == 0.0
    assert t["phot_flux"][0] == 0.0 and t["phot_flux"][1] > 0.0
    print(f"fft_flux {t['fft_flux'][0]:.1f}, realized {t['realized_flux'][0]:.1f}, 5 sigma {5.0 * math.sqrt(t['fft_flux'][0]):.1f}")
    assert abs(t["realized_flux"][0] - t["fft_flux"][0]) <= 5.0 * math.sqrt(t["fft_flux"][0])
    assert a.images[0].sum() > 0.9 * (t["fft_flux"][0] + t["phot_flux"][1]) * 0.5
    rows = truthmod.read(str(tmp_path / "auto" / "centroid.txt"))
    np.testing.assert_allclose(rows["fft_flux"], t["fft_flux"], rtol=2e-8)
    np.testing.assert_allclose(rows["phot_flux"], t["phot_flux"], rtol=2e-8)
    p = res["phot"].truth[0]
    assert list(p["mode"]) == ["phot", "phot"] and not np.asarray(p["fft_flux"]).any() and (np.asarray(p["phot_flux"]) > 0).all()
