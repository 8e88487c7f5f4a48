"""The optical phase screen of AtmosphericPSF(doOpt=True) on the GPU (IMS_PSF_OPTICAL_SCREEN, csrc/ims_optical.h): the device
functions against the numpy restatement bit for bit, the invariants of the RNG addressing with the component on, the null state,
and two known answers (defocus on the pupil side, astigmatism that changes sign over the field)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import optical_screen_numpy as R
from imsim_amd import _abi, atm_psf, catalog, configs, diffraction, optical_system, optics

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden")
EPS, R_OUT, LAM0 = 0.61, 4.18, 500.0
KICK = 1.0e-9 * atm_psf.ARCSEC                      # arcsec per (nm/m), the screens' conversion


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _scene(optical=None, n=256, sensor=False, seed=398414):
    return configs.scene_c3b(nx=n, ny=n, seed=seed, sensor=sensor, screen_size=102.4, screen_scale=0.1, optical=optical)


def _objects(scene, n_obj=100, flux_seed=2, n=256):
    cat = catalog.synthetic_catalog(n_obj, nx=n, ny=n)
    phot = catalog.realize_fluxes(cat["nominal_flux"], flux_seed)
    return configs.c3b_objects(cat, phot, scene)[0]


def _render(scene, objects, how="fused", lsst=False):
    from imsim_amd.engine import Renderer
    r = Renderer(scene)
    if lsst:
        r.render_lsst_image(objects, nrecalc=3000)
    elif how == "fused":
        r.render(objects)
    elif how == "pooled":
        pool = r.shoot_photons(objects)
        r.apply_ops(pool)
        r.accumulate(pool)
    else:                                            # the photons of every object in `how` batches, one render each
        F = objects["n_phot"].copy()
        for i in range(how):
            part = objects.copy()
            lo, hi = (F * i) // how, (F * (i + 1)) // how
            part["phot_first"], part["n_phot"] = lo, hi - lo
            r.render(part[part["n_phot"] > 0])
    r.synchronize()
    return r.image_numpy()


ON = dict(doOpt=True, data_dir=DATA)


def test_device_functions_match_the_restatement_bit_for_bit(torch_cuda):
    """ims_test_optical_screen against tests/optical_screen_numpy.py on 12 000 random (theta, u, v), |theta| <= 1.75 deg, (u, v)
    in the annulus, for a drawn visit state: the 19 coefficients and both gradient components, every bit.  The restatement
    follows the documented order; the fma steps of the per-photon Horner are emulated exactly (rational arithmetic)."""
    torch = torch_cuda
    lib = _abi.load()
    S = optical_system.visit_optical_state(1234, DATA).screen_struct()
    rng = np.random.default_rng(11)
    n = 12_000
    thx = np.radians(rng.uniform(-1.75, 1.75, n))
    thy = np.radians(rng.uniform(-1.75, 1.75, n))
    rr = np.sqrt(rng.uniform((EPS * R_OUT) ** 2, R_OUT ** 2, n))
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    u, v = rr * np.cos(ang), rr * np.sin(ang)
    dev = torch.device("cuda:0")
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    S_dev = put(np.frombuffer(bytes(S), dtype=np.uint8).copy())
    t = [put(a) for a in (thx, thy, u, v)]
    coef = torch.empty((n, 19), dtype=torch.float64, device=dev)
    du, dv = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    _abi.check(lib.ims_test_optical_screen(S_dev.data_ptr(), *[x.data_ptr() for x in t], n, coef.data_ptr(), du.data_ptr(),
                                           dv.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "ims_test_optical_screen")
    torch.cuda.synchronize(dev)
    a_ref, du_ref, dv_ref = R.evaluate(S, thx, thy, u, v)
    got_a, got_du, got_dv = coef.cpu().numpy(), du.cpu().numpy(), dv.cpu().numpy()
    print("max |coef|", np.abs(got_a).max(), "max |grad| nm/m", np.abs(got_du).max(),
          "differing: coef", int((got_a != a_ref).sum()), "du", int((got_du != du_ref).sum()), "dv", int((got_dv != dv_ref).sum()))
    assert np.abs(got_a).max() > 0.01 and np.abs(got_du).max() > 1.0
    assert got_a.tobytes() == a_ref.tobytes()
    assert got_du.tobytes() == du_ref.tobytes() and got_dv.tobytes() == dv_ref.tobytes()


def test_doopt_changes_the_image_and_keeps_the_rng_invariants(torch_cuda):
    """doOpt is no longer dropped: the image differs from the doOpt-false one, and is bit-identical between two runs, between
    the fused and the pooled path, and between one batch and three (unit fluxes, no sensor: the f64 image is a sum of ones)."""
    off, on = _scene(None), _scene(ON)
    objects = _objects(on)
    img_off = _render(off, objects)
    img_on = _render(on, objects)
    assert img_on.sum() > 0 and img_on.tobytes() != img_off.tobytes()
    assert _render(on, objects).tobytes() == img_on.tobytes()
    assert _render(on, objects, "pooled").tobytes() == img_on.tobytes()
    assert _render(on, objects, 3).tobytes() == img_on.tobytes()


def test_null_state_is_the_doopt_false_image(torch_cuda):
    """zero deviations without the nominal term: a zero kick is added to every photon and moves none, and the components behind
    the optical screen draw the deviates they draw without it -- the image of doOpt false, bit for bit, with and without the
    Silicon sensor (LSST_Image plan: both specialised kernels)."""
    null = dict(ON, optical_deviations=np.zeros(50), optical_nominal=False)
    for sensor in (False, True):
        off, on = _scene(None, sensor=sensor), _scene(null, sensor=sensor)
        if sensor:
            off.sensor.scratch_cells = on.sensor.scratch_cells = 500_000
        assert np.all(on.atm.opt.field_matrix == 0.0) and any(int(c[0]) == _abi.IMS_PSF_OPTICAL_SCREEN for c in on.psf)
        objects = _objects(on)
        a, b = _render(off, objects, lsst=sensor), _render(on, objects, lsst=sensor)
        assert a.sum() > 0 and a.tobytes() == b.tobytes()


def _single_term_scene(rows):
    """a scene whose optical screen is set by hand: rows = {(Zernike row, field monomial): value}, nothing else"""
    sc = _scene(dict(ON, optical_deviations=np.zeros(50), optical_nominal=False))
    for (j, t), val in rows.items():
        sc.atm.opt.field_matrix[j, t] = val
    sc.psf = [sc.atm.optical_component()]
    sc.ops = []
    return sc


def test_defocus_is_a_radial_linear_kick(torch_cuda):
    """Only a_4 (annular defocus) non-zero, no other PSF component, point sources, no sensor, the photon pool read back:
    Z4 = sqrt 3 (2 rho^2 - 1 - eps^2) / (1 - eps^2), so grad W = lam0 a_4 4 sqrt 3 / ((1 - eps^2) R^2) (u, v) and every photon
    lands at x0 + winv g (u, v) with g that constant times 1e-9 * 206264.8.

    Bound per coordinate: the device rounds u / R, two Horner steps, grad_scale, p0, three operations of winv (u, v) and the
    monomial coefficient itself carries the rounding of the expansion -- 16 roundings relative to the kick is generous --
    and then adds the kick to the profile position and that to x0: two roundings at the size of the pixel coordinate
    (< 512, half an ulp each: 2^-44 together).  tol = 2^-44 + 16 * 2^-53 * |kick|."""
    from imsim_amd.engine import Renderer
    a4 = 12.0
    sc = _single_term_scene({(0, 0): a4})
    objects = _objects(sc, n_obj=40)
    objects["prof_table"] = _abi.IMS_PROF_POINT
    objects["stamp_xmin"], objects["stamp_ymin"], objects["stamp_xmax"], objects["stamp_ymax"] = -10000, -10000, 10000, 10000
    k = int(np.argmin(np.hypot(objects["x0"] - 128.0, objects["y0"] - 128.0)))      # the star nearest the centre, made bright
    objects["n_phot"][k] = 20_000
    r = Renderer(sc)
    pool = r.shoot_photons(objects)
    r.synchronize()
    p = pool.to_host()
    o = objects[p["obj_index"]]
    g = KICK * LAM0 * a4 * 4.0 * math.sqrt(3.0) / ((1.0 - EPS ** 2) * R_OUT ** 2)        # arcsec per m
    ku, kv = g * p["pupil_u"], g * p["pupil_v"]
    ex = o["winv"][:, 0] * ku + o["winv"][:, 1] * kv
    ey = o["winv"][:, 2] * ku + o["winv"][:, 3] * kv
    rad = np.hypot(p["pupil_u"], p["pupil_v"])
    assert len(rad) > 10_000 and rad.min() >= EPS * R_OUT * (1 - 1e-12) and rad.max() <= R_OUT * (1 + 1e-12)
    dx, dy = p["x"] - (o["x0"] + ex), p["y"] - (o["y0"] + ey)
    tol_x, tol_y = 2.0 ** -44 + 16 * 2.0 ** -53 * np.abs(ex), 2.0 ** -44 + 16 * 2.0 ** -53 * np.abs(ey)
    print("max |dx|, |dy| [px]", np.abs(dx).max(), np.abs(dy).max(), "max kick [px]", np.abs(ex).max(), "min tol", tol_x.min())
    assert np.abs(ex).max() > 5.0
    assert np.all(np.abs(dx) <= tol_x) and np.all(np.abs(dy) <= tol_y)
    # the image of one star is an annulus of radius ratio 0.61: in the sky plane (winv undone) exactly so per photon
    sel = p["obj_index"] == k
    w = objects["winv"][k].reshape(2, 2)
    sky = np.linalg.solve(w, np.stack([p["x"][sel] - objects["x0"][k], p["y"][sel] - objects["y0"][k]]))
    rs = np.hypot(sky[0], sky[1])
    assert sel.sum() > 1000
    assert rs.min() >= g * EPS * R_OUT * (1 - 1e-9) and rs.max() <= g * R_OUT * (1 + 1e-9)
    assert rs.min() / rs.max() < EPS * 1.02                       # and both edges are reached (> 1000 photons)
    # ... and on the pixels: every lit pixel of that star alone lies within half a pixel diagonal of the annulus
    one = objects[k:k + 1].copy()
    img = _render(sc, one)
    jj, ii = np.nonzero(img)
    s = np.linalg.svd(w, compute_uv=False)
    rp = np.hypot(ii + 1 - one["x0"][0], jj + 1 - one["y0"][0])
    assert img.sum() == one["n_phot"][0]
    assert rp.min() >= s.min() * g * EPS * R_OUT - 0.7072 and rp.max() <= s.max() * g * R_OUT + 0.7072
    assert img[int(round(one["y0"][0])) - 1, int(round(one["x0"][0])) - 1] == 0          # the hole


def test_astigmatism_linear_in_thx_flips_the_ellipticity(torch_cuda):
    """Field side.  A kick that is a pure astigmatism, (k u, -k v), has equal second moments in u and v for either sign of k (the
    moments are quadratic in the coefficient), so a single aberration term cannot give ellipticities of opposite sign: the sign
    comes from the cross term with defocus, as in the real states.  State: constant a_4 = d and a_6 = c * thx.  Then the kick
    is (A u, B v), A = g4 d + g6 a_6, B = g4 d - g6 a_6 with g4 = 4 sqrt 3 / (1 - eps^2), g6 = 2 sqrt 6 / sqrt(1 + eps^2 + eps^4)
    (annular Z6 = sqrt 6 rho^2 cos 2t / sqrt(1 + eps^2 + eps^4), Mahajan 1981), <u^2> = <v^2> over the annulus, and
    e1 = (A^2 - B^2) / (A^2 + B^2): opposite at +thx and -thx, zero on axis.  Checked on the photons' sky-plane offsets to 4 sigma,
    sigma from the delta method on the photon count."""
    from imsim_amd.engine import Renderer
    d, c, th_deg = 4.0, 2.0, 1.0
    sc = _single_term_scene({(0, 0): d, (2, 1): c})                  # row 2 = Z6, monomial 1 = thx
    objects = _objects(sc, n_obj=60)
    objects = objects[np.argsort(objects["n_phot"])[-3:]].copy()
    objects["prof_table"] = _abi.IMS_PROF_POINT
    objects["atm_tan_x"] = np.radians([th_deg, -th_deg, 0.0])
    objects["atm_tan_y"] = 0.0
    r = Renderer(sc)
    pool = r.shoot_photons(objects)
    r.synchronize()
    p = pool.to_host()
    g4, g6 = 4.0 * math.sqrt(3.0) / (1.0 - EPS ** 2), 2.0 * math.sqrt(6.0) / math.sqrt(1.0 + EPS ** 2 + EPS ** 4)
    a6 = c * th_deg * optical_system.THETA_REMAP
    A, B = g4 * d + g6 * a6, g4 * d - g6 * a6
    e_pred = (A * A - B * B) / (A * A + B * B)
    assert e_pred > 0.2
    for k, want in enumerate((e_pred, -e_pred, 0.0)):
        sel = p["obj_index"] == k
        w = objects["winv"][k].reshape(2, 2)
        su, sv = np.linalg.solve(w, np.stack([p["x"][sel] - objects["x0"][k], p["y"][sel] - objects["y0"][k]]))
        n = sel.sum()
        q, s = su * su - sv * sv, su * su + sv * sv
        e1 = q.mean() / s.mean()
        sigma = np.std(q - e1 * s) / (math.sqrt(n) * s.mean())
        print(f"star {k}: n {n} e1 {e1:+.5f} predicted {want:+.5f} sigma {sigma:.5f}")
        assert n > 2000 and abs(e1 - want) < 4.0 * sigma
        e2 = (2.0 * su * sv).mean() / s.mean()
        assert abs(e2) < 4.0 * np.std(2.0 * su * sv - e2 * s) / (math.sqrt(n) * s.mean())


def test_c3b_and_perturbed_telescope_run_with_the_component(torch_cuda):
    """The six-screen C3b configuration through the LSST_Image plan (Silicon sensor: the kernels specialised for the default
    chain, layout and AtmosphericPSF with doOpt) and the perturbed-telescope layout (the loops), each once with the component on:
    the image differs from off and is the same run to run."""
    for perturbed in (False, True):
        scenes = []
        for opt in (None, ON):
            sc = _scene(opt, sensor=True)
            sc.sensor.scratch_cells = 500_000
            if perturbed:
                tel = optics.apply_perturbations(optics.rubin_like_telescope(configs.VISIT["band"]),
                                                 [{"M2": {"shift": [50e-6, 0.0, 0.0]}}])
                n = 256
                fp = (100.0, 0.0, (n - 1) / 2.0 + 0.5, 0.0, 100.0, (n - 1) / 2.0 + 0.5)
                po = optics.make_optics(tel, fp, math.radians(configs.VISIT["rottelpos"]))
                assert isinstance(po, _abi.OpticsPerturbed)
                po.img_wcs, po.icrf_to_field = sc.optics.img_wcs, sc.optics.icrf_to_field
                diffraction.fill_optics(po, math.radians(configs.VISIT["latitude"]), math.radians(configs.VISIT["azimuth"]),
                                        math.radians(configs.VISIT["altitude"]))
                sc.optics = po
            scenes.append(sc)
        objects = _objects(scenes[1], n_obj=80)
        off = _render(scenes[0], objects, lsst=True)
        on = _render(scenes[1], objects, lsst=True)
        assert on.sum() > 0 and np.all(np.isfinite(on)) and on.tobytes() != off.tobytes()
        assert _render(scenes[1], objects, lsst=True).tobytes() == on.tobytes()


@pytest.mark.parametrize("itype", ["LSST_Image", "LSST_PhotonPoolingImage"])
def test_process_passes_doopt_on(torch_cuda, tmp_path, itype):
    """config.Process: input.atm_psf.doOpt reaches the photons (before, the key was accepted and dropped) in both image types,
    save_file is reported.  Photon pooling runs without stamp.fft_sb_thresh: with it the config is refused (CPU test)."""
    from imsim_amd import config

    def run(sub, do_opt):
        o = {"input.instance_catalog.file_name": os.path.join(HERE, "golden", "example_instcat_subset.txt"),
             "image.nobjects": 40, "stamp.draw_method": "phot", "output.dir": str(tmp_path / sub),
             "input.atm_psf": {"airmass": 1.1, "rawSeeing": 0.7, "band": "r", "boresight": "unused", "screen_size": 102.4, "doOpt": do_opt,
                               "save_file": "atm.pkl"},
             "psf.items.0": {"type": "AtmosphericPSF"}}
        if itype != "LSST_Image":
            o.update({"image.type": itype, "stamp.type": "LSST_Photons", "input.checkpoint": "", "stamp.fft_sb_thresh": 0.0})
        return config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")],
                              overrides=o, data_dir=str(data_dir))
    # a data directory with everything the package ships plus the three optics tables of the fixtures
    data_dir = tmp_path / "data"
    data_dir.mkdir()
    for name in os.listdir(configs.DATA_DIR):
        os.symlink(os.path.join(configs.DATA_DIR, name), data_dir / name)
    os.symlink(os.path.join(DATA, "optics_data"), data_dir / "optics_data")
    on, off = run("on", True), run("off", False)
    assert on.images[0].sum() > 0 and on.images[0].tobytes() != off.images[0].tobytes()
    assert any("save_file" in s for s in on.ignored) and not any("doOpt" in s for s in on.ignored)
