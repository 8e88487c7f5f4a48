"""Perturbed telescopes on the host: input.telescope.perturbations / focusZ parsing (the forms and errors of the reference's
tests/test_telescope_loader.py), the batoid YAML loader's frames, the Cartesian figure polynomial, the perturbed numpy
trace against closed forms, the descriptor, output.sag and the fea refusal."""
import ctypes as C
import dataclasses
import math
import textwrap

import numpy as np
import pytest
import yaml

from imsim_amd import _abi, config, fits_io, opd, optics, sag
from imsim_amd.lsst_image import GalSimConfigError

ARCMIN = math.pi / 10800.0


@pytest.fixture(scope="module")
def nominal():
    return optics.rubin_like_telescope("r")


def _ev():
    return config.Evaluator({})


def _perturbed(nominal, text):
    cfg = yaml.safe_load(textwrap.dedent(text))
    return optics.apply_perturbations(nominal, config.parse_perturbations(cfg["perturbations"], _ev()))


def _same(a, b):
    assert len(a.surfaces) == len(b.surfaces)
    for s, t in zip(a.surfaces, b.surfaces):
        assert s == t, (s.item_path, s, t)
    assert a.groups == b.groups


SHIFT_FORMS = ["""
    perturbations:
        M1: {shift: [1.e-3, 1.e-3, 0.0]}
        LSSTCamera: {shift: [0.0, 0.0, -1.e-3]}
    """, """
    perturbations:
        - M1: {shift: [1.e-3, 1.e-3, 0.0]}
          LSSTCamera: {shift: [0.0, 0.0, -1.e-3]}
    """, """
    perturbations:
        - M1: {shift: [1.e-3, 1.e-3, 0.0]}
        - LSSTCamera: {shift: [0.0, 0.0, -1.e-3]}
    """]


def test_shift_forms_give_one_telescope(nominal):
    ref = optics.shift_optic(optics.shift_optic(nominal, "M1", [1e-3, 1e-3, 0.0]), "LSSTCamera", [0.0, 0.0, -1e-3])
    for text in SHIFT_FORMS:
        _same(_perturbed(nominal, text), ref)
    assert ref.perturbed and not nominal.perturbed
    m1 = ref.surfaces[0]
    assert m1.origin == (1e-3, 1e-3, 0.0)
    det = ref.surfaces[-1]
    assert det.origin[2] == pytest.approx(nominal.surfaces[-1].z0 - 1e-3, abs=1e-15)


def test_rot_forms_and_angle_units(nominal):
    ref = optics.rotate_optic(optics.rotate_optic(nominal, "M2", optics.rot_x(1e-3)), "M2", optics.rot_y(1e-3))
    for rot in ("1.e-3 rad", "0.0572957795130823 deg"):
        texts = [f"""
            perturbations:
                M2: {{rotX: {rot}, rotY: 1.e-3 rad}}
            """, f"""
            perturbations:
                - M2: {{rotX: {rot}}}
                - M2: {{rotY: 1.e-3 rad}}
            """]
        for text in texts:
            t = _perturbed(nominal, text)
            for s, r in zip(t.surfaces, ref.surfaces):
                assert np.allclose(s.frame()[1], r.frame()[1], rtol=0, atol=1e-15)
    ev = _ev()
    assert ev.value("1 arcmin") == pytest.approx(ARCMIN, rel=1e-15)
    assert ev.value("3 arcsec") == pytest.approx(3 * ARCMIN / 60, rel=1e-15)
    assert ev.value("2 hours") == pytest.approx(math.pi / 6, rel=1e-15)
    assert ev.value("30 deg") == pytest.approx(math.pi / 6, rel=1e-15)
    with pytest.raises(GalSimConfigError):
        config.parse_perturbations({"M2": {"rotX": 0.001}}, ev)        # an angle needs a unit


def test_rotation_is_about_the_items_origin(nominal):
    t = optics.rotate_optic(nominal, "LSSTCamera", optics.rot_x(ARCMIN))
    cam_o = np.array(nominal.groups["LSSTCamera"][0])
    for s, s0 in zip(t.surfaces, nominal.surfaces):
        if not s0.item_path.startswith("LSSTCamera."):
            assert s.coaxial
            continue
        o, R = s.frame()
        assert np.allclose(R, optics.rot_x(ARCMIN), atol=1e-16)
        assert np.allclose(o - cam_o, optics.rot_x(ARCMIN) @ (np.array([0, 0, s0.z0]) - cam_o), atol=1e-15)


def test_shift_errors(nominal):
    ev = _ev()
    for bad in ([1.e-3, 1.e-3], ["a", "b", "c"], "abc"):
        with pytest.raises(ValueError):
            optics.apply_perturbations(nominal, config.parse_perturbations({"M1": {"shift": bad}}, ev))
        with pytest.raises(ValueError):
            optics.apply_perturbations(nominal, {"M1": {"shift": bad}})


def test_zernike_forms_radii_and_errors(nominal):
    ref = optics.figure_optic(optics.figure_optic(nominal, "M1", [0.0] * 4 + [1e-7], 4.18, 2.558), "M2", [0.0] * 5 + [2e-7],
                              1.71, 0.9)
    forms = ["""
        perturbations:
            M1: {Zernike: {coef: [0.0, 0.0, 0.0, 0.0, 1.e-7]}}
            M2: {Zernike: {coef: [0.0, 0.0, 0.0, 0.0, 0.0, 2.e-7]}}
        """, """
        perturbations:
            - M1: {Zernike: {coef: [0.0, 0.0, 0.0, 0.0, 1.e-7]}}
            - M2: {Zernike: {coef: [0.0, 0.0, 0.0, 0.0, 0.0, 2.e-7]}}
        """, """
        perturbations:
            M1: {Zernike: {idx: 4, val: 1.e-7}}
            M2: {Zernike: {idx: 5, val: 2.e-7}}
        """]
    for text in forms:
        _same(_perturbed(nominal, text), ref)
    assert ref.surfaces[0].figure[0].r_outer == 4.18 and ref.surfaces[0].figure[0].r_inner == 2.558   # from the optic
    two = ["""
        perturbations:
            M1: {Zernike: {coef: [0.0, 0.0, 0.0, 0.0, 1.e-7, 3.e-7], R_outer: 1.2, R_inner: 0.6}}
        """, """
        perturbations:
            M1: {Zernike: {idx: [4, 5], val: [1.e-7, 3.e-7], R_outer: 1.2, R_inner: 0.6}}
        """]
    a, b = (_perturbed(nominal, t) for t in two)
    _same(a, b)
    assert a.surfaces[0].figure == (optics.Figure((0.0, 0.0, 0.0, 0.0, 1e-7, 3e-7), 1.2, 0.6),)
    ev = _ev()
    with pytest.raises(ValueError, match="both or neither"):
        config.parse_perturbations({"M1": {"Zernike": {"idx": 4, "val": 1e-7, "R_outer": 1.2}}}, ev)
    with pytest.raises(ValueError, match="both coef and idx"):
        config.parse_perturbations({"M1": {"Zernike": {"idx": 4, "val": 1e-7, "coef": [0.0, 1.0]}}}, ev)
    with pytest.raises(ValueError, match="both or neither"):
        optics.apply_perturbations(nominal, {"M1": {"Zernike": {"idx": 4, "val": 1e-7, "R_inner": 0.5}}})
    with pytest.raises(ValueError):
        optics.apply_perturbations(nominal, {"L1": {"Zernike": {"idx": 4, "val": 1e-7}}})      # a lens is not an interface
    with pytest.raises(ValueError):
        optics.apply_perturbations(nominal, {"M7": {"shift": [0.0, 0.0, 1e-3]}})              # no such optic
    with pytest.raises(ValueError):
        optics.apply_perturbations(nominal, {"M1": {"tilt": 1e-3}})                          # no such perturbation


def test_item_names_resolve_like_batoid(nominal):
    assert optics.resolve_item(nominal, "L1_entrance") == "LSSTCamera.L1.L1_entrance"
    assert optics.resolve_item(nominal, "LSSTCamera.L1") == "LSSTCamera.L1"
    assert optics.resolve_item(nominal, nominal.name + ".M2") == "M2"
    assert optics.resolve_item(nominal, "Detector") == "LSSTCamera.Detector"


def test_zero_perturbations_leave_the_telescope_coaxial(nominal):
    t = optics.apply_perturbations(nominal, [{"M2": {"shift": [0.0, 0.0, 0.0], "rotX": 0.0}},
                                             {"M1": {"Zernike": {"idx": [4, 11], "val": [0.0, 0.0]}}}])
    t = optics.focus_camera(t, 0.0)
    _same(t, nominal)
    o = optics.make_optics(t, (100.0, 0.0, 2048.0, 0.0, 100.0, 2002.0), 0.3)
    assert type(o) is _abi.Optics
    ref = _abi.Optics()
    optics.fill_optics(ref, nominal, (100.0, 0.0, 2048.0, 0.0, 100.0, 2002.0), 0.3)
    assert bytes(o) == bytes(ref)


def test_perturbation_structs_match_the_library():
    lib = _abi.load()
    assert lib.ims_struct_size(_abi.OPTICS_PERTURBED_STRUCT_INDEX) == C.sizeof(_abi.OpticsPerturbed)
    assert lib.ims_struct_size(_abi.PERTURBATION_STRUCT_INDEX) == C.sizeof(_abi.Perturbation)
    assert C.sizeof(_abi.OpticsPerturbed) == C.sizeof(_abi.Optics) + C.sizeof(_abi.Perturbation)
    assert _abi.OpticsPerturbed.pert.offset == C.sizeof(_abi.Optics)
    assert _abi.OpticsPerturbed not in _abi.STRUCTS and lib.ims_abi_version() == 22


def test_descriptor_of_a_perturbed_telescope(nominal):
    t = optics.apply_perturbations(nominal, [{"M2": {"shift": [1e-4, 0.0, 0.0]}}, {"M1": {"Zernike": {"idx": 7, "val": 1e-7}}}])
    o = optics.make_optics(t, (100.0, 0.0, 2048.0, 0.0, 100.0, 2002.0), 0.4)
    assert isinstance(o, _abi.OpticsPerturbed)
    assert (o.cam_rot[0], o.cam_rot[1]) == (1.0, 0.0)                 # the rotator is in the camera's frames
    assert o.pert.surf[1].moved == 1 and list(o.pert.surf[1].origin) == [1e-4, 0.0, t.surfaces[1].z0]
    assert o.pert.surf[0].moved == 0 and o.pert.surf[0].fig_deg == 3
    assert o.pert.surf[0].fig_inv_r == 1.0 / 4.18
    det = o.pert.surf[len(t.surfaces) - 1]
    R = np.array(det.rot).reshape(3, 3)
    assert det.moved == 1 and np.allclose(R, optics.rot_z(0.4), atol=1e-16)
    with pytest.raises(ValueError):
        optics.fill_optics(_abi.Optics(), t, (100.0, 0.0, 2048.0, 0.0, 100.0, 2002.0))


def test_cartesian_figure_matches_the_annular_zernikes():
    """the Cartesian expansion against opd.py's basis evaluated directly: 1e-14 relative to max |Z_j| for Noll 1 .. 21; from
    Noll 22 on the power-basis coefficients grow (Z22: |C| ~ 900) and both evaluations round at that scale"""
    rng = np.random.default_rng(0)
    R, eps = 4.18, 0.612
    r = np.sqrt(rng.uniform((eps * R) ** 2, R ** 2, 4000))
    a = rng.uniform(0.0, 2.0 * np.pi, 4000)
    x, y = r * np.cos(a), r * np.sin(a)
    Z = opd.zernike_basis(66, x, y, R, eps)
    for j in range(1, 67):
        coef = [0.0] * (j + 1)
        coef[j] = 1.0
        fig = optics.Figure(tuple(coef), R, eps * R)
        f, fx, fy = fig(x, y)
        scale = np.abs(Z[j - 1]).max()
        bound = 1e-14 * (1.0 if j <= 21 else max(1.0, np.abs(fig.cartesian()).max()))
        assert np.abs(f - Z[j - 1]).max() <= bound * scale, j
        if j in (4, 7, 11, 22):                          # the gradient by finite differences
            h = 1e-6
            gx = (fig(x + h, y)[0] - fig(x - h, y)[0]) / (2 * h)
            gy = (fig(x, y + h)[0] - fig(x, y - h)[0]) / (2 * h)
            assert np.allclose(fx, gx, rtol=0, atol=1e-7 * scale) and np.allclose(fy, gy, rtol=0, atol=1e-7 * scale)


def _rays(tel, n=20000, seed=1):
    rng = np.random.default_rng(seed)
    r = np.sqrt(rng.uniform(tel.pupil_inner ** 2, tel.pupil_outer ** 2, n))
    a = rng.uniform(0, 2 * np.pi, n)
    pos = np.stack([r * np.cos(a), r * np.sin(a), np.full(n, tel.stop_z)], 1)
    th = np.deg2rad(1.5) * np.sqrt(rng.uniform(0, 1, n))
    ph = rng.uniform(0, 2 * np.pi, n)
    thx, thy = np.tan(th) * np.cos(ph), np.tan(th) * np.sin(ph)
    g = 1 / np.sqrt(1 + thx ** 2 + thy ** 2)
    return pos, np.stack([thx * g, thy * g, -g], 1), rng.uniform(540, 700, n)


def _z_moved(tel, dz, which):
    return dataclasses.replace(tel, surfaces=[dataclasses.replace(S, z0=S.z0 + dz) if which(S) else dataclasses.replace(S)
                                              for S in tel.surfaces])


def _agree(a, b, tol=1e-12):
    (pa, va, ga, fa), (pb, vb, gb, fb) = a, b
    assert np.array_equal(ga | fa, gb | fb)
    ok = ~(ga | fa)
    assert ok.sum() > 1000
    assert np.abs(pa[ok, :2] - pb[ok, :2]).max() <= tol
    ua = va[ok] / np.linalg.norm(va[ok], axis=1)[:, None]
    ub = vb[ok] / np.linalg.norm(vb[ok], axis=1)[:, None]
    assert np.abs(ua - ub).max() <= 1e-12


def test_perturbed_trace_closed_forms(nominal):
    pos, vel, wave = _rays(nominal)
    tr = lambda t, **k: optics.trace_numpy(t, pos, vel, wave, **k)
    dz = 3e-5
    in_camera = lambda S: S.item_path.startswith("LSSTCamera.")
    # Detector: shift [0, 0, dz] == the detector at z0 + dz
    _agree(tr(optics.apply_perturbations(nominal, {"Detector": {"shift": [0, 0, dz]}}), local_last=True),
           tr(_z_moved(nominal, dz, lambda S: S.name == "Detector")))
    # LSSTCamera: shift [0, 0, dz] and focusZ = dz == every camera surface at z0 + dz
    cam = tr(_z_moved(nominal, dz, in_camera))
    _agree(tr(optics.apply_perturbations(nominal, {"LSSTCamera": {"shift": [0, 0, dz]}}), local_last=True), cam)
    _agree(tr(optics.focus_camera(nominal, dz), local_last=True), cam)
    # a Zernike piston delta on M2 == M2 shifted by [0, 0, delta]
    d = 1e-6
    _agree(tr(optics.apply_perturbations(nominal, {"M2": {"Zernike": {"idx": 1, "val": d}}})),
           tr(optics.apply_perturbations(nominal, {"M2": {"shift": [0, 0, d]}})))
    _agree(tr(optics.apply_perturbations(nominal, {"M2": {"Zernike": {"idx": 1, "val": d}}})),
           tr(_z_moved(nominal, d, lambda S: S.name == "M2")))
    # LSSTCamera: rotZ theta == rotTelPos theta, on the pixels of field_to_pixel
    th = 0.3
    fp = (100.0, 0.0, 2048.0, 0.0, 100.0, 2002.0)
    rz = optics.apply_perturbations(nominal, {"LSSTCamera": {"rotZ": th}})
    for f in ((0.0, 0.0), (0.01, 0.005), (-0.02, 0.012)):
        a = optics.field_to_pixel(rz, f[0], f[1], fp)
        b = optics.field_to_pixel(nominal, f[0], f[1], fp, rot_tel_pos=th)
        assert np.abs(np.subtract(a, b)).max() <= 1e-12 / 10e-6                 # 1e-12 m in 10 um pixels


def test_perturbation_moves_the_image(nominal):
    fp = (100.0, 0.0, 2048.0, 0.0, 100.0, 2002.0)
    t = optics.apply_perturbations(nominal, {"M2": {"shift": [1e-4, 0.0, 0.0]}})
    a = np.array(optics.field_to_pixel(t, 0.0, 0.0, fp))
    b = np.array(optics.field_to_pixel(nominal, 0.0, 0.0, fp))
    assert np.hypot(*(a - b)) > 5.0                                  # a 100 um decentre of M2 moves the image by pixels


YAML = """
opticalSystem:
  type: CompoundOptic
  name: T
  inMedium: 1.0
  pupilSize: 2.0
  pupilObscuration: 0.3
  stopSurface: {{type: Interface, surface: {{type: Plane}}, coordSys: {{z: 0.5}}}}
  items:
    - type: Mirror
      name: M
      surface: {{type: Paraboloid, R: 8.0}}
      obscuration: {{type: ClearAnnulus, inner: 0.3, outer: 1.0}}
    - type: CompoundOptic
      name: Cam
      coordSys: {{x: {cx}, y: {cy}, z: 3.9, rotX: {rx}}}
      items:
        - type: Detector
          name: D
          surface: {{type: Plane}}
          coordSys: {{z: 0.1, rotZ: {rz}}}
          obscuration: {{type: ClearCircle, radius: 0.2}}
"""


def test_yaml_loader_takes_coordsys_offsets_and_rotations(tmp_path):
    p0, p1 = tmp_path / "a.yaml", tmp_path / "b.yaml"
    p0.write_text(YAML.format(cx=0.0, cy=0.0, rx=0.0, rz=0.0))
    p1.write_text(YAML.format(cx=1e-3, cy=-2e-3, rx=1e-3, rz=0.2))
    t0, t1 = optics.load_batoid_yaml(str(p0)), optics.load_batoid_yaml(str(p1))
    assert not t0.perturbed and t1.perturbed
    assert [S.item_path for S in t1.surfaces] == ["M", "Cam.D"] and "Cam" in t1.groups
    # the same telescope through the perturbations: shift the camera, turn it about its origin, turn the detector
    t2 = optics.apply_perturbations(t0, [{"Cam": {"shift": [1e-3, -2e-3, 0.0]}}, {"Cam": {"rotX": 1e-3}},
                                         {"D": {"rotZ": 0.2}}])
    for a, b in zip(t1.surfaces, t2.surfaces):
        oa, Ra = a.frame()
        ob, Rb = b.frame()
        assert np.allclose(oa, ob, rtol=0, atol=1e-15) and np.allclose(Ra, Rb, rtol=0, atol=1e-15)
    pos, vel = optics.pupil_rays(t1, 0.001, 0.0)
    a, b = optics.trace_numpy(t1, pos, vel, 620.0), optics.trace_numpy(t2, pos, vel, 620.0)
    assert np.abs(a[0] - b[0]).max() < 1e-12 and np.array_equal(a[2], b[2])


def test_sag_output(nominal, tmp_path):
    t = optics.apply_perturbations(nominal, [{"M2": {"shift": [1e-4, 0.0, 0.0]}}, {"M1": {"Zernike": {"idx": 4, "val": 1e-7}}}])
    maps = sag.compute(t, nx=63)
    assert len(maps) == len(t.surfaces)
    m1, h1 = maps[0]
    assert h1["name"][0] == t.name + ".M1" and h1["telescop"][0] == t.name and h1["units"][0] == "m"
    assert all(k in h1 for k in sag.HEADER_KEYS)
    xs = np.linspace(-1, 1, 63) * 4.18
    xx, yy = np.meshgrid(xs, xs)
    rr = np.hypot(xx, yy)
    assert np.array_equal(np.isnan(m1), (rr > 4.18) | (rr < 2.558))
    good = np.isfinite(m1)
    plain = sag.surface_sag(nominal.surfaces[0], xx[good], yy[good])
    fig = optics.Figure((0.0,) * 4 + (1e-7,), 4.18, 2.558)(xx[good], yy[good])[0]
    assert np.allclose(m1[good], plain + fig, rtol=0, atol=1e-15)
    m2, h2 = maps[1]
    assert h2["x0"][0] == 1e-4 and h2["R00"][0] == 1.0 and h2["dx"][0] == pytest.approx(2 * 1.71 / 62, rel=1e-14)
    fn = str(tmp_path / "sag.fits")
    sag.write(fn, maps)
    hdus = fits_io.read_fits(fn)
    assert len(hdus) == len(maps)
    assert hdus[1][0]["X0"] == 1e-4 and np.array_equal(np.isnan(hdus[0][1]), np.isnan(m1))


def test_process_config_errors():
    ev = _ev()
    with pytest.raises(GalSimConfigError, match="batoid_rubin"):
        config.build_telescope({"fea": {"m1m3TBulk": 0.1}}, ev, "r")
    with pytest.raises(GalSimConfigError):
        config.parse_perturbations({"M1": {"wobble": 1.0}}, ev)
    t = config.build_telescope({"perturbations": {"M2": {"shift": [1e-4, 0.0, 0.0]}}, "focusZ": 1e-5}, ev, "r")
    assert t.perturbed and t.surfaces[-1].origin[2] == pytest.approx(optics.rubin_like_telescope("r").surfaces[-1].z0 + 1e-5)
    with pytest.raises(GalSimConfigError, match="file_name"):
        config._process_sag({"nx": 32}, ev, {}, t, config.ProcessResult())
