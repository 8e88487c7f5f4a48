"""The cases of tests/test_opd_ref.py (reference alone, CPU) and tests/test_opd_ref_gpu.py (ims_opd against tests/opd_ref.py).

Grids, against the 256-ray block of the trace, the 64-pixel tile and the 4096-pixel chunk of k_opd_zk_normal: nx = 5 (fewer
finite pixels than jmax), 15 (225 rays: one partly filled block whose last tile holds 33 pixels), 16 (exactly one block), 17,
64 (exactly one chunk), 65 (a second chunk of 129 pixels: two tiles and one pixel), 91 (three chunks: the chunk-order sum of
k_opd_zk_final).  jmax = 66 (nine packed entries per thread) goes with nx = 65 and 91 only.  OUT lies outside the field of view:
every pixel ray is vignetted or lost, the map is all NaN and the normal equations are all zeros; in the four-field calls it
sits between good fields.  Every map is a few thousand rays."""
import math

from imsim_amd import _abi, optics

DEG = math.pi / 180.0
ARCMIN = math.pi / 10800.0
F0, F1, F2, OUT = (0.0, 0.0), (0.5 * DEG, 0.3 * DEG), (1.2 * DEG, -0.8 * DEG), (3.0 * DEG, 1.0 * DEG)
FOUR = [F0, F1, OUT, F2]
WAVE = 622.0


def one_mirror(conic=-1.0, det_z=10.0, R=20.0):
    """one mirror (R = 20 m, clear annulus 0.1 .. 0.5 m), stop at z = 1 m, a detector plane at the focus"""
    surf = [optics.Surface(_abi.IMS_SURF_MIRROR, 0.0, R, conic, (), _abi.IMS_OBSC_CLEAR_ANNULUS, 0.1, 0.5, name="M"),
            optics.Surface(_abi.IMS_SURF_DETECTOR, det_z, name="Detector")]
    return optics.Telescope(surf, stop_z=1.0, pupil_outer=0.5, pupil_inner=0.1, name="one_mirror", sphere_radius=10.0, eps=0.2)


def _m2(tel):
    return optics.apply_perturbations(tel, {"M2": {"shift": [100e-6, -60e-6, 0.0], "rotX": ARCMIN, "rotY": -0.5 * ARCMIN}})


def _camera(tel):
    return optics.apply_perturbations(tel, {"LSSTCamera": {"rotX": 0.5 * ARCMIN, "shift": [0.0, -30e-6, 0.0]}})


def _m1_figure(tel):
    return optics.apply_perturbations(tel, [{"M1": {"Zernike": {"idx": [5, 11], "val": [0.3e-6, -0.2e-6]}}},
                                            {"M2": {"rotY": ARCMIN}}])


_TEL = {}


def telescope(name):
    if name not in _TEL:
        if name == "one_mirror":
            _TEL[name] = one_mirror()
        else:
            nominal = _TEL.setdefault("rubin", optics.rubin_like_telescope())
            _TEL[name] = {"rubin": lambda t: t, "m2": _m2, "camera": _camera, "m1_figure": _m1_figure}[name](nominal)
    return _TEL[name]


def descriptor(tel):
    """the optics block as opd.compute uploads it (rot_tel_pos = 0)"""
    return optics.make_optics(tel, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), 0.0)


def _case(name, tel, fields, nx, projection="postel", reference="chief", sphere_radius=None, jmax=28, direct=False):
    return dict(name=name, tel=tel, fields=list(fields), nx=nx, projection=projection, reference=reference,
                sphere_radius=sphere_radius, jmax=jmax, direct=direct)


CASES = [
    _case("rubin_nx5_rank_deficient", "rubin", [F0], 5),
    _case("rubin_nx15_gnomonic_mean", "rubin", [F1], 15, "gnomonic", "mean", jmax=2),
    _case("rubin_nx16_zemax", "rubin", [F2], 16, "zemax", jmax=1),
    _case("rubin_nx17_four_mean", "rubin", FOUR, 17, "postel", "mean", sphere_radius=10.0),
    _case("rubin_nx64_gnomonic", "rubin", [F2], 64, "gnomonic"),
    _case("rubin_nx65_four_j66", "rubin", FOUR, 65, "zemax", jmax=66),
    _case("rubin_nx91_mean_j66", "rubin", [F1], 91, "postel", "mean", sphere_radius=10.0, jmax=66),
    _case("rubin_nx65_direct_j66", "rubin", [F0, OUT, F2], 65, "postel", jmax=66, direct=True),
    _case("rubin_out_alone", "rubin", [OUT], 17, "postel", "mean"),
    _case("one_mirror_nx17", "one_mirror", [F0, (0.1 * DEG, 0.05 * DEG)], 17),
    _case("one_mirror_nx65_mean", "one_mirror", [(0.1 * DEG, 0.05 * DEG)], 65, "zemax", "mean", sphere_radius=4.0),
    _case("m2_nx17", "m2", [F1, F2], 17),
    _case("m2_nx15_mean", "m2", [F0], 15, "gnomonic", "mean", jmax=2),
    _case("camera_nx65_mean", "camera", [F2], 65, "gnomonic", "mean"),
    _case("m1_figure_nx64", "m1_figure", [F1], 64, "zemax"),
    _case("m1_figure_nx16_four", "m1_figure", FOUR, 16, "postel", "mean", jmax=2),
]
BY_NAME = {c["name"]: c for c in CASES}


def parameters(case):
    """(tel, sphere_radius, eps) as opd.compute resolves them"""
    tel = telescope(case["tel"])
    R = tel.sphere_radius if case["sphere_radius"] is None else case["sphere_radius"]
    eps = tel.eps if tel.eps is not None else tel.pupil_inner / tel.pupil_outer
    return tel, float(R), float(eps)


_REF = {}


def reference(case, mutate=None):
    """tests/opd_ref.py's result for the case: computed once and shared (never modified by a test)"""
    import opd_ref
    key = (case["name"], mutate)
    if key not in _REF:
        tel, R, eps = parameters(case)
        _REF[key] = opd_ref.compute(descriptor(tel), case["fields"], WAVE, case["nx"], tel.pupil_outer, case["projection"], R,
                                    case["reference"], eps, case["jmax"], mutate)
    return _REF[key]
