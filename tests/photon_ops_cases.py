"""Planted photon pools for the operator-chain tests (tests/test_photon_ops.py on the oracle, tests/test_photon_ops_ref_gpu.py
on the device): a scene, an operator list and a pool whose nine fields are planted, not shot.

About 20 000 photons per case over 24 object rows with n_phot from {1, 255, 256, 257, 513, 4099} and phot_first / obj_id beyond
32 bits, so that the segment -> object lookup crosses object boundaries and the Philox counter carries."""
import functools
import math
import os

import numpy as np

import photon_ops_ref as ref
from imsim_amd import _abi, camera, configs, diffraction, optics, tables
from imsim_amd.engine import Scene
from imsim_amd._abi import OBJECT_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
N_PHOT = (1, 255, 256, 257, 513, 4099)
OBJ_IDS = (0, 2 ** 31, 2 ** 32 + 5, 2 ** 40 + 7)
PHOT_FIRST = (0, 1000, 2 ** 32 - 100, 2 ** 33 + 3)
SEED = (0x9E3779B9 << 32) | 398414
NX = 4096
N_ROWS = 24
RAD2AS = 180.0 / math.pi * 3600.0
ARCMIN = math.pi / 10800.0
DCR, FOCUS, REFR, RATIO = _abi.IMS_OP_PHOTON_DCR, _abi.IMS_OP_FOCUS_DEPTH, _abi.IMS_OP_REFRACTION, _abi.IMS_OP_BANDPASS_RATIO
R_OPT, R_DIFF, R_DOPT = _abi.IMS_OP_RUBIN_OPTICS, _abi.IMS_OP_RUBIN_DIFFRACTION, _abi.IMS_OP_RUBIN_DIFFRACTION_OPTICS
ATMOSPHERES = {"site": (69.328, 293.15, 1.067), "sea": (101.325, 288.15, 0.0), "cold": (85.0, 258.15, 0.19)}


def rows(n=N_ROWS):
    o = np.zeros(n, dtype=OBJECT_DTYPE)
    i = np.arange(n)
    o["obj_id"] = [OBJ_IDS[k % 4] + 16 * (k // 4) for k in i]
    o["phot_first"] = [PHOT_FIRST[(k // 4 + k) % 4] for k in i]
    o["n_phot"] = [N_PHOT[k % 6] for k in i]
    o["flux_per_photon"] = 1.0
    o["prof_table"], o["sed_table"], o["sed_wave"] = _abi.IMS_PROF_POINT, -1, 620.0
    for k in i:
        a = 0.3 + 0.4 * k
        m = np.array([math.cos(a), -1.3 * math.sin(a), math.sin(a), 0.8 * math.cos(a)]) * 5.0     # non-diagonal
        if k % 2:
            m[2:] = -m[2:]                                                                        # negative determinant
        o["winv"][k] = m
        q = 0.4 + k * math.pi / 2.0 + 0.05 * k                                                    # all four quadrants
        o["dcr_sinp"][k], o["dcr_cosp"][k] = math.sin(q), math.cos(q)
    o["dcr_tanz"] = np.where(i % 5 == 0, 0.0, np.where(i % 5 == 1, math.tan(math.radians(70.0)), 0.2 + 0.05 * i))
    o["stamp_xmin"], o["stamp_xmax"], o["stamp_ymin"], o["stamp_ymax"] = 1, NX, 1, NX
    return o


class Case:
    def __init__(self, name, scene, objects, pool, rubin=False):
        self.name, self.scene, self.objects, self.pool, self.rubin = name, scene, np.ascontiguousarray(objects, dtype=OBJECT_DTYPE), pool, rubin
        n = int(self.objects["n_phot"].sum())
        assert all(len(pool[f]) == n and pool[f].dtype == np.float64 for f in ref.FIELDS) and n <= 25_000

    def blocks(self):
        sc = self.scene
        return dict(seed=sc.seed, optics=sc.optics, ratio_tables=None if sc.ratio_tables is None else np.atleast_2d(sc.ratio_tables),
                    ratio_wl_min=sc.ratio_wl_min, ratio_wl_step=sc.ratio_wl_step)

    def reference(self, mutate=None, loose=True):
        return ref.apply(self.scene.ops, self.blocks(), self.objects, self.pool, mutate=mutate, loose=loose)

    def obj_index(self):
        return np.repeat(np.arange(len(self.objects)), self.objects["n_phot"]).astype(np.int32)


def base_pool(objects, seed):
    """generic planted fields: positions over the CCD, slopes up to the f/1.2 beam's (0.42), the r band, the pupil annulus"""
    rng = np.random.default_rng(seed)
    n = int(objects["n_phot"].sum())
    r = np.sqrt(rng.uniform(2.558 ** 2, 4.18 ** 2, n))
    a = rng.uniform(0.0, 2.0 * np.pi, n)
    return dict(x=rng.uniform(1.0, NX, n), y=rng.uniform(1.0, NX, n), flux=rng.choice([1.0, 0.75, -1.0], n),
                dxdz=rng.uniform(-0.42, 0.42, n), dydz=rng.uniform(-0.42, 0.42, n), wavelength=rng.uniform(540.0, 700.0, n),
                pupil_u=r * np.cos(a), pupil_v=r * np.sin(a), time=rng.uniform(0.0, 30.0, n))


def _scene(ops, **kw):
    return Scene(nx=NX, ny=NX, seed=SEED, psf=[], ops=ops, **kw)


def dcr_case(atm):
    o = rows()
    pool = base_pool(o, 1)
    special = np.array([300.0, 1100.0, 620.0, 540.0, 700.0, 552.0, 691.0])          # ends, the base itself, the r-band edges
    pool["wavelength"][::3] = special[np.arange(len(pool["wavelength"][::3])) % len(special)]
    return Case(f"dcr_{atm}", _scene([(DCR, 0, [620.0, *ATMOSPHERES[atm], RAD2AS])]), o, pool)


def focus_case(name, depth):
    o = rows()
    return Case(f"focus_{name}", _scene([(FOCUS, 0, [depth])]), o, base_pool(o, 2))


def refraction_case(name, ratio):
    o = rows()
    pool = base_pool(o, 3)
    mag = np.array([0.1, -0.1, 0.3, -0.45, 0.6, -0.6, 0.0])
    pool["dxdz"][::2] = mag[np.arange(len(pool["dxdz"][::2])) % 7]
    pool["dydz"][::2] = mag[(np.arange(len(pool["dydz"][::2])) // 7) % 7]
    pool["dxdz"][1::50], pool["dydz"][1::50] = 0.0, 0.0                               # zero slopes stay exactly zero
    return Case(f"refraction_{name}", _scene([(FOCUS, 0, [0.0]), (REFR, 0, [ratio])]), o, pool)


def ratio_tables():
    wl, thr = tables.synthetic_r_band()
    bp = tables.Bandpass(wl, thr)
    t0, wl_min, wl_step = (bp * 0.8).ratio_table(bp)
    t1 = 0.5 + 0.4 * np.sin(np.arange(len(t0)) * 0.37) ** 2                              # distinct end values
    t1[0], t1[-1] = 0.25, 1.75
    return np.stack([t0, t1]), float(wl_min), float(wl_step)


def ratio_case(table, faint_rows=False):
    o = rows()
    if faint_rows:
        o["flags"][::4] = _abi.IMS_OBJ_FAINT
    t, wl_min, wl_step = ratio_tables()
    pool = base_pool(o, 4)
    npts = t.shape[1]
    knots = wl_min + wl_step * np.arange(npts)
    sel = np.concatenate([knots[[0, -1, 1, npts // 2, npts - 2]], [wl_min - 40.0, wl_min - 1e-9, knots[-1] + 1e-9, knots[-1] + 55.0,
                                                                      knots[3] + 0.5 * wl_step]])
    pool["wavelength"][::2] = sel[np.arange(len(pool["wavelength"][::2])) % len(sel)]
    sc = _scene([(RATIO, table, [])], ratio_tables=t, ratio_wl_min=wl_min, ratio_wl_step=wl_step)
    return Case(f"ratio_t{table}{'_faint' if faint_rows else ''}", sc, o, pool)


# ---------------- Rubin operators ----------------
def _everything(tel):
    """the shifted, tilted and figured surfaces of tests/test_perturbed_gpu.py"""
    rng = np.random.default_rng(5)
    coef = [0.0] * 4 + list(0.3e-6 * rng.standard_normal(19))
    return optics.apply_perturbations(tel, [
        {"M2": {"shift": [100e-6, 0.0, 0.0], "rotX": ARCMIN}},
        {"LSSTCamera": {"rotY": 0.5 * ARCMIN, "shift": [20e-6, -30e-6, 15e-6]}},
        {"M1": {"Zernike": {"coef": coef}}},
        {"L1": {"shift": [40e-6, 25e-6, 0.0]}}])


@functools.lru_cache(maxsize=None)
def _wcs(offaxis):
    v = configs.VISIT
    tel = optics.rubin_like_telescope(v["band"])
    fp = camera.fp_to_pix("R01_S00" if offaxis else "R22_S11", NX, NX)
    rot = math.radians(v["rottelpos"])
    img, i2f, th = optics.build_wcs_pair(tel, fp, math.radians(v["ra"]), math.radians(v["dec"]), rot_sky=math.radians(v["rotskypos"]),
                                         rot_tel_pos=rot, nx=NX, ny=NX)
    return tel, fp, rot, img, i2f, th


@functools.lru_cache(maxsize=None)
def optics_block(offaxis=False, zenith=False, perturbed=False, aniso=False):
    tel, fp, rot, img, i2f, th = _wcs(offaxis)
    if aniso:
        # no science CCD has them, but fp_to_pix is a free affine map: pixels 10 x 8 um, so that slope_jac is not symmetric.
        # (The WCS pair stays that of the square pixels; the operators only need it to be a TAN-SIP.)
        fp = (fp[0], fp[1], fp[2], fp[3], 125.0, fp[5])
    if offaxis:
        assert math.degrees(math.hypot(*th)) > 1.5                                      # field radius of the placement
    o = optics.make_optics(_everything(tel) if perturbed else tel, fp, rot)
    assert isinstance(o, _abi.OpticsPerturbed) == perturbed
    o.img_wcs, o.icrf_to_field = img, i2f
    g = np.load(os.path.join(HERE, "golden", "diffraction_golden.npz"))
    lat, az, alt = g["zenith_lat_az_alt" if zenith else "visit_lat_az_alt"]
    diffraction.fill_optics(o, float(lat), float(az), float(alt))
    return o


def rubin_pool(objects, seed):
    rng = np.random.default_rng(seed)
    pool = base_pool(objects, seed)
    n = len(pool["x"])
    i = np.arange(n)
    # the CCD's four corners and centre, a few pixels of scatter
    cx = np.array([1.0, NX, 1.0, NX, (NX + 1) / 2.0])[i % 5]
    cy = np.array([1.0, 1.0, NX, NX, (NX + 1) / 2.0])[(i % 5)]
    pool["x"], pool["y"] = cx + rng.uniform(-3.0, 3.0, n), cy + rng.uniform(-3.0, 3.0, n)
    pool["dxdz"][:], pool["dydz"][:] = 0.0, 0.0
    pool["flux"][:] = rng.choice([1.0, 0.75], n)
    pool["time"] = np.where(i % 3 == 0, 0.0, np.where(i % 3 == 1, 30.0, pool["time"]))
    # pupil: uniform over the annulus, a ring a millimetre inside each edge, points outside it (vignetted by M1), rays that
    # miss M2's conic altogether
    ring = np.where(i % 2 == 0, 2.558 + 1e-3, 4.18 - 1e-3)
    r = np.hypot(pool["pupil_u"], pool["pupil_v"])
    r = np.where(i % 16 == 7, ring, r)
    r = np.where(i % 64 == 9, np.where(i % 128 == 9, 2.3, 4.35), r)
    r = np.where(i % 4096 == 11, 11.0 + (i % 7), r)
    a = np.arctan2(pool["pupil_v"], pool["pupil_u"])
    pool["pupil_u"], pool["pupil_v"] = r * np.cos(a), r * np.sin(a)
    return pool


def plant_near_vanes(pool, block):
    """one pupil point in 32 at 15 .. 30 um from the edge of a spider vane, 2.8 .. 3.5 m along it: there 1 / (2 k d) ~ 3e-3, where
    atan(x) and x part by x^3 / 3 ~ 1e-8 rad, a hundred times the kick's bound; far from every other element (no argmin tie).
    For a case without field rotation, where the distance is taken at the pupil point itself."""
    i = np.flatnonzero(np.arange(len(pool["x"])) % 32 == 5)
    j = np.arange(len(i))
    L = np.array([list(block.lines[k]) for k in range(block.n_lines)])[j % block.n_lines]
    along = np.where(j % 2 == 0, 1.0, -1.0) * (2.8 + 0.1 * (j % 8))
    across = L[:, 2] + np.where((j // 2) % 2 == 0, 1.0, -1.0) * (L[:, 3] + 1e-6 * (15.0 + 5.0 * (j % 4)))
    pool["pupil_u"][i] = L[:, 0] * across - L[:, 1] * along
    pool["pupil_v"][i] = L[:, 1] * across + L[:, 0] * along
    r = np.hypot(pool["pupil_u"][i], pool["pupil_v"][i])
    assert np.all((r > 2.558 + 0.1) & (r < 4.18 - 0.1))


def rubin_case(name, kind, op_index, disable_rot=0.0, offaxis=False, zenith=False, perturbed=False, aniso=False, near_vanes=False, seed=7):
    o = rows()
    ops = [(FOCUS, 0, [0.0])] * op_index + [(kind, 0, [1.0, disable_rot])]
    block = optics_block(offaxis, zenith, perturbed, aniso)
    sc = _scene(ops, optics=block)
    pool = rubin_pool(o, seed + op_index)
    if near_vanes:
        assert disable_rot
        plant_near_vanes(pool, block)
    return Case(name + ("_pert" if perturbed else ""), sc, o, pool, rubin=True)


RUBIN = [("optics_onaxis", R_OPT, 0, {}), ("optics_offaxis", R_OPT, 1, dict(offaxis=True)), ("optics_aniso", R_OPT, 0, dict(aniso=True)),
         ("diff0_rot_visit", R_DIFF, 0, {}), ("diff1_norot_zenith", R_DIFF, 1, dict(disable_rot=1.0, zenith=True, near_vanes=True)),
         ("diff2_rot_zenith", R_DIFF, 2, dict(zenith=True)), ("diff3_rot_offaxis", R_DIFF, 3, dict(offaxis=True)),
         ("dopt0_rot_visit", R_DOPT, 0, {}), ("dopt1_rot_zenith_offaxis", R_DOPT, 1, dict(zenith=True, offaxis=True)),
         ("dopt2_rot_visit", R_DOPT, 2, {}), ("dopt3_norot_visit", R_DOPT, 3, dict(disable_rot=1.0))]


def chain_case(name, perturbed=False, faint=False):
    """the default chain of six (config/imsim-config.yaml:281-320) with a BandpassRatio behind it"""
    o = rows()
    if faint:
        o["flags"] = _abi.IMS_OBJ_FAINT
    t, wl_min, wl_step = ratio_tables()
    ops = configs.c3_ops(30.0, 620.0) + [(RATIO, 1, [])]
    sc = _scene(ops, optics=optics_block(False, False, perturbed), ratio_tables=t, ratio_wl_min=wl_min, ratio_wl_step=wl_step)
    return Case(name, sc, o, rubin_pool(o, 21), rubin=not faint)


@functools.lru_cache(maxsize=None)
def plain_cases():
    return ([dcr_case(a) for a in ATMOSPHERES] + [focus_case("zero", 0.0), focus_case("pos", 2.75), focus_case("neg", -13.5)]
            + [refraction_case("3.9", 3.9), refraction_case("1", 1.0)] + [ratio_case(0), ratio_case(1, faint_rows=True)]
            + [chain_case("chain_faint", faint=True)])


@functools.lru_cache(maxsize=None)
def rubin_cases(perturbed=False):
    return [rubin_case(name, kind, k, perturbed=perturbed, **kw) for name, kind, k, kw in RUBIN] + [
        chain_case("chain_default_pert" if perturbed else "chain_default", perturbed=perturbed)]


def all_cases():
    return plain_cases() + rubin_cases(False) + rubin_cases(True)


def by_name(name):
    return next(c for c in all_cases() if c.name == name)
