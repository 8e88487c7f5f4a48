"""Hand-made scenes and object tables for the photon-source tests (tests/test_photon_source.py on the oracle,
tests/test_photon_source_gpu.py on the device), and the reference's view of each (photon_source_ref.Source).

Images are 64 x 64; every object takes n_phot from {1, 255, 256, 257, 513, 4099} (segment guard, partial last segment) and the
tables hold several objects, so that the segment -> object lookup crosses object boundaries inside a launch."""
import copy
import functools
import math

import numpy as np

import photon_source_ref as ref
from imsim_amd import _abi, atm_psf, configs
from imsim_amd.engine import QUINTIC_NEGATIVE, Scene, image_profile_cdf, interpolant_cdf
from imsim_amd._abi import OBJECT_DTYPE

G, RAD, SCR, DG = _abi.IMS_PSF_GAUSSIAN, _abi.IMS_PSF_RADIAL, _abi.IMS_PSF_SCREENS, _abi.IMS_PSF_DOUBLE_GAUSSIAN
N_PHOT = (1, 255, 256, 257, 513, 4099)
OBJ_IDS = (0, 2 ** 31, 2 ** 32 + 5, 2 ** 40 + 7)
PHOT_FIRST = (0, 1000, 2 ** 32 - 100, 2 ** 33 + 3)          # 2^32 - 100: the block of 256+ photons crosses the 32-bit carry
SEED = (0x9E3779B9 << 32) | 398414                          # a nonzero high half
NX = 64
ARCSEC = atm_psf.ARCSEC


def rows(n, first=None, ids=None, n_phot=None):
    """n object rows: point sources with a sheared jac and a rotated, non-diagonal winv"""
    o = np.zeros(n, dtype=OBJECT_DTYPE)
    i = np.arange(n)
    o["obj_id"] = [OBJ_IDS[k % 4] + 16 * (k // 4) for k in i] if ids is None else ids
    o["phot_first"] = [PHOT_FIRST[(k // 4 + k) % 4] for k in i] if first is None else first
    o["n_phot"] = [N_PHOT[k % 6] for k in i] if n_phot is None else n_phot
    o["x0"], o["y0"] = 8.25 + (37 * i) % 48, 9.5 + (23 * i) % 47
    o["flux_per_photon"] = 1.0
    o["prof_table"], o["sed_table"], o["sed_wave"] = _abi.IMS_PROF_POINT, -1, 600.0 + 7.0 * i
    o["prof_scale"] = 0.4 + 0.05 * (i % 5)
    for k in i:
        a = 0.3 + 0.4 * k
        o["jac"][k] = (1.0, 0.35 + 0.01 * k, -0.1, 0.8)                                       # sheared
        o["winv"][k] = np.array([math.cos(a), -math.sin(a), math.sin(a), math.cos(a)]) * 5.0  # rotated, 0.2 arcsec pixels
    o["stamp_xmin"], o["stamp_xmax"], o["stamp_ymin"], o["stamp_ymax"] = 1, NX, 1, NX
    return o


def sed_tables(n_pts):
    """two inverse-CDF wavelength tables on n_pts points; the second has a flat stretch"""
    u = np.linspace(0.0, 1.0, n_pts)
    a = 550.0 + 140.0 * u ** 1.5
    b = 540.0 + 160.0 * np.clip(1.6 * u - 0.3, 0.0, 1.0)     # flat below u = 0.1875 and above 0.8125
    return np.stack([a, b])


def toy_radial(n_bins):
    """(r2, cdf) [n_tables][n_bins + 1] of the toy tables of one length, r2 ascending from 0"""
    if n_bins == 1:
        return np.array([[0.0, 2.25]]), np.array([[0.0, 1.0]])
    if n_bins == 2:
        return np.array([[0.0, 1.0, 9.0]]), np.array([[0.0, 0.999, 1.0]])
    if n_bins == 7:
        # two repeated values: bins of no width (the arm that returns the lower knot), with a jump in r2 across them
        cdf = np.array([[0.0, 0.125, 0.125, 0.4, 0.7, 0.7, 0.90625, 1.0],
                        [0.0, 0.0, 0.3, 0.3, 0.5, 0.8, 1.0, 1.0]])
        r2 = np.array([[0.0, 0.25, 1.0, 1.5, 2.0, 4.0, 4.5, 6.25],
                       [0.0, 0.5, 0.75, 2.0, 2.5, 3.0, 3.5, 8.0]])
        return r2, cdf
    assert n_bins == 4096
    # geometric: cdf[i] = 2^-30 * ratio^i up to 1, so that > 1000 bins lie inside the first of the 512 guide cells (below 1 / 512)
    # and the last bin [cdf[4095], 1] holds several hundred guide cells
    i = np.arange(n_bins)
    cdf = np.concatenate([[0.0], 2.0 ** (-30.0 + 29.0 * i[:-1] / (n_bins - 2)), [1.0]])
    cdf[n_bins - 1] = 0.5
    r2 = np.concatenate([[0.0], np.geomspace(1.0e-6, 16.0, n_bins)])
    assert np.all(np.diff(cdf) > 0) and (cdf < 1.0 / 512).sum() > 1000
    return r2[None, :], cdf[None, :]


class Case:
    """scene, objects, the environment switches of the renderer, and whether the pre-pass is asked for"""

    def __init__(self, name, scene, objects, env=None, prepass=None):
        self.name, self.scene, self.objects = name, scene, np.ascontiguousarray(objects, dtype=OBJECT_DTYPE)
        self.env = dict(env or {})
        self.prepass = prepass                          # None: no pre-pass; True / False: asked for, and expected to be taken or not
        assert self.objects["n_phot"].sum() <= 200_000

    def source(self):
        sc = self.scene
        cdfs = [image_profile_cdf(im) for im in (sc.image_profiles or [])]
        interp = None
        if sc.image_profiles and sc.image_interpolant == "quintic":
            kx, kcdf, norm = interpolant_cdf()
            interp = (kx, kcdf, norm, QUINTIC_NEGATIVE)
        return ref.Source(sc, cdfs, interp)


def _scene(psf, r2=None, cdf=None, sed=None, **kw):
    return Scene(nx=NX, ny=NX, seed=SEED, psf=list(psf), ops=[], radial_r2=r2, radial_cdf=cdf, sed_tables=sed, **kw)


GAUSS = [(G, 0, s, 0.0, 1.0) for s in (0.11, 0.23, 0.37, 0.53, 0.71)]           # distinct widths: a word swap shows


def addressing_case(n_gauss):
    o = rows(16)                                          # every obj_id with every phot_first
    o["phot_first"] = [PHOT_FIRST[k // 4] for k in range(16)]
    o["obj_id"] = [OBJ_IDS[k % 4] for k in range(16)]
    o["n_phot"] = [N_PHOT[(k + k // 4) % 6] for k in range(16)]
    o["sed_table"] = [(-1, 0, 1)[k % 3] for k in range(16)]
    o["prof_table"][::3] = _abi.IMS_PROF_BOX
    o["prof_aux"] = 0.15
    return Case(f"gauss{n_gauss}", _scene(GAUSS[:n_gauss], sed=sed_tables(2049)), o)


def wavelength_case(n_pts):
    o = rows(9)
    o["sed_table"] = [(0, 1, -1)[k % 3] for k in range(9)]
    return Case(f"wavelength{n_pts}", _scene([(G, 0, 0.3, -0.2, 620.0)], sed=sed_tables(n_pts)), o)


def production_case():
    """Sersic 1, Sersic 4 and Kolmogorov as profiles; Kolmogorov (chromatic, -0.3) plus a Gaussian (+1) as the PSF"""
    r2, cdf = configs.standard_tables()
    o = rows(9)
    o["prof_table"] = [k % 3 for k in range(9)]
    o["sed_table"] = [(0, -1)[k % 2] for k in range(9)]
    return Case("production", _scene([(RAD, 2, 0.7, -0.3, 620.0), (G, 0, 0.2, 1.0, 650.0)], r2, cdf, sed_tables(3)), o)


def toy_case(n_bins):
    r2, cdf = toy_radial(n_bins)
    nt = len(r2)
    o = rows(8)
    o["prof_table"] = [k % nt for k in range(8)]
    o["prof_table"][7] = _abi.IMS_PROF_POINT
    o["sed_table"] = [(1, -1, 0)[k % 3] for k in range(8)]
    psf = [(RAD, nt - 1, 0.6, -0.2, 600.0), (G, 0, 0.15, 0.0, 1.0), (RAD, 0, 0.35, 0.0, 1.0)]
    return Case(f"toy{n_bins}", _scene(psf, r2, cdf, sed_tables(2)), o)


def profiles_case(interpolant):
    """box, knots of 1, 2 and 37, FITS stamps of 1 x 1, 3 x 5 and 8 x 8 with empty pixels; the double Gaussian with p2 = 0, 0.3, 1"""
    rng = np.random.default_rng(11)
    im35 = rng.uniform(0.1, 1.0, size=(5, 3))
    im35[0, 0] = im35[2, 1] = im35[4, 2] = 0.0
    im88 = rng.uniform(0.0, 1.0, size=(8, 8)) ** 2
    im88[3, :] = 0.0
    im88[:, 5] = 0.0
    o = rows(10)
    kinds = [_abi.IMS_PROF_BOX, _abi.IMS_PROF_KNOTS, _abi.IMS_PROF_KNOTS, _abi.IMS_PROF_KNOTS, _abi.IMS_PROF_IMAGE,
             _abi.IMS_PROF_IMAGE, _abi.IMS_PROF_IMAGE, _abi.IMS_PROF_BOX, _abi.IMS_PROF_IMAGE, _abi.IMS_PROF_KNOTS]
    aux = [0.13, 1, 2, 37, 0, 1, 2, 3.7, 2, 37]           # box width != length; knot count; image index
    o["prof_table"], o["prof_aux"] = kinds, aux
    o["prof_scale"][7] = 6.1
    o["sed_table"] = [(0, 1, -1)[k % 3] for k in range(10)]
    psf = [(DG, 0, 0.21, 0.0, 1.0, 0.47, 0.0), (DG, 0, 0.12, -0.3, 620.0, 0.33, 0.3), (DG, 0, 0.28, 0.0, 1.0, 0.09, 1.0)]
    sc = _scene(psf, sed=sed_tables(3), image_profiles=[np.array([[2.5]]), im35, im88], image_interpolant=interpolant)
    return Case(f"profiles_{interpolant}", sc, o)


@functools.lru_cache(maxsize=None)
def _atmosphere(width, layers, hand_made):
    atm = atm_psf.AtmosphericPSF(1.2, 0.75, "r", seed=31 + width, exptime=30.0, screen_size=width * 0.1, screen_scale=0.1, no2k=True)
    pick = list(range(6)) if layers == 6 else [0, 3, 5]                       # the 15.46-km layer stays
    atm.altitudes = np.array([0.2, 2.58, 5.16, 7.73, 12.89, 15.46])[pick]
    atm.speeds = np.array([3.0, 20.0, 7.5, 11.0, 16.0, 20.0])[pick]           # 20 m/s x 30 s = 600 m
    atm.directions = np.array([0.3, 2.2, 4.0, 5.5, 1.1, 3.6])[pick]
    if hand_made:
        l, r, c = np.meshgrid(np.arange(layers), np.arange(width), np.arange(width), indexing="ij")
        atm.screens = (1000.0 * l + 10.0 * r + 0.01 * c).astype(np.float32)   # a jump at the seam: a wrong wrap is a gross error
    else:
        atm.screens = np.ascontiguousarray(atm.screens[pick])
    return atm


def screen_case(width, layers, hand_made=False, quads="1", prepass=None, comp=0, first=None, n_phot=None, tag=""):
    """screens of `width` samples at 0.1 m: 64 / 128 wrap by a mask, 96 / 100 by wrap_index; field angles of both signs up to
    +- 0.031 (15.46 km x 0.031 = 479 m: the 10-m screen wraps about a hundred times in both directions)"""
    atm = copy.copy(_atmosphere(width, layers, hand_made))           # (a device copy of the screens is cached on the object)
    n = 8 if first is None else len(first)
    if first is None and prepass:
        first = [0, 1000, 2 ** 31 - 100, 2 ** 32 - 5000, 2 ** 31 + 3, 7, 2 ** 32 - 4100, 12345][:n]      # each with its n_phot fits 32 bits
    o = rows(n, first=first, n_phot=n_phot)
    tan = np.array([0.031, -0.031, 0.0007, -0.0123, 0.0201, -0.0298, 0.0, 0.0155])
    o["atm_tan_x"], o["atm_tan_y"] = tan[np.arange(n) % 8], tan[(np.arange(n) + 3) % 8] * np.where(np.arange(n) % 2, 1.0, -1.0)
    o["sed_table"] = [(0, -1, 1)[k % 3] for k in range(n)]
    screens = (SCR, 0, 1.0e-9 * ARCSEC, -0.3, atm.wlen_eff)
    psf = [screens, (G, 0, 0.3 / 2.3548200450309493, 0.0, 1.0)] if comp == 0 else [GAUSS[1], screens, GAUSS[0]]
    sc = _scene(psf, sed=sed_tables(3), atm=atm)
    env = {"IMS_SCREEN_QUADS": quads, "IMS_SCREEN_PREPASS": "1" if prepass is not None else "0"}
    name = f"screens{width}x{layers}{'h' if hand_made else ''}_q{quads}{'_pre' if prepass is not None else ''}{'_c1' if comp else ''}{tag}"
    return Case(name, sc, o, env, prepass)


def limit_cases():
    """the pre-pass packs phot_first + j into 32 bits: phot_first + n_phot = 2^32 - 1 still fits, 2^32 does not"""
    n_phot = [513, 257, 4099]
    fits = [2 ** 32 - 1 - n for n in n_phot]
    over = [1000, 2 ** 32 - 257, 0]
    return [screen_case(96, 3, quads="0", prepass=True, first=fits, n_phot=n_phot, tag="_fits"),
            screen_case(96, 3, quads="0", prepass=False, first=over, n_phot=n_phot, tag="_over")]


def source_cases():
    """the cases without screens"""
    return ([addressing_case(k) for k in (1, 2, 3, 4)] + [wavelength_case(n) for n in (2, 3, 2049)] + [production_case()]
            + [toy_case(n) for n in (1, 2, 7, 4096)] + [profiles_case("nearest"), profiles_case("quintic")])


def screen_cases():
    out = []
    for width in (64, 128, 96, 100):
        out += [screen_case(width, 6, quads="1"), screen_case(width, 3, quads="0"),
                screen_case(width, 3, quads="0", prepass=True, comp=width in (128, 100))]
    out += [screen_case(64, 6, quads="0"), screen_case(96, 3, quads="1", comp=1),
            screen_case(100, 3, hand_made=True, quads="1"), screen_case(100, 3, hand_made=True, quads="0"),
            screen_case(64, 6, hand_made=True, quads="1"), screen_case(128, 6, hand_made=True, quads="0", prepass=True),
            screen_case(100, 3, hand_made=True, quads="0", prepass=True, comp=1), screen_case(64, 6, quads="0", prepass=True)]
    return out + limit_cases()


def all_cases():
    return source_cases() + screen_cases()
