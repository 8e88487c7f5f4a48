"""Optical path difference (wavefront) maps and their annular Zernike coefficients: the `opd` extra output
(imsim/opd.py, which calls batoid's `wavefront` and `zernike`), traced on the GPU (ims_opd, csrc/ims_opd.h).

Conventions (batoid is not available here to check its grid against; these are the ones this module implements):

* Pupil grid.  A map is nx x nx rays on a square grid in the entrance-pupil plane (z = stop_z) with spacing
  dx = pupil_size / nx, pupil_size = 2 tel.pupil_outer.  Column i and row j sit at x_i = (i - (nx - 1) / 2) dx and
  y_j = (j - (nx - 1) / 2) dx, so an even nx has no sample at the centre; array[j, i] is the ray at (x_i, y_j).  The
  world origin of the header's OffsetWCS is the pupil coordinate of array[nx // 2, nx // 2].
* Incoming plane wave.  The field angle (u, v) becomes a unit propagation direction d through `projection`: postel
  (sin rho (u, v) / rho, rho = hypot(u, v)), gnomonic ((u, v, 1) / norm) or zemax ((tan u, tan v, 1) / norm), with
  the z component negated -- the sign optics.pupil_rays uses: the light travels towards -z and +thx gives +x.  Each
  ray starts at (x, y, stop_z) with optical path n_in (d . r), the phase of the plane wave measured from the plane
  through the origin (without it an off-axis field gets a spurious tilt).
* Trace.  n_medium x geometric length is added per segment, through every surface to the detector, with the asphere
  intersections iterated to f64 resolution (the photon path stops earlier, ims_photon.h surf_hit).  The chief ray
  runs from the stop centre (0, 0, stop_z) and is traced even where it is obscured, as batoid does.
* Reference sphere.  Centred on the reference point -- the chief ray's detector hit (`chief`) or the mean detector
  hit of the unvignetted rays (`mean`) -- with radius sphere_radius, on the upstream side: each ray goes back from its
  detector hit along its direction by s < 0 to the sphere, t = path_det + n_det s.
* OPD.  (t0 - t) 1e9 nm with t in metres; t0 is the chief ray's t (`chief`) or the mean t of the unvignetted rays
  (`mean`).  NaN where a ray was vignetted or lost.
* Zernikes.  Annular Zernikes in Noll order with Mahajan's normalisation (unit mean square over the annulus
  eps R_outer <= r <= R_outer, R_outer = pupil_size / 2), j = 1 .. jmax <= 66, fitted by least squares to the finite
  pixels; AZ_jjj in nm.  The fit is the minimum-norm least-squares solution over the finite pixels (what the reference's
  np.linalg.lstsq on the basis returns): every coefficient is 0 for a map without a finite pixel (a field outside the field
  of view, a lost chief ray), and where fewer pixels are finite than terms are fitted it is the pseudo-inverse's solution.
  It is taken from the device's normal equations (solve_normal): eigenvalues of A^T A below jmax 8192 2^-52 of the largest,
  the bound of the device sums' rounding, count as zero.

A perturbed telescope (optics.apply_perturbations: shifted, rotated or figured surfaces) is traced surface by surface in
each surface's frame (ims_opd_perturbed); the path lengths and the reference sphere are taken in telescope coordinates.

There is no CPU fallback: without the library or a GPU, compute() raises like the engine does.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

from . import _abi, fits_io, optics as opticsmod

PROJECTIONS = ("postel", "gnomonic", "zemax")
REFERENCES = {"chief": _abi.IMS_OPD_REF_CHIEF, "mean": _abi.IMS_OPD_REF_MEAN}
MAX_JMAX = _abi.IMS_OPD_MAX_J
HEADER_KEYS = ("units", "dx", "dy", "thx", "thy", "r_thx", "r_thy", "wavelen", "prjct", "sph_rad", "sph_ref", "eps", "jmax",
               "telescop")


# ---------------- annular Zernike basis ----------------
def noll_to_nm(j):
    """(n, m) of Noll index j >= 1: m > 0 is the cos(m theta) term, m < 0 the sin(|m| theta) term."""
    n, j1 = 0, j - 1
    while j1 > n:
        n += 1
        j1 -= n
    m = (n % 2) + 2 * ((j1 + ((n + 1) % 2)) // 2)
    return n, (m if j % 2 == 0 else -m)


def _radial_table(n_max, eps):
    """{(n, |m|): coefficients of rho^0 .. rho^n} of the annular radial polynomials normalised to unit mean square over the
    annulus (weight 2 rho / (1 - eps^2) on [eps, 1]), positive at rho = 1.  Gram-Schmidt of rho^|m|, rho^(|m|+2), ... in
    exact rational arithmetic (eps^2 is the float's exact value), so no conditioning is lost; the one rounding is the
    final square root of the norm."""
    e2 = Fraction(eps) ** 2
    denom = 1 - e2

    def inner(a, b):                # a, b: {power: Fraction}
        s = Fraction(0)
        for pa, ca in a.items():
            for pb, cb in b.items():
                k = pa + pb + 2
                s += ca * cb * (1 - e2 ** (k // 2)) / k
        return 2 * s / denom

    out = {}
    for m in range(n_max + 1):
        basis = []
        for n in range(m, n_max + 1, 2):
            p = {n: Fraction(1)}
            for q in basis:
                c = inner(p, q) / inner(q, q)
                for k, v in q.items():
                    p[k] = p.get(k, Fraction(0)) - c * v
            basis.append(p)
            norm2 = inner(p, p)
            sign = 1.0 if sum(p.values()) > 0 else -1.0
            coef = np.zeros(n + 1)
            for k, v in p.items():
                coef[k] = sign * float(v) / math.sqrt(float(norm2))
            out[(n, m)] = coef
    return out


def zernike_table(jmax, eps):
    """(poly [jmax, IMS_OPD_NPOW], m [jmax]): the device table of ims_opd_t -- row j - 1 holds the coefficients of rho^0 ..
    rho^10 of Noll term j including its normalisation (sqrt 2 for m != 0), m its signed azimuthal order."""
    jmax = int(jmax)
    if not 1 <= jmax <= MAX_JMAX:
        raise ValueError(f"jmax must be in 1 .. {MAX_JMAX}")
    nm = [noll_to_nm(j) for j in range(1, jmax + 1)]
    radial = _radial_table(max(n for n, _ in nm), float(eps))
    poly = np.zeros((jmax, _abi.IMS_OPD_NPOW))
    ms = np.zeros(jmax, dtype=np.int32)
    for k, (n, m) in enumerate(nm):
        c = radial[(n, abs(m))] * (math.sqrt(2.0) if m != 0 else 1.0)
        poly[k, :len(c)] = c
        ms[k] = m
    return poly, ms


def zernike_basis(jmax, x, y, r_outer, eps):
    """Z_1 .. Z_jmax at pupil points (x, y) [m]: array [jmax, *x.shape] from the same table the device evaluates."""
    poly, ms = zernike_table(jmax, eps)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    rho = np.hypot(x, y) / r_outer
    th = np.arctan2(y, x)
    out = np.empty((len(ms),) + x.shape)
    for k, m in enumerate(ms):
        rad = np.polynomial.polynomial.polyval(rho, poly[k])
        out[k] = rad * (np.cos(m * th) if m > 0 else np.sin(-m * th) if m < 0 else 1.0)
    return out


# ---------------- fields ----------------
def field_direction(thx, thy, projection="postel"):
    """Unit propagation direction of the plane wave of field angle (thx, thy) [rad]; z < 0, +thx gives +x."""
    if projection == "postel":
        rho = math.hypot(thx, thy)
        if rho == 0.0:
            return np.array([0.0, 0.0, -1.0])
        s = math.sin(rho) / rho
        return np.array([s * thx, s * thy, -math.cos(rho)])
    if projection == "gnomonic":
        d = np.array([thx, thy, -1.0])
    elif projection == "zemax":
        d = np.array([math.tan(thx), math.tan(thy), -1.0])
    else:
        raise ValueError(f"unknown projection {projection!r} (one of {', '.join(PROJECTIONS)})")
    return d / np.linalg.norm(d)


def rotate_field(thx, thy, rot_tel_pos):
    """(r_thx, r_thy) = Rot(rot_tel_pos) @ (thx, thy) (imsim/opd.py:108-123)"""
    c, s = math.cos(rot_tel_pos), math.sin(rot_tel_pos)
    return c * thx - s * thy, s * thx + c * thy


def check_params(nx, projection, reference, jmax):
    if not 1 <= int(nx) <= _abi.IMS_OPD_MAX_NX:
        raise ValueError(f"nx must be in 1 .. {_abi.IMS_OPD_MAX_NX}")
    if projection not in PROJECTIONS:
        raise ValueError(f"unknown projection {projection!r} (one of {', '.join(PROJECTIONS)})")
    if reference not in REFERENCES:
        raise ValueError(f"unknown reference {reference!r} (chief or mean)")
    if not 1 <= int(jmax) <= MAX_JMAX:
        raise ValueError(f"jmax must be in 1 .. {MAX_JMAX}")


# ---------------- header ----------------
def make_header(thx, thy, r_thx, r_thy, dx, wavelength, projection, sphere_radius, reference, eps, jmax, telescope_name, zk):
    """The provenance keys of one map (imsim/opd.py:170-195); angles in rad, zk [jmax] in nm"""
    h = {"units": ("nm", "OPD units"),
         "dx": (float(dx), "entrance pupil coord scale (m)"),
         "dy": (float(dx), "entrance pupil coord scale (m)"),
         "thx": (math.degrees(thx), "field angle (deg)"),
         "thy": (math.degrees(thy), "field angle (deg)"),
         "r_thx": (math.degrees(r_thx), "rotated field angle (deg)"),
         "r_thy": (math.degrees(r_thy), "rotated field angle (deg)"),
         "wavelen": (float(wavelength), "(nm)"),
         "prjct": (projection, "field angle map projection"),
         "sph_rad": (float(sphere_radius), "reference sphere radius (m)"),
         "sph_ref": (reference, "reference point"),
         "eps": (float(eps), "Annular Zernike obscuration fraction"),
         "jmax": (int(jmax), "Max index for annular Zernike coefficients"),
         "telescop": (str(telescope_name), None)}
    for j in range(1, int(jmax) + 1):
        h[f"AZ_{j:03d}"] = (float(zk[j - 1]), "(nm)")
    return h


def wcs_cards(nx, dx):
    """GalSim's FITS keys of the map's OffsetWCS (scale dx, origin the image centre (0, 0), world origin the pupil coordinate
    of array[nx // 2, nx // 2]) as galsim.fits.write puts them: bounds shifted to a (1, 1) origin."""
    u0 = (nx // 2 - (nx - 1) / 2.0) * dx
    xmin = -(nx // 2)                                   # image.setCenter(0, 0)
    x0 = float(1 - xmin)                                # FITS pixel of the image origin (0, 0)
    return {"GS_XMIN": (xmin, "GalSim image minimum x coordinate"), "GS_YMIN": (xmin, "GalSim image minimum y coordinate"),
            "GS_WCS": ("OffsetWCS", "GalSim WCS name"), "GS_SCALE": (float(dx), "GalSim image scale"),
            "GS_X0": (x0, "GalSim image origin x"), "GS_Y0": (x0, "GalSim image origin y"),
            "GS_U0": (u0, "GalSim world origin u"), "GS_V0": (u0, "GalSim world origin v"),
            "CTYPE1": ("LINEAR", "name of the world coordinate axis"), "CTYPE2": ("LINEAR", "name of the world coordinate axis"),
            "CRVAL1": (u0, "world coordinate at reference pixel = u0"), "CRVAL2": (u0, "world coordinate at reference pixel = v0"),
            "CRPIX1": (x0, "image coordinate of reference pixel = x0"), "CRPIX2": (x0, "image coordinate of reference pixel = y0"),
            "CD1_1": (float(dx), "CD1_1 = dudx"), "CD1_2": (0.0, "CD1_2 = dudy"),
            "CD2_1": (0.0, "CD2_1 = dvdx"), "CD2_2": (float(dx), "CD2_2 = dvdy")}


def write(file_name, images):
    """images: [(array, header)] of compute(): one f64 image HDU per field, the first one primary (galsim.fits.writeMulti)"""
    hdus = []
    for arr, hdr in images:
        arr = np.asarray(arr, dtype=np.float64)
        h = dict(hdr)
        h.update(wcs_cards(arr.shape[1], float(hdr["dx"][0] if isinstance(hdr["dx"], tuple) else hdr["dx"])))
        hdus.append((h, arr))
    fits_io.write_fits(file_name, hdus)


# ---------------- GPU ----------------
# eigenvalues of A^T A below this fraction of the largest per Zernike term are rounding: an entry of the device's sums is an fma
# chain over a chunk of 4096 pixels followed by up to 4096 chunk partials, 8192 roundings of 2^-52 at the size of the largest
# eigenvalue, and the matrix norm of jmax x jmax such entries is at most jmax times that
NORMAL_RCOND_PER_TERM = 8192 * 2.0 ** -52


def solve_normal(ata, atw):
    """The least-squares coefficients from the normal equations, as the minimum-norm solution (the module docstring's rule):
    all zeros for a map without a finite pixel, the pseudo-inverse's answer where fewer pixels are finite than terms are
    fitted, the plain solution otherwise.  Never raises on a singular system."""
    ata, atw = np.asarray(ata, dtype=np.float64), np.asarray(atw, dtype=np.float64)
    if not np.any(ata):
        return np.zeros(len(atw))
    return np.linalg.lstsq(ata, atw, rcond=len(atw) * NORMAL_RCOND_PER_TERM)[0]


def _run(lib, torch, dev, opt_dev, tel, dirs, nx, dx, wavelength, sphere_radius, reference, eps, jmax):
    """one ims_opd call: (maps [n, nx, nx], zk [n, jmax] or None)"""
    n = len(dirs)
    P = _abi.Opd()
    P.n_fields, P.nx, P.reference, P.jmax = n, nx, REFERENCES[reference], jmax
    P.dx, P.wavelength, P.sphere_radius = dx, wavelength, sphere_radius
    P.r_outer, P.eps = tel.pupil_outer, eps
    keep = []

    def put(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr()

    P.dirs = put(np.asarray(dirs, dtype=np.float64))
    maps = torch.empty((n, nx, nx), dtype=torch.float64, device=dev)
    P.opd = maps.data_ptr()
    scratch = torch.empty(_abi.opd_scratch_bytes(n, nx, jmax), dtype=torch.uint8, device=dev)
    P.scratch = scratch.data_ptr()
    if jmax > 0:
        poly, ms = zernike_table(jmax, eps)
        P.zk_poly, P.zk_m = put(poly), put(ms)
        ata = torch.empty((n, jmax * (jmax + 1) // 2), dtype=torch.float64, device=dev)
        atw = torch.empty((n, jmax), dtype=torch.float64, device=dev)
        P.zk_ata, P.zk_atw = ata.data_ptr(), atw.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    if opt_dev.numel() == C.sizeof(_abi.OpticsPerturbed):
        _abi.check(lib.ims_opd_perturbed(C.byref(P), opt_dev.data_ptr(), stream), "ims_opd_perturbed")
    else:
        _abi.check(lib.ims_opd(C.byref(P), opt_dev.data_ptr(), stream), "ims_opd")
    maps_h = maps.cpu().numpy()
    if jmax == 0:
        return maps_h, None
    ata_h, atw_h = ata.cpu().numpy(), atw.cpu().numpy()
    iu = np.triu_indices(jmax)
    zk = np.empty((n, jmax))
    for f in range(n):
        A = np.zeros((jmax, jmax))
        A[iu] = ata_h[f]
        A = A + np.triu(A, 1).T
        zk[f] = solve_normal(A, atw_h[f])
    return maps_h, zk


def compute(tel, fields, wavelength, nx=255, projection="postel", sphere_radius=None, reference="chief", eps=None, jmax=28,
            rot_tel_pos=0.0, device="cuda:0"):
    """OPD maps of `tel` for the field angles `fields` [(thx, thy) in rad] at `wavelength` [nm]: [(array [nx, nx] in nm,
    header dict)] in the order of `fields`.  The image is traced at the rotated field Rot(rot_tel_pos) (thx, thy); the
    header's Zernikes are fitted at the UNROTATED (thx, thy) -- the reference does exactly this (imsim/opd.py:143-149
    against :186-195), and it is mirrored here."""
    import torch
    nx, jmax = int(nx), int(jmax)
    check_params(nx, projection, reference, jmax)
    sphere_radius = tel.sphere_radius if sphere_radius is None else float(sphere_radius)
    if sphere_radius is None or not sphere_radius > 0.0:
        raise ValueError("opd: the telescope has no reference-sphere radius; give sphere_radius")
    if eps is None:
        eps = tel.eps if tel.eps is not None else tel.pupil_inner / tel.pupil_outer
    eps = float(eps)
    if not 0.0 <= eps < 1.0:
        raise ValueError("opd: eps must be in [0, 1)")
    if not wavelength > 0.0:
        raise ValueError("opd: wavelength must be positive")
    lib = _abi.load()
    if not torch.cuda.is_available():
        raise _abi.ImsimHipError("opd.compute needs a GPU (there is no CPU fallback)")
    dev = torch.device(device)
    # a perturbed telescope is traced as the reference's telescope input holds it: with the camera turned by the rotator
    # (imsim/telescope_loader.py:242-246); for a coaxial one that rotation changes nothing and is left out
    opt = opticsmod.make_optics(tel, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), rot_tel_pos if tel.perturbed else 0.0)
    _abi.check(lib.ims_fill_derived_medium(int(opt.in_medium_kind), opt.in_medium_c), "ims_fill_derived_medium")
    for k in range(opt.n_surfaces):
        _abi.check(lib.ims_fill_derived_medium(int(opt.surf[k].medium_kind), opt.surf[k].medium_c), "ims_fill_derived_medium")
    _abi.check(lib.ims_fill_derived_optics(C.byref(opt)), "ims_fill_derived_optics")
    opt_dev = torch.from_numpy(np.frombuffer(bytes(opt), dtype=np.uint8).copy()).to(dev)
    fields = [(float(a), float(b)) for a, b in fields]
    rot_fields = [rotate_field(a, b, rot_tel_pos) for a, b in fields]
    dx = 2.0 * tel.pupil_outer / nx
    rotated = any(r != f for r, f in zip(rot_fields, fields))
    run = lambda fl, j: _run(lib, torch, dev, opt_dev, tel, [field_direction(a, b, projection) for a, b in fl], nx, dx,
                             float(wavelength), sphere_radius, reference, eps, j)
    if not fields:
        return []
    maps, zk = run(rot_fields, 0 if rotated else jmax)
    if rotated:
        _, zk = run(fields, jmax)
    return [(maps[k], make_header(fields[k][0], fields[k][1], rot_fields[k][0], rot_fields[k][1], dx, wavelength, projection,
                                  sphere_radius, reference, eps, jmax, tel.name, zk[k]))
            for k in range(len(fields))]
