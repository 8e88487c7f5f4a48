"""Telescope description for the sequential ray-trace kernel (host side).

imSim traces photons with batoid (`telescope.trace(ray_vec)`, imsim/photon_ops.py:109-123) through
a telescope loaded from batoid's YAML files (imsim/telescope_loader.py:121-252).  Here the
telescope is a flat list of coaxial surfaces (`Surface`) that the HIP kernel walks; it can be read
from a batoid-format YAML (`load_batoid_yaml`, the subset of the format the Rubin files use:
coaxial CompoundOptic / Lens / Mirror / RefractiveInterface / Baffle / Detector, Plane / Sphere /
Paraboloid / Quadric / Asphere, annular/circular obscurations, constant / Sellmeier / Air media).

batoid's own `LSST_r.yaml` is not part of the reference tree (it ships with batoid), so
`rubin_like_telescope()` provides a clearly-labelled APPROXIMATE Rubin prescription (public LSST
optical design values, refocused numerically) so the benchmark configs have a realistic surface
list to trace.  Users with batoid's files point `load_batoid_yaml` at them.
"""
import dataclasses
import math
from typing import List, Optional

import numpy as np

from . import _abi, wcs as wcsmod

SILICA = (_abi.IMS_MEDIUM_SELLMEIER,
          (0.6961663, 0.4079426, 0.8974794, 0.00467914825849, 0.013512063073959999, 97.93400253792099))
VACUUM = (_abi.IMS_MEDIUM_CONST, (1.0, 0, 0, 0, 0, 0))
AIR = (_abi.IMS_MEDIUM_AIR, (69.328, 293.15, 1.067, 0, 0, 0))   # batoid.Air defaults [kPa, K, kPa]


@dataclasses.dataclass
class Surface:
    kind: int
    z0: float
    R: float = 0.0
    conic: float = 0.0
    asph: tuple = ()
    obsc_kind: int = _abi.IMS_OBSC_NONE
    obsc_inner: float = 0.0
    obsc_outer: float = 0.0
    medium: tuple = VACUUM          # medium after the surface (refractive only)
    name: str = ""
    # item path of the surface in the optic hierarchy, dotted ("LSSTCamera.L1.L1_entrance"); "" = the name alone
    path: str = ""
    # rigid frame (perturbed telescopes): vertex origin (x, y, z) and row-major rotation R (telescope = origin + R local) in
    # telescope coordinates.  None, None: coaxial at (0, 0, z0), the frame of every unperturbed surface.  A moved surface keeps
    # z0 == origin[2].
    origin: Optional[tuple] = None
    rot: Optional[tuple] = None
    # Zernike figures added to the sag (batoid's Sum([surface, Zernike, ...])), in the local x, y
    figure: tuple = ()
    # the optic's R_outer / R_inner (batoid Interface attributes); None: from the obscuration
    r_outer: Optional[float] = None
    r_inner: Optional[float] = None

    @property
    def item_path(self):
        return self.path or self.name

    @property
    def coaxial(self):
        return self.origin is None and self.rot is None and not self.figure

    def frame(self):
        """(origin [3], R [3, 3]) in telescope coordinates"""
        o = np.array(self.origin if self.origin is not None else (0.0, 0.0, self.z0), dtype=np.float64)
        R = np.array(self.rot if self.rot is not None else np.eye(3).ravel(), dtype=np.float64).reshape(3, 3)
        return o, R

    def radii(self):
        """(R_outer, R_inner) of the optic, as batoid's withPerturbedSurface defaults take them"""
        if self.r_outer is not None:
            return float(self.r_outer), float(self.r_inner or 0.0)
        if self.obsc_kind in (_abi.IMS_OBSC_CLEAR_ANNULUS, _abi.IMS_OBSC_OBSC_ANNULUS):
            return float(self.obsc_outer), float(self.obsc_inner)
        if self.obsc_kind != _abi.IMS_OBSC_NONE:
            return float(self.obsc_outer), 0.0
        raise ValueError(f"optic {self.item_path}: no R_outer / R_inner known; give both with the Zernike perturbation")


@dataclasses.dataclass(frozen=True)
class Figure:
    """batoid.Zernike(coef, R_outer, R_inner): sum_j coef[j] Z_j(x, y) with annular Zernikes in Noll order (coef[0] unused)
    on the annulus R_inner <= r <= R_outer, normalised to unit mean square over it (opd.py's basis)."""
    coef: tuple
    r_outer: float
    r_inner: float

    def cartesian(self):
        """C [d + 1, d + 1]: the figure as sum_{p, q} C[p, q] u^p v^q with u = x / r_outer, v = y / r_outer"""
        return zernike_cartesian(self.coef, self.r_inner / self.r_outer)

    def __call__(self, x, y):
        """value and gradient (f, df/dx, df/dy) at local x, y [m], by Horner's rule on the Cartesian form"""
        return poly2d_eval(self.cartesian(), np.asarray(x, dtype=np.float64) / self.r_outer,
                           np.asarray(y, dtype=np.float64) / self.r_outer, 1.0 / self.r_outer)


def _binom(n, k):
    return math.comb(n, k)


def zernike_cartesian(coef, eps):
    """Cartesian coefficients C[p, q] (u^p v^q, u = x / R_outer) of sum_j coef[j] Z_j with the annular Zernikes of opd.py
    (Noll order, coef[0] unused).  rho^k cos(m theta) = (u^2 + v^2)^((k - m) / 2) Re (u + i v)^m, sin with Im: the integer
    coefficients of those products are exact, the radial coefficients the one rounding."""
    from . import opd as opdmod
    coef = [float(c) for c in coef]
    jmax = len(coef) - 1
    while jmax > 0 and coef[jmax] == 0.0:
        jmax -= 1
    if jmax < 1:
        return np.zeros((1, 1))
    if jmax > opdmod.MAX_JMAX:
        raise ValueError(f"Zernike figure: Noll index up to {opdmod.MAX_JMAX} (radial order {_abi.IMS_FIG_MAX_DEG})")
    poly, ms = opdmod.zernike_table(jmax, eps)
    deg = max(opdmod.noll_to_nm(j)[0] for j in range(1, jmax + 1) if coef[j] != 0.0)
    C = np.zeros((deg + 1, deg + 1))
    for j in range(1, jmax + 1):
        if coef[j] == 0.0:
            continue
        m = int(ms[j - 1])
        am = abs(m)
        for k in range(am, len(poly[j - 1])):
            a = poly[j - 1][k]
            if a == 0.0 or (k - am) % 2:
                continue
            s = (k - am) // 2
            # Re / Im (u + i v)^|m| = sum_l C(|m|, l) u^(|m| - l) (i v)^l: even l real, odd l imaginary
            for l in range(am + 1):
                if (m >= 0) == (l % 2 == 1):
                    continue
                sign = (-1) ** (l // 2)
                for b in range(s + 1):          # (u^2 + v^2)^s = sum_b C(s, b) u^(2b) v^(2(s - b))
                    C[am - l + 2 * b, l + 2 * (s - b)] += coef[j] * a * sign * _binom(am, l) * _binom(s, b)
    return C


def poly2d_eval(C, u, v, scale=1.0):
    """sum C[p, q] u^p v^q and its derivatives times `scale` (d/dx = scale d/du): Horner in v inside Horner in u"""
    P = np.zeros_like(u)
    Pu = np.zeros_like(u)
    Pv = np.zeros_like(u)
    d = C.shape[0] - 1
    for p in range(d, -1, -1):
        a = np.zeros_like(u)
        av = np.zeros_like(u)
        for q in range(d - p, -1, -1):
            av = av * v + a
            a = a * v + C[p, q]
        Pu = Pu * u + P
        P = P * u + a
        Pv = Pv * u + av
    return P, Pu * scale, Pv * scale


def surface_figure_cartesian(S):
    """(inv_r, C) of all figures of S summed on the first one's R_outer; None without a figure"""
    if not S.figure:
        return None
    r0 = S.figure[0].r_outer
    d = 0
    parts = []
    for f in S.figure:
        C = f.cartesian()
        k = r0 / f.r_outer
        scale = np.array([[k ** (p + q) for q in range(C.shape[1])] for p in range(C.shape[0])])
        parts.append(C * scale)
        d = max(d, C.shape[0] - 1)
    out = np.zeros((d + 1, d + 1))
    for C in parts:
        out[:C.shape[0], :C.shape[1]] += C
    return 1.0 / r0, out


def rot_x(th):
    c, s = math.cos(th), math.sin(th)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def rot_y(th):
    c, s = math.cos(th), math.sin(th)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def rot_z(th):
    c, s = math.cos(th), math.sin(th)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


@dataclasses.dataclass
class Telescope:
    surfaces: List[Surface]
    stop_z: float = 0.4393899
    in_medium: tuple = VACUUM
    pupil_outer: float = 4.18
    pupil_inner: float = 2.558
    name: str = "telescope"
    # reference-sphere radius [m] of the opd extra output (batoid's sphereRadius); None: none known, opd.compute needs one
    sphere_radius: Optional[float] = None
    # annular-Zernike obscuration of the opd extra output (batoid's pupilObscuration); None: pupil_inner / pupil_outer
    eps: Optional[float] = None
    # the compound optics above the surfaces: dotted item path -> (origin (x, y, z), row-major R), the frame a shift or a
    # rotation of the group is local to (batoid's CompoundOptic / Lens coordSys)
    groups: dict = dataclasses.field(default_factory=dict)
    # the group the camera rotator and focusZ move (imsim's cameraName)
    camera_name: str = "LSSTCamera"

    @property
    def perturbed(self):
        """True when some surface is moved or figured: the perturbed trace applies"""
        return any(not S.coaxial for S in self.surfaces)

    def with_detector_z(self, z):
        surf = [dataclasses.replace(s) for s in self.surfaces]
        surf[-1] = dataclasses.replace(surf[-1], z0=z)
        return dataclasses.replace(self, surfaces=surf)


def medium_n(medium, wave_nm):
    kind, c = medium
    wave_nm = np.asarray(wave_nm, dtype=np.float64)
    if kind == _abi.IMS_MEDIUM_CONST:
        return np.full_like(wave_nm, c[0])
    if kind == _abi.IMS_MEDIUM_SELLMEIER:
        l2 = (wave_nm * 1e-3) ** 2
        return np.sqrt(1.0 + c[0] * l2 / (l2 - c[3]) + c[1] * l2 / (l2 - c[4]) + c[2] * l2 / (l2 - c[5]))
    P = c[0] * 7.50061683
    T = c[1] - 273.15
    W = c[2] * 7.50061683
    s2 = 1.0 / (wave_nm * 1e-3) ** 2
    n1 = (64.328 + 29498.1 / (146.0 - s2) + 255.4 / (41.0 - s2)) * 1e-6
    n1 = n1 * (P * (1.0 + (1.049 - 0.0157 * T) * 1e-6 * P) / (720.883 * (1.0 + 0.003661 * T)))
    n1 = n1 - (0.0624 - 0.000680 * s2) / (1.0 + 0.003661 * T) * W * 1e-6
    return 1.0 + n1


def _sag(S, r2):
    z = np.zeros_like(r2)
    dz = np.zeros_like(r2)
    ok = np.ones(r2.shape, dtype=bool)
    if S.R != 0.0:
        c = 1.0 / S.R
        arg = 1.0 - (1.0 + S.conic) * c * c * r2
        ok = arg >= 0
        sq = np.sqrt(np.where(ok, arg, 1.0))
        z = c * r2 / (1.0 + sq)
        dz = c / (2.0 * sq)
    rp = r2.copy()
    for k, a in enumerate(S.asph):
        dz = dz + a * (k + 2) * rp
        rp = rp * r2
        z = z + a * rp
    return z, dz, ok


def _obsc_vig(S, r):
    if S.obsc_kind == _abi.IMS_OBSC_CLEAR_ANNULUS:
        return ~((r >= S.obsc_inner) & (r <= S.obsc_outer))
    if S.obsc_kind == _abi.IMS_OBSC_CLEAR_CIRCLE:
        return ~(r <= S.obsc_outer)
    if S.obsc_kind == _abi.IMS_OBSC_OBSC_CIRCLE:
        return r < S.obsc_outer
    if S.obsc_kind == _abi.IMS_OBSC_OBSC_ANNULUS:
        return (r >= S.obsc_inner) & (r < S.obsc_outer)
    return np.zeros(r.shape, dtype=bool)


def _obsc_edge(S, r):
    """distance of r from the nearest edge of S's obscuration (inf without one)"""
    if S.obsc_kind == _abi.IMS_OBSC_NONE:
        return np.full(r.shape, np.inf)
    d = np.abs(r - S.obsc_outer)
    if S.obsc_kind in (_abi.IMS_OBSC_CLEAR_ANNULUS, _abi.IMS_OBSC_OBSC_ANNULUS):
        d = np.minimum(d, np.abs(r - S.obsc_inner))
    return d


def trace_numpy(tel: Telescope, pos, vel, wave_nm, local_last=False, edge=False):
    """Vectorised host tracer with the same algorithm as the kernel (used to fit the WCS and to
    focus the approximate prescription; NOT part of the photon path).  pos, vel: (n,3).

    A moved surface (Surface.origin / rot) is traced in its frame: the ray goes in, meets the surface whose vertex is the
    origin, is vignetted with the local x, y and bent with the normal of the full sag (conic + asphere + Zernike figure, Newton
    on z - sag(x, y) with its x / y gradient), and comes out again -- except the last surface with local_last (the photon
    trace's detector hit, in the detector's frame).  edge=True also returns every ray's smallest distance from an obscuration
    edge it was tested against [m]."""
    pos = np.array(pos, dtype=np.float64)
    vel = np.array(vel, dtype=np.float64)
    wave_nm = np.broadcast_to(np.asarray(wave_nm, dtype=np.float64), pos.shape[:1])
    vig = np.zeros(len(pos), dtype=bool)
    fail = np.zeros(len(pos), dtype=bool)
    near = np.full(len(pos), np.inf)
    n_cur = medium_n(tel.in_medium, wave_nm)
    for i_s, S in enumerate(tel.surfaces):
        moved = S.origin is not None or S.rot is not None
        fig = surface_figure_cartesian(S)
        if moved:
            o, Rm = S.frame()
            pos = (pos - o) @ Rm
            vel = vel @ Rm
            z0 = 0.0
        else:
            z0 = S.z0
        pz = pos[:, 2] - z0
        if S.R != 0.0:
            k1 = 1.0 + S.conic
            A = vel[:, 0] ** 2 + vel[:, 1] ** 2 + k1 * vel[:, 2] ** 2
            B = 2.0 * (pos[:, 0] * vel[:, 0] + pos[:, 1] * vel[:, 1] + k1 * pz * vel[:, 2] - S.R * vel[:, 2])
            Cq = pos[:, 0] ** 2 + pos[:, 1] ** 2 + k1 * pz * pz - 2.0 * S.R * pz
            disc = B * B - 4.0 * A * Cq
            fail |= disc < 0
            sq = np.sqrt(np.clip(disc, 0.0, None))
            q = -0.5 * (B + np.where(B < 0, -sq, sq))
            with np.errstate(divide="ignore", invalid="ignore"):
                t1, t2 = q / A, Cq / q
            z1, z2 = pz + vel[:, 2] * t1, pz + vel[:, 2] * t2
            t = np.where((np.abs(z2) <= np.abs(z1)) | ~(np.abs(z1) < 1e300), t2, t1)
        else:
            t = -pz / vel[:, 2]

        def full_sag(x, y):
            sag, ds, ok = _sag(S, x * x + y * y)
            gx, gy = 2.0 * ds * x, 2.0 * ds * y
            if fig is not None:
                f, fx, fy = poly2d_eval(fig[1], x * fig[0], y * fig[0], fig[0])
                sag, gx, gy = sag + f, gx + fx, gy + fy
            return sag, gx, gy, ok

        if fig is None:
            for _ in range(5 if S.asph else 0):
                x = pos[:, 0] + vel[:, 0] * t
                y = pos[:, 1] + vel[:, 1] * t
                z = pz + vel[:, 2] * t
                sag, ds, ok = _sag(S, x * x + y * y)
                fail |= ~ok
                f = z - sag
                fp = vel[:, 2] - 2.0 * ds * (x * vel[:, 0] + y * vel[:, 1])
                t = np.where(np.abs(f) <= 1e-14, t, t - f / fp)
        else:
            for _ in range(8):
                x = pos[:, 0] + vel[:, 0] * t
                y = pos[:, 1] + vel[:, 1] * t
                z = pz + vel[:, 2] * t
                sag, gx, gy, ok = full_sag(x, y)
                fail |= ~ok
                f = z - sag
                fp = vel[:, 2] - (gx * vel[:, 0] + gy * vel[:, 1])
                t = np.where(np.abs(f) <= 1e-15, t, t - f / fp)
        x = pos[:, 0] + vel[:, 0] * t
        y = pos[:, 1] + vel[:, 1] * t
        if fig is None:
            sag, ds, ok = _sag(S, x * x + y * y)
            gx, gy = 2.0 * ds * x, 2.0 * ds * y
        else:
            sag, gx, gy, ok = full_sag(x, y)
        fail |= ~ok
        pos = np.stack([x, y, z0 + sag], axis=1)
        r = np.hypot(x, y)
        vig |= _obsc_vig(S, r)
        if edge:
            near = np.minimum(near, _obsc_edge(S, r))
        if S.kind not in (_abi.IMS_SURF_BAFFLE, _abi.IMS_SURF_DETECTOR):
            nrm = np.stack([-gx, -gy, np.ones_like(x)], axis=1)
            nrm /= np.linalg.norm(nrm, axis=1)[:, None]
            if S.kind == _abi.IMS_SURF_MIRROR:
                d = np.sum(vel * nrm, axis=1)
                vel = vel - 2.0 * d[:, None] * nrm
            else:
                n2 = medium_n(S.medium, wave_nm)
                dvec = vel * n_cur[:, None]
                alpha = np.sum(dvec * nrm, axis=1)
                flip = alpha > 0
                nrm[flip] = -nrm[flip]
                alpha = np.where(flip, -alpha, alpha)
                eta = n_cur / n2
                sinsqr = eta * eta * (1.0 - alpha * alpha)
                fail |= sinsqr > 1.0
                nfac = eta * alpha + np.sqrt(np.clip(1.0 - sinsqr, 0.0, None))
                vel = (eta[:, None] * dvec - nfac[:, None] * nrm) / n2[:, None]
                n_cur = n2
        if moved and not (local_last and i_s == len(tel.surfaces) - 1):
            pos = pos @ Rm.T + o
            vel = vel @ Rm.T
    if edge:
        return pos, vel, vig, fail, near
    return pos, vel, vig, fail


# Reference-sphere radius of rubin_like_telescope: its exit-pupil distance, found once by tracing a chief ray (from the stop
# centre, field 1e-4 rad, r band, refocused detector) and extending it from the detector hit to the optical axis -- the exit
# pupil of the stand-in is virtual, 2.7038 m beyond the detector (2.7024 .. 2.7062 m over the bands).
RUBIN_LIKE_SPHERE_RADIUS = 2.7038


def rubin_like_telescope(band="r", refocus=True):
    """APPROXIMATE Rubin/LSST prescription (public optical-design values recalled, not batoid's
    LSST_r.yaml): M1/M2/M3, three fused-silica lenses, filter, detector.  The detector position is
    refocused numerically so the system forms a sharp image.  For benchmarking and tests only."""
    M, RF, DET = _abi.IMS_SURF_MIRROR, _abi.IMS_SURF_REFRACT, _abi.IMS_SURF_DETECTOR
    CA, CC = _abi.IMS_OBSC_CLEAR_ANNULUS, _abi.IMS_OBSC_CLEAR_CIRCLE
    z_m3 = -0.2338
    z_l1 = z_m3 + 3.6305
    filt_t = dict(u=0.0265, g=0.0215, r=0.0179, i=0.0158, z=0.0144, y=0.0130).get(band, 0.0179)
    z_l1b = z_l1 + 0.08223
    z_l2 = z_l1b + 0.41264
    z_l2b = z_l2 + 0.030
    z_f = z_l2b + 0.34958
    z_fb = z_f + filt_t
    z_l3 = z_fb + 0.0511
    z_l3b = z_l3 + 0.060
    z_det = z_l3b + 0.0285
    surf = [
        Surface(M, 0.0, 19.835, -1.215, (0.0, -1.381e-9), CA, 2.558, 4.18, name="M1"),
        Surface(M, 6.1562006, 6.788, -0.222, (0.0, 1.274e-5, 9.68e-7), CA, 0.9, 1.71, name="M2"),
        Surface(M, z_m3, 8.3445, 0.155, (0.0, 4.5e-7, 8.15e-9), CA, 0.55, 2.508, name="M3"),
        Surface(RF, z_l1, 2.824, 0.0, (), CC, 0.0, 0.775, SILICA, "L1_entrance", "LSSTCamera.L1.L1_entrance"),
        Surface(RF, z_l1b, 5.021, 0.0, (), CC, 0.0, 0.775, VACUUM, "L1_exit", "LSSTCamera.L1.L1_exit"),
        Surface(RF, z_l2, 0.0, 0.0, (), CC, 0.0, 0.551, SILICA, "L2_entrance", "LSSTCamera.L2.L2_entrance"),
        Surface(RF, z_l2b, 2.529, -1.57, (0.0, -1.656e-3), CC, 0.0, 0.551, VACUUM, "L2_exit", "LSSTCamera.L2.L2_exit"),
        Surface(RF, z_f, 5.632, 0.0, (), CC, 0.0, 0.375, SILICA, "Filter_entrance", "LSSTCamera.Filter.Filter_entrance"),
        Surface(RF, z_fb, 5.606, 0.0, (), CC, 0.0, 0.375, VACUUM, "Filter_exit", "LSSTCamera.Filter.Filter_exit"),
        Surface(RF, z_l3, 3.169, -0.962, (), CC, 0.0, 0.361, SILICA, "L3_entrance", "LSSTCamera.L3.L3_entrance"),
        Surface(RF, z_l3b, -13.36, 0.0, (), CC, 0.0, 0.361, VACUUM, "L3_exit", "LSSTCamera.L3.L3_exit"),
        Surface(DET, z_det, 0.0, 0.0, (), CC, 0.0, 0.4, name="Detector", path="LSSTCamera.Detector"),
    ]
    # the groups of batoid's LSST files.  Each rotates about its origin on the axis: a lens and the filter about the vertex of
    # their entrance surface, the camera about the vertex of L1's entrance (M1, M2, M3 and the detector, single surfaces, about
    # their own vertex)
    eye = tuple(np.eye(3).ravel())
    groups = {"LSSTCamera": ((0.0, 0.0, z_l1), eye), "LSSTCamera.L1": ((0.0, 0.0, z_l1), eye),
              "LSSTCamera.L2": ((0.0, 0.0, z_l2), eye), "LSSTCamera.Filter": ((0.0, 0.0, z_f), eye),
              "LSSTCamera.L3": ((0.0, 0.0, z_l3), eye)}
    tel = Telescope(surf, stop_z=0.4393899, in_medium=VACUUM, name=f"rubin_like_{band}", sphere_radius=RUBIN_LIKE_SPHERE_RADIUS,
                    groups=groups)
    if refocus:
        tel = refocus_detector(tel)
    return tel


def pupil_rays(tel, thx, thy, n_ring=6, n_az=24, wave_nm=620.0):
    """Rays filling the annular pupil for field angle (thx, thy) [rad]."""
    rr = np.linspace(tel.pupil_inner + 0.05, tel.pupil_outer - 0.05, n_ring)
    aa = np.linspace(0.0, 2 * np.pi, n_az, endpoint=False)
    r, a = np.meshgrid(rr, aa)
    x, y = (r * np.cos(a)).ravel(), (r * np.sin(a)).ravel()
    g = 1.0 / math.sqrt(1.0 + thx * thx + thy * thy)
    n = medium_n(tel.in_medium, np.array([wave_nm]))[0]
    vel = np.tile(np.array([thx * g, thy * g, -g]) / n, (len(x), 1))
    pos = np.stack([x, y, np.full_like(x, tel.stop_z)], axis=1)
    return pos, vel


def spot_rms(tel, fields=((0.0, 0.0), (0.012, 0.0), (0.0, 0.02), (0.018, 0.018)), wave_nm=620.0):
    tot = 0.0
    for thx, thy in fields:
        pos, vel = pupil_rays(tel, thx, thy, wave_nm=wave_nm)
        p, _, vig, fail = trace_numpy(tel, pos, vel, wave_nm)
        good = ~(vig | fail)
        if good.sum() < 10:
            return 1e9
        tot += np.var(p[good, 0]) + np.var(p[good, 1])
    return math.sqrt(tot / len(fields))


def refocus_detector(tel, span=0.02, n=81):
    """Move the detector plane to the best-focus z (minimum mean spot rms over a few field points)."""
    z0 = tel.surfaces[-1].z0
    zs = np.linspace(z0 - span, z0 + span, n)
    best = min(zs, key=lambda z: spot_rms(tel.with_detector_z(z)))
    zs = np.linspace(best - 2 * span / n, best + 2 * span / n, 41)
    best = min(zs, key=lambda z: spot_rms(tel.with_detector_z(z)))
    return tel.with_detector_z(float(best))


# ---------------- batoid-format YAML ----------------
def _medium_from_yaml(m, default):
    if m is None:
        return default
    if isinstance(m, (int, float)):
        return (_abi.IMS_MEDIUM_CONST, (float(m), 0, 0, 0, 0, 0))
    t = m.get("type", "ConstMedium")
    if t == "ConstMedium":
        return (_abi.IMS_MEDIUM_CONST, (float(m["n"]), 0, 0, 0, 0, 0))
    if t == "SellmeierMedium":
        return (_abi.IMS_MEDIUM_SELLMEIER, tuple(float(m[k]) for k in ("B1", "B2", "B3", "C1", "C2", "C3")))
    if t == "Air":
        return (_abi.IMS_MEDIUM_AIR, (float(m.get("pressure", 69.328)), float(m.get("temperature", 293.15)),
                                      float(m.get("h2o_pressure", 1.067)), 0, 0, 0))
    raise ValueError(f"unsupported medium {t}")


def _surface_from_yaml(s):
    t = s.get("type", "Plane")
    if t == "Plane":
        return 0.0, 0.0, ()
    if t == "Sphere":
        return float(s["R"]), 0.0, ()
    if t == "Paraboloid":
        return float(s["R"]), -1.0, ()
    if t == "Quadric":
        return float(s["R"]), float(s["conic"]), ()
    if t == "Asphere":
        return float(s["R"]), float(s["conic"]), tuple(float(c) for c in s.get("coefs", []))
    raise ValueError(f"unsupported surface {t}")


def _obsc_from_yaml(o):
    if o is None:
        return _abi.IMS_OBSC_NONE, 0.0, 0.0
    t = o["type"]
    if t == "ClearAnnulus":
        return _abi.IMS_OBSC_CLEAR_ANNULUS, float(o["inner"]), float(o["outer"])
    if t == "ClearCircle":
        return _abi.IMS_OBSC_CLEAR_CIRCLE, 0.0, float(o["radius"])
    if t == "ObscCircle":
        return _abi.IMS_OBSC_OBSC_CIRCLE, 0.0, float(o["radius"])
    if t == "ObscAnnulus":
        return _abi.IMS_OBSC_OBSC_ANNULUS, float(o["inner"]), float(o["outer"])
    if t == "ObscNegation":
        inner = o["original"]
        k, a, b = _obsc_from_yaml(inner)
        flip = {_abi.IMS_OBSC_OBSC_CIRCLE: _abi.IMS_OBSC_CLEAR_CIRCLE, _abi.IMS_OBSC_OBSC_ANNULUS: _abi.IMS_OBSC_CLEAR_ANNULUS,
                _abi.IMS_OBSC_CLEAR_CIRCLE: _abi.IMS_OBSC_OBSC_CIRCLE, _abi.IMS_OBSC_CLEAR_ANNULUS: _abi.IMS_OBSC_OBSC_ANNULUS}
        return flip[k], a, b
    raise ValueError(f"unsupported obscuration {t}")


def _coord_frame(node, parent):
    """the item's frame from its coordSys relative to the parent frame (origin, R): shift in the parent's axes, then
    rotX, rotY, rotZ about the local axes in that order, as batoid's YAML parser composes them"""
    o, R = parent
    cs = node.get("coordSys") or {}
    o = o + R @ np.array([float(cs.get(k, 0.0)) for k in ("x", "y", "z")])
    for k, rot in (("rotX", rot_x), ("rotY", rot_y), ("rotZ", rot_z)):
        a = float(cs.get(k, 0.0))
        if a != 0.0:
            R = R @ rot(a)
    return o, R


def _walk_yaml(node, frame, in_medium, out, groups, prefix):
    t = node["type"]
    if t in ("CompoundOptic", "Lens"):
        fr = _coord_frame(node, frame)
        path = prefix + node.get("name", "") if node.get("name") else prefix.rstrip(".")
        if path:
            groups[path] = (tuple(float(v) for v in fr[0]), tuple(float(v) for v in fr[1].ravel()))
        sub = path + "." if path else ""
        medium = _medium_from_yaml(node.get("medium"), in_medium)
        items = node.get("items", [])
        if t == "Lens":
            first, last = items[0], items[-1]
            _walk_item(first, fr, in_medium, medium, out, sub)
            _walk_item(last, fr, medium, in_medium, out, sub)
        else:
            for it in items:
                _walk_yaml(it, fr, _medium_from_yaml(node.get("inMedium"), in_medium), out, groups, sub)
        return
    _walk_item(node, frame, in_medium, _medium_from_yaml(node.get("outMedium", node.get("medium")), in_medium), out, prefix)


def _walk_item(node, parent, in_medium, out_medium, out, prefix):
    o, R = _coord_frame(node, parent)
    R_, conic, asph = _surface_from_yaml(node.get("surface", {}))
    ok, oi, oo = _obsc_from_yaml(node.get("obscuration"))
    kind = {"Mirror": _abi.IMS_SURF_MIRROR, "RefractiveInterface": _abi.IMS_SURF_REFRACT,
            "Detector": _abi.IMS_SURF_DETECTOR, "Baffle": _abi.IMS_SURF_BAFFLE,
            "Interface": _abi.IMS_SURF_BAFFLE}.get(node["type"])
    if kind is None:
        raise ValueError(f"unsupported optic type {node['type']}")
    name = node.get("name", "")
    S = Surface(kind, float(o[2]), R_, conic, asph, ok, oi, oo, out_medium, name, prefix + name,
                r_outer=float(node["R_outer"]) if "R_outer" in node else None,
                r_inner=float(node.get("R_inner", 0.0)) if "R_outer" in node else None)
    if o[0] != 0.0 or o[1] != 0.0 or not np.array_equal(R, np.eye(3)):
        S.origin = tuple(float(v) for v in o)
        S.rot = tuple(float(v) for v in R.ravel())
    out.append(S)


def load_batoid_yaml(path):
    """Read a batoid optic YAML into a Telescope: every surface keeps its item path, and a coordSys with x, y or rotations
    (composed down the tree of CompoundOptic / Lens items) gives the surface its frame -- a perturbed telescope."""
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f)["opticalSystem"]
    in_medium = _medium_from_yaml(cfg.get("inMedium", cfg.get("medium")), VACUUM)
    out: List[Surface] = []
    groups = {}
    top = (np.zeros(3), np.eye(3))
    if cfg.get("type") in ("CompoundOptic", "Lens"):
        # the top-level optic names the telescope, not an item path (batoid's itemDict keys start below it)
        fr = _coord_frame(cfg, top)
        medium = _medium_from_yaml(cfg.get("inMedium"), in_medium)
        for it in cfg.get("items", []):
            _walk_yaml(it, fr, medium, out, groups, "")
    else:
        _walk_yaml(cfg, top, in_medium, out, groups, "")
    stop = cfg.get("stopSurface", {})
    stop_z = float((stop.get("coordSys") or {}).get("z", 0.0))
    pupil = float(cfg.get("pupilSize", 8.36)) / 2.0
    eps = float(cfg.get("pupilObscuration", 0.612))
    sphere = cfg.get("sphereRadius")
    cam = "LSSTCamera" if "LSSTCamera" in groups or not groups else next((g for g in groups if "." not in g and "Cam" in g),
                                                                         "LSSTCamera")
    return Telescope(out, stop_z=stop_z, in_medium=in_medium, pupil_outer=pupil, pupil_inner=pupil * eps,
                     name=cfg.get("name", "telescope"), sphere_radius=None if sphere is None else float(sphere), eps=eps,
                     groups=groups, camera_name=cam)


# ---------------- perturbations (imsim/telescope_loader.py:121-252) ----------------
def item_names(tel):
    """every item path of the telescope: groups and surfaces"""
    return list(tel.groups) + [S.item_path for S in tel.surfaces]


def resolve_item(tel, name):
    """the item path `name` refers to, as batoid's itemDict lookup: a full dotted path (with or without the telescope's own
    name in front) or a unique last component"""
    names = item_names(tel)
    key = str(name)
    if key.startswith(tel.name + "."):
        key = key[len(tel.name) + 1:]
    if key in names:
        return key
    hits = [n for n in names if n.split(".")[-1] == key or n.endswith("." + key)]
    if len(hits) == 1:
        return hits[0]
    if not hits:
        raise ValueError(f"optic {name!r} not found in telescope {tel.name} (items: {', '.join(names)})")
    raise ValueError(f"optic {name!r} is ambiguous in telescope {tel.name}: {', '.join(hits)}")


def _item_frame(tel, path):
    if path in tel.groups:
        o, R = tel.groups[path]
        return np.array(o, dtype=np.float64), np.array(R, dtype=np.float64).reshape(3, 3)
    return next(S for S in tel.surfaces if S.item_path == path).frame()


def _members(tel, path):
    """(surface indices, group paths) that move with item `path`"""
    inside = lambda p: p == path or p.startswith(path + ".")
    return [k for k, S in enumerate(tel.surfaces) if inside(S.item_path)], [g for g in tel.groups if inside(g)]


def _set_frame(S, o, R):
    S.origin = tuple(float(v) for v in o)
    S.rot = tuple(float(v) for v in R.ravel())
    S.z0 = S.origin[2]


def _copy(tel):
    return dataclasses.replace(tel, surfaces=[dataclasses.replace(S) for S in tel.surfaces], groups=dict(tel.groups))


def shift_optic(tel, name, shift):
    """batoid's withLocallyShiftedOptic: the item and everything in it move by `shift` given in the item's own axes"""
    shift = np.asarray(shift, dtype=np.float64)
    if not np.any(shift != 0.0):
        return tel
    tel = _copy(tel)
    path = resolve_item(tel, name)
    _, R = _item_frame(tel, path)
    d = R @ shift
    surf, groups = _members(tel, path)
    for k in surf:
        o, Rs = tel.surfaces[k].frame()
        _set_frame(tel.surfaces[k], o + d, Rs)
    for g in groups:
        o, Rg = tel.groups[g]
        tel.groups[g] = (tuple(float(v) for v in np.array(o) + d), Rg)
    return tel


def rotate_optic(tel, name, rot):
    """batoid's withLocallyRotatedOptic: the item and everything in it turn by `rot` (3 x 3, in the item's own axes) about
    the item's origin"""
    rot = np.asarray(rot, dtype=np.float64)
    if np.array_equal(rot, np.eye(3)):
        return tel
    tel = _copy(tel)
    path = resolve_item(tel, name)
    og, Rg = _item_frame(tel, path)
    G = Rg @ rot @ Rg.T
    surf, groups = _members(tel, path)
    for k in surf:
        o, Rs = tel.surfaces[k].frame()
        _set_frame(tel.surfaces[k], og + G @ (o - og), G @ Rs)
    for g in groups:
        o, Rs = _item_frame(tel, g)
        tel.groups[g] = (tuple(float(v) for v in og + G @ (o - og)), tuple(float(v) for v in (G @ Rs).ravel()))
    return tel


def figure_optic(tel, name, coef, r_outer=None, r_inner=None):
    """batoid's withPerturbedSurface(name, Zernike(coef, R_outer, R_inner)): the interface's sag gains the figure"""
    coef = tuple(float(c) for c in coef)
    if not any(c != 0.0 for c in coef[1:]):
        return tel
    tel = _copy(tel)
    path = resolve_item(tel, name)
    hits = [k for k, S in enumerate(tel.surfaces) if S.item_path == path]
    if not hits:
        raise ValueError(f"Zernike perturbation of {name!r}: not an interface (a surface of the telescope)")
    S = tel.surfaces[hits[0]]
    if r_outer is None:
        r_outer, r_inner = S.radii()
    fig = Figure(coef, float(r_outer), float(r_inner))
    if fig.cartesian().shape[0] - 1 > _abi.IMS_FIG_MAX_DEG:
        raise ValueError(f"Zernike perturbation of {name!r}: radial order above {_abi.IMS_FIG_MAX_DEG}")
    S.figure = tuple(S.figure) + (fig,)
    return tel


def _check_shift(v):
    if not isinstance(v, (list, tuple, np.ndarray)) or len(v) != 3:
        raise ValueError("Expecting a list of 3 elements")
    try:
        return [float(x) for x in v]
    except (TypeError, ValueError):
        raise ValueError(f"shift: the elements must be numbers, got {list(v)!r}") from None


def zernike_coef(pval):
    """coef (Noll order, [0] unused) of a Zernike perturbation dict: `coef`, or `idx` + `val` (scalars or lists)"""
    if "coef" in pval and "idx" in pval:
        raise ValueError("Cannot specify both coef and idx for Zernike perturbation")
    if "coef" in pval:
        return [float(c) for c in pval["coef"]]
    if "idx" not in pval:
        raise ValueError("Zernike perturbation: give coef, or idx and val")
    idx, val = pval["idx"], pval.get("val")
    idx = [int(i) for i in idx] if isinstance(idx, (list, tuple)) else [int(idx)]
    val = [float(v) for v in val] if isinstance(val, (list, tuple)) else [float(val)]
    if len(idx) != len(val):
        raise ValueError("Zernike perturbation: idx and val differ in length")
    coef = [0.0] * (max(idx) + 1)
    for i, v in zip(idx, val):
        coef[i] = v
    return coef


def apply_perturbations(tel, groups):
    """load_telescope's perturbations (imsim/telescope_loader.py:211-238): a dict {optic: {kind: value}} or a list of them,
    applied in order -- the list, the optics within a dict and the kinds within an optic's dict.  Kinds: shift [dx, dy, dz]
    (local to the optic), rotX / rotY / rotZ [rad] (about the optic's origin, local axes), Zernike {coef | idx + val,
    R_outer, R_inner} (one interface; the radii from the optic when both are absent).  A perturbation that is exactly zero
    leaves the telescope as it is."""
    if groups is None:
        return tel
    if isinstance(groups, dict):
        groups = [groups]
    for group in groups:
        if not isinstance(group, dict):
            raise ValueError(f"perturbations: expected a dict of optics, got {group!r}")
        for optic, perturbs in group.items():
            if not isinstance(perturbs, dict):
                raise ValueError(f"perturbations of {optic!r}: expected a dict, got {perturbs!r}")
            for ptype, pval in perturbs.items():
                if ptype == "shift":
                    tel = shift_optic(tel, optic, _check_shift(pval))
                elif ptype in ("rotX", "rotY", "rotZ"):
                    tel = rotate_optic(tel, optic, {"rotX": rot_x, "rotY": rot_y, "rotZ": rot_z}[ptype](float(pval)))
                elif ptype == "Zernike":
                    if not isinstance(pval, dict):
                        raise ValueError(f"Zernike perturbation of {optic!r}: expected a dict")
                    ro, ri = pval.get("R_outer"), pval.get("R_inner")
                    if (ro is None) != (ri is None):
                        raise ValueError("Must specify both or neither of R_outer and R_inner")
                    tel = figure_optic(tel, optic, zernike_coef(pval), None if ro is None else float(ro),
                                       None if ri is None else float(ri))
                else:
                    raise ValueError(f"unknown perturbation {ptype!r} of {optic!r} (shift, rotX, rotY, rotZ, Zernike)")
    return tel


def focus_camera(tel, focus_z):
    """load_telescope's focusZ: the camera shifted by [0, 0, focusZ] in its own axes"""
    return shift_optic(tel, tel.camera_name, [0.0, 0.0, float(focus_z)]) if focus_z else tel


def with_camera_rotation(tel, rot_tel_pos):
    """load_telescope's rotTelPos: the camera turned by RotZ(rot_tel_pos) about its origin"""
    return rotate_optic(tel, tel.camera_name, rot_z(rot_tel_pos)) if rot_tel_pos else tel


# ---------------- ABI struct ----------------
def fill_optics(o: "_abi.Optics", tel: Telescope, fp_to_pix, rot_tel_pos=0.0):
    """Write the telescope, the camera rotator and the focal-plane->pixel affine into an Optics struct.

    fp_to_pix = (m0, m1, m2, m3, m4, m5): x_pix = m0*fpx + m1*fpy + m2, y_pix = m3*fpx + m4*fpy + m5
    (imsim/utils.py:42-59; e.g. R22_S11: (100, 0, 2047.5, 0, 100, 2001.5), tests/test_photon_ops.py:668-691)."""
    if len(tel.surfaces) > _abi.IMS_MAX_SURFACES:
        raise ValueError("too many surfaces")
    if tel.perturbed:
        if not isinstance(o, _abi.OpticsPerturbed):
            raise ValueError("a perturbed telescope needs an _abi.OpticsPerturbed descriptor (make_optics)")
        # the camera rotator is a rotation of the camera (load_telescope): part of the frames, the detector hit comes back in
        # the rotated detector's frame
        tel = with_camera_rotation(tel, rot_tel_pos)
        rot_tel_pos = 0.0
        fill_perturbation(o.pert, tel)

    def medium_coeffs(medium):
        c = [float(v) for v in medium[1]]
        if medium[0] == _abi.IMS_MEDIUM_CONST:
            c[1] = 1.0 / c[0]            # constant media carry 1/n for the kernel (include/imsim_hip.h)
        return c

    o.in_medium_kind = tel.in_medium[0]
    for k, v in enumerate(medium_coeffs(tel.in_medium)):
        o.in_medium_c[k] = v
    o.n_surfaces = len(tel.surfaces)
    o.stop_z = tel.stop_z
    media = {}
    for k, S in enumerate(tel.surfaces):
        s = o.surf[k]
        s.medium_id = media.setdefault((S.medium[0], tuple(float(c) for c in S.medium[1])), len(media))
        s.kind, s.obsc_kind, s.medium_kind = S.kind, S.obsc_kind, S.medium[0]
        if len(S.asph) > 4:
            raise ValueError("at most 4 asphere coefficients")
        s.n_asphere = len(S.asph)
        s.z0, s.R, s.conic = S.z0, S.R, S.conic
        s.inv_R = (1.0 / S.R) if S.R != 0.0 else 0.0
        for m in range(4):
            s.asph[m] = float(S.asph[m]) if m < len(S.asph) else 0.0
        s.obsc_inner, s.obsc_outer = S.obsc_inner, S.obsc_outer
        for m, v in enumerate(medium_coeffs(S.medium)):
            s.medium_c[m] = v
    o.cam_rot[0], o.cam_rot[1] = math.cos(rot_tel_pos), math.sin(rot_tel_pos)
    for k in range(6):
        o.fp_to_pix[k] = float(fp_to_pix[k])
    a, b, c, d = fp_to_pix[0], fp_to_pix[1], fp_to_pix[3], fp_to_pix[4]
    s = math.sqrt(abs(a * d - b * c))
    # normalised M @ J with M = [[0, 1e3], [1e3, 0]] (imsim/photon_ops.py:497-500)
    o.slope_jac[0], o.slope_jac[1], o.slope_jac[2], o.slope_jac[3] = c / s, d / s, a / s, b / s
    return o


def fill_perturbation(pt: "_abi.Perturbation", tel: Telescope):
    """ims_perturbation_t of `tel`: every surface's frame and its figures as one Cartesian polynomial"""
    for k, S in enumerate(tel.surfaces):
        F = pt.surf[k]
        moved = S.origin is not None or S.rot is not None
        F.moved = 1 if moved else 0
        o, R = S.frame()
        for m in range(3):
            F.origin[m] = float(o[m])
        for m in range(9):
            F.rot[m] = float(R.ravel()[m])
        fig = surface_figure_cartesian(S)
        F.fig_deg, F.fig_inv_r = 0, 0.0
        for m in range(_abi.IMS_FIG_NCOEF):
            F.fig[m] = 0.0
        if fig is not None:
            inv_r, C = fig
            d = C.shape[0] - 1
            if d > _abi.IMS_FIG_MAX_DEG:
                raise ValueError(f"figure of {S.item_path}: degree {d} > {_abi.IMS_FIG_MAX_DEG}")
            F.fig_deg, F.fig_inv_r = max(d, 1), inv_r
            for p_ in range(d + 1):
                for q in range(d + 1 - p_):
                    F.fig[_abi.fig_row(p_) + q] = float(C[p_, q])
    return pt


def make_optics(tel: Telescope, fp_to_pix, rot_tel_pos=0.0, force_perturbed=False):
    """A filled descriptor for `tel`: _abi.Optics for a coaxial telescope, _abi.OpticsPerturbed (the perturbed trace) for a
    perturbed one -- or for any with force_perturbed (the perturbed trace of a coaxial telescope, for comparisons)."""
    if tel.perturbed or force_perturbed:
        o = _abi.OpticsPerturbed()
        if not tel.perturbed:
            tel = with_camera_rotation(tel, rot_tel_pos)
            rot_tel_pos = 0.0
            fill_perturbation(o.pert, tel)
        return fill_optics(o, tel, fp_to_pix, rot_tel_pos)
    return fill_optics(_abi.Optics(), tel, fp_to_pix, rot_tel_pos)


def field_to_pixel(tel, thx, thy, fp_to_pix, rot_tel_pos=0.0, wave_nm=620.0):
    """Pixel position of the pupil-averaged image of field angle (thx, thy) (the focal-plane
    position batoid_wcs.py:352-373 computes, followed by focal_to_pixel).  A perturbed telescope is traced with its camera
    turned by the rotator angle and the hit taken in the detector's frame, as the kernel does."""
    pos, vel = pupil_rays(tel, thx, thy, wave_nm=wave_nm)
    if tel.perturbed:
        p, _, vig, fail = trace_numpy(with_camera_rotation(tel, rot_tel_pos), pos, vel, wave_nm, local_last=True)
        good = ~(vig | fail)
        x, y = p[good, 0].mean(), p[good, 1].mean()
        fpx, fpy = y * 1e3, x * 1e3
        return (fp_to_pix[0] * fpx + fp_to_pix[1] * fpy + fp_to_pix[2],
                fp_to_pix[3] * fpx + fp_to_pix[4] * fpy + fp_to_pix[5])
    p, _, vig, fail = trace_numpy(tel, pos, vel, wave_nm)
    good = ~(vig | fail)
    x, y = p[good, 0].mean(), p[good, 1].mean()
    c, s = math.cos(rot_tel_pos), math.sin(rot_tel_pos)
    rx, ry = c * x + s * y, -s * x + c * y
    fpx, fpy = ry * 1e3, rx * 1e3
    return (fp_to_pix[0] * fpx + fp_to_pix[1] * fpy + fp_to_pix[2],
            fp_to_pix[3] * fpx + fp_to_pix[4] * fpy + fp_to_pix[5])


class FieldTracer:
    """The batched field-point trace on the GPU (ims_trace_field_points): the descriptor and the pupil rays of
    `pupil_rays` uploaded once, then one launch per call.  There is no host fallback."""

    def __init__(self, desc_or_tel, fp_to_pix=None, rot_tel_pos=0.0, wave_nm=620.0, device="cuda:0", pupil=None):
        import ctypes as C
        import torch
        self.lib = _abi.load()
        if not torch.cuda.is_available():
            raise _abi.ImsimHipError("the GPU field-point trace needs a GPU (there is no CPU fallback)")
        if isinstance(desc_or_tel, Telescope):
            if fp_to_pix is None:
                raise ValueError("FieldTracer: a Telescope needs fp_to_pix")
            if pupil is None:
                pos, _ = pupil_rays(desc_or_tel, 0.0, 0.0, wave_nm=wave_nm)
                pupil = pos[:, :2]
            src = make_optics(desc_or_tel, fp_to_pix, rot_tel_pos)
        else:
            if pupil is None:
                raise ValueError("FieldTracer: a filled descriptor does not hold the pupil's radii; give the pupil rays")
            src = desc_or_tel
        # a private copy with the derived fields filled, as the engine does before it uploads a descriptor
        opt = type(src).from_buffer_copy(bytes(src))
        _abi.check(self.lib.ims_fill_derived_medium(int(opt.in_medium_kind), opt.in_medium_c), "ims_fill_derived_medium")
        for k in range(opt.n_surfaces):
            _abi.check(self.lib.ims_fill_derived_medium(int(opt.surf[k].medium_kind), opt.surf[k].medium_c), "ims_fill_derived_medium")
        _abi.check(self.lib.ims_fill_derived_optics(C.byref(opt)), "ims_fill_derived_optics")
        self.torch = torch
        self.dev = torch.device(device)
        self.perturbed = isinstance(opt, _abi.OpticsPerturbed)
        self.wave_nm = float(wave_nm)
        self.opt_dev = torch.from_numpy(np.frombuffer(bytes(opt), dtype=np.uint8).copy()).to(self.dev)
        pupil = np.ascontiguousarray(np.asarray(pupil, dtype=np.float64).reshape(-1, 2))
        self.n_rays = len(pupil)
        self.pupil_dev = torch.from_numpy(pupil).to(self.dev)

    def __call__(self, thx, thy):
        """(xy [n, 2] pixel positions, ngood [n] rays averaged) of the field angles thx, thy [rad]"""
        torch = self.torch
        thx = np.ascontiguousarray(np.atleast_1d(np.asarray(thx, dtype=np.float64)))
        thy = np.ascontiguousarray(np.atleast_1d(np.asarray(thy, dtype=np.float64)))
        if thx.shape != thy.shape or thx.ndim != 1:
            raise ValueError("field_to_pixel_hip: thx and thy must be 1-d arrays of one length")
        n = len(thx)
        th = torch.from_numpy(np.stack([thx, thy])).to(self.dev)
        xy = torch.empty((n, 2), dtype=torch.float64, device=self.dev)
        ngood = torch.empty(n, dtype=torch.int32, device=self.dev)
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            fn = self.lib.ims_trace_field_points_perturbed if self.perturbed else self.lib.ims_trace_field_points
            _abi.check(fn(self.opt_dev.data_ptr(), th[0].data_ptr(), th[1].data_ptr(), n, self.wave_nm, self.pupil_dev.data_ptr(),
                          self.n_rays, xy.data_ptr(), ngood.data_ptr(), stream), "ims_trace_field_points")
        return xy.cpu().numpy(), ngood.cpu().numpy()


def field_to_pixel_hip(desc_or_tel, thx, thy, fp_to_pix=None, rot_tel_pos=0.0, wave_nm=620.0, device="cuda:0", pupil=None):
    """field_to_pixel for arrays of field angles in one GPU launch: (xy [n, 2], ngood [n]).  desc_or_tel: a Telescope (with
    fp_to_pix and rot_tel_pos, the rays of pupil_rays) or a filled _abi.Optics / OpticsPerturbed (with `pupil`, [n_rays, 2])."""
    return FieldTracer(desc_or_tel, fp_to_pix, rot_tel_pos, wave_nm, device, pupil)(thx, thy)


# 0.2 arcsec per 10 micron pixel: the focal length [m] the paraxial start of build_wcs_pair divides by
PLATE_FOCAL_M = 1.0e-5 / (0.2 * math.pi / 648000.0)


def image_sign(tel):
    """+1 when the telescope's image is upright (a field angle +thx lands at +x on the detector), -1 when inverted: read off one
    chief ray from the stop centre, once per Telescope object (kept on it; a copy made by a perturbation finds its own)."""
    sign = tel.__dict__.get("_image_sign")
    if sign is None:
        h = 1e-4
        g = 1.0 / math.sqrt(1.0 + h * h)
        n = medium_n(tel.in_medium, np.array([620.0]))[0]
        p, _, _, _ = trace_numpy(tel, [[0.0, 0.0, tel.stop_z]], [[h * g / n, 0.0, -g / n]], 620.0)
        sign = tel.__dict__["_image_sign"] = 1.0 if p[0, 0] > 0.0 else -1.0
    return sign


def paraxial_field(tel, fp_to_pix, rot_tel_pos, nx, ny):
    """Field angle [rad] of the CCD's centre in the paraxial picture: its focal-plane centre (the point fp_to_pix sends to pixel
    ((nx - 1) / 2 + 0.5, (ny - 1) / 2 + 0.5)) through the rotator and the plate scale.  Exactly (0, 0) for a CCD on the axis.
    Whether the image is upright or inverted is the telescope's (image_sign)."""
    m0, m1, m2, m3, m4, m5 = (float(v) for v in fp_to_pix)
    dx, dy = (nx - 1) / 2.0 + 0.5 - m2, (ny - 1) / 2.0 + 0.5 - m5
    det = m0 * m4 - m1 * m3
    fpx, fpy = (m4 * dx - m1 * dy) / det, (m0 * dy - m3 * dx) / det          # [mm]
    if fpx == 0.0 and fpy == 0.0:
        return np.zeros(2)
    rx, ry = fpy * 1e-3, fpx * 1e-3
    c, s = math.cos(rot_tel_pos), math.sin(rot_tel_pos)
    x, y = c * rx - s * ry, s * rx + c * ry
    return np.array([x, y]) / (image_sign(tel) * PLATE_FOCAL_M)


def build_wcs_pair(tel, fp_to_pix, boresight_ra, boresight_dec, rot_sky=0.0, rot_tel_pos=0.0,
                   nx=4096, ny=4004, wave_nm=620.0, order=3, device=None, what="the CCD"):
    """Build (img_wcs, icrf_to_field) consistent with the telescope by ray tracing, as
    imsim/batoid_wcs.py does: icrf_to_field is the TAN projection about the boresight rotated by
    `rot_sky`; img_wcs is an order-3 TAN-SIP fitted through traced field points over the detector.

    The search for the detector centre's field angle starts from the paraxial guess (paraxial_field; (0, 0) on the axis).
    device=None traces on the host (field_to_pixel); with a device the three points of a Newton step are one launch of
    ims_trace_field_points and the 127 fit points another; the fit stays on the host.  A field point that no ray reaches
    unvignetted is an error naming `what`."""
    basis = wcsmod.tangent_basis(boresight_ra, boresight_dec, rot_sky)
    icrf_to_field = wcsmod.make_tansip((0.0, 0.0), np.eye(2), basis)
    if device is None:
        def trace(points):
            return np.array([field_to_pixel(tel, a, b, fp_to_pix, rot_tel_pos, wave_nm) for a, b in points])
    else:
        tracer = FieldTracer(tel, fp_to_pix, rot_tel_pos, wave_nm, device)

        def trace(points):
            points = np.asarray(points, dtype=np.float64)
            xy, ngood = tracer(points[:, 0], points[:, 1])
            if np.any(ngood == 0):
                k = int(np.flatnonzero(ngood == 0)[0])
                raise ValueError(f"WCS of {what}: no ray of field angle ({points[k, 0]:.6g}, {points[k, 1]:.6g}) rad reaches the "
                                 f"detector unvignetted ({int((ngood == 0).sum())} of {len(points)} points)")
            return xy
    # field angle of the detector centre by Newton iteration on the traced mapping
    target = np.array([(nx + 1) / 2.0, (ny + 1) / 2.0])
    th = paraxial_field(tel, fp_to_pix, rot_tel_pos, nx, ny)
    h = 1e-4
    for _ in range(8):
        p0, px, py = trace([(th[0], th[1]), (th[0] + h, th[1]), (th[0], th[1] + h)])
        J = np.stack([(px - p0) / h, (py - p0) / h], axis=1)
        th = th - np.linalg.solve(J, p0 - target)
    # hexapolar grid of field angles of radius 0.16 deg about the detector centre (batoid_wcs.py:408-427)
    rings = [(0, 1)] + [(k, 6 * k) for k in range(1, 7)]
    pts = []
    for k, m in rings:
        for j in range(m):
            r = math.radians(0.16) * k / 6.0
            a = 2 * math.pi * j / m
            pts.append((th[0] + r * math.cos(a), th[1] + r * math.sin(a)))
    pts = np.array(pts)
    pix = trace(pts)
    vec = wcsmod.tansip_pix_to_vec(icrf_to_field, pts[:, 0], pts[:, 1])
    img_wcs = wcsmod.fit_tansip(pix[:, 0], pix[:, 1], vec, crpix=target, order=order)
    return img_wcs, icrf_to_field, th
