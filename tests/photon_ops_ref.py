"""The photon operator chain restated in np.longdouble, independently of oracle/, the kernels and imsim_amd's own numpy code.

"Operator chain" = what ims_apply_ops does to a photon pool between the source (tests/photon_source_ref.py) and the sensor:
TimeSampler, PupilAnnulusSampler, PhotonDCR, FocusDepth, Refraction, BandpassRatio, RubinOptics, RubinDiffraction and
RubinDiffractionOptics.  Inputs are only what the product uploads -- the planted photon fields, the object rows, the op
descriptors as the user gave them (p[0..4]; the derived p[5..7] are formed here), the ims_optics_t block (ctypes layout of
imsim_amd._abi, pinned by tests/test_abi.py), the ratio tables, the Philox words -- and the written spec (DESIGN.md 2,
include/imsim_hip.h).  Every operator is written the way its source states it, not the way the kernel rearranges it:

* PhotonDCR: Filippenko (1982) / Edlen (1953) in its three separate terms, r0 = (n^2 - 1) / (2 n^2), kick through winv.
* Refraction: Snell's law on the unit vector of the slopes.   FocusDepth: x += dxdz depth.   BandpassRatio: linear table,
  clamped at both ends (include/imsim_hip.h, ims_lin_tables_t).
* Rubin*: TAN-SIP forward by the plain double sum, inverse by Newton to long-double resolution with cd inverted here (not the
  uploaded cdinv); the spider kick of imsim/diffraction.py (field_rotation_matrix, directed_dist, phi* = atan(1 / (2 k d)),
  kick along the element's normal times v_z, applied to the unit velocity over the index and rescaled to its old length); a
  textbook sequential trace (explicit sag, unit normals, unit direction, vector reflection and Snell, Newton on z - sag to
  long-double resolution, Sellmeier and Edlen media, surface frames and figure polynomials); cam_rot, the mm and axis swap,
  fp_to_pix, slope_jac; failed ray -> x = y = dxdz = dydz = flux = 0, vignetted -> flux = 0 with the geometry kept.

`apply` returns, next to every field, a per-photon bound and the photons "near a decision".  Bounds (EPS = 2^-52):

* time 4 EPS (|p0| + |p1|);  pupil (1.5e-11 + 8 EPS) r (the spec's sin / cos of a word, tests/test_oracle_math.py).
* DCR x, y: the two r0 ~ 2e-4 are formed with ~24 roundings each at their own size and subtracted, so the shift carries
  64 EPS r0 tan z scale, times |winv|_inf, plus 8 EPS |x|.   p[5..7]: 16 EPS of the value (test_abi.py).
* FocusDepth 4 EPS (|x| + |slope depth|);  Refraction 8 EPS |slope| (sqrt within 1 ulp, five more roundings);
  BandpassRatio 8 EPS |flux| (max(v_i, v_i+1) + |f| |v_i+1 - v_i|), f = (wl - wl_min) / wl_step being rounded at its own size.
* Rubin operators.  The kick, as a tilt of the direction: |g| v_z (phi* (8 EPS + 32 EPS / (|e_focal x e_z| |e_focal x e_z0|)) +
  dphi*/dd dd) + 1.7e-11 r phi* v_z (r the radius of the deviate g = r cos), with dphi*/dd = 1 / (2 k d^2) / (1 + 1 / (2 k d)^2)
  -- the ill-conditioning near an element -- and dd = 32 EPS (|p| + 1) + |p| 32 EPS / (|e_focal x e_z| |e_focal x e_z0|) -- the
  ill-conditioning of the rotation near the zenith -- plus the pupil's own bound; the rotation's error also turns the kick.
  Field angles: 64 EPS (|thx| + |thy| + |cd|_inf (|x| + |y| + |crpix|_1)): roundings at the size of the operands.
  A tilt of delta is a displacement of the pixel position by at most delta / (sigma_min(cd) (1 - |grad SIP|)) px; the
  reference's own central differences of the whole operator against x, y, pupil_u, pupil_v (every eighth photon of an object,
  the largest doubled for the photons in between) carry that displacement, and whatever bound those inputs already have
  (a chain), to the outputs.  RubinDiffraction adds 256 EPS (|x| + |y| + |crpix|_1) for its two WCS passes (the kernel's
  Newton stops when the step is below 1e-10 of the position: the next error is its square).
  Trace by the descriptor loop (Newton stop |G| <= 1e-8): DESIGN.md 2's claim, 5e-9 m on the detector = 5e-4 px at
  100 px / mm (scaled by |fp_to_pix|_inf), and 1.5e-9 on each component of the unit direction n
  (tests/test_trace_formulations.py): a slope (s . n_xy) / n_z then carries 1.5e-9 (|slope_jac|_inf + |slope|) sqrt(1 + rho^2).
  Perturbed trace (Newton to f64 resolution): every surface adds 64 roundings at the size of its operands -- positions up to
  S_k = max(|z0|, |R|, 10) m, unit directions -- to the ray that leaves it, and Optics.surface_conditioning gives, surface by
  surface, what a displacement (Kp[k], per metre) and a tilt (Kv[k], per radian) of that ray do to the detector point and the
  slopes, by the reference's own differences on one planted ray in 128 (doubled for the others):
  2 * 64 EPS sum_k (Kp[k] S_k + Kv[k]), the stop included, plus 8 EPS of the result.
* flux: 2 EPS |flux|.

Near a decision (flagged; compared on everything except what the decision feeds: x, y, slopes and flux for the argmin over
spider elements and for a surface hit's discriminant, flux alone for an obscuration edge):
the two smallest element distances within 64 EPS (|p| + 1) + their rotation term of each other; r^2 within
2 r (1e-8 m + 64 EPS r) of obsc^2; the conic discriminant, or the sag's radicand, within 2^-20 of their own operands.
At most 1e-4 of a case's photons may be flagged; tests/test_photon_ops.py checks that on the reference alone.

Observed worst error / bound per field (every case of tests/photon_ops_cases.py; a ratio above 1 fails the test; records, not
thresholds):

    field        oracle (CPU)   MI355X
    x            0.396          0.396
    y            0.587          0.587
    flux         0.0625         0.0625
    dxdz         0.319          0.319
    dydz         0.411          0.411
    wavelength   0              0
    pupil_u      0.461          0.461
    pupil_v      0.462          0.462
    time         0              0

(oracle: the plain and the coaxial cases -- it traces no perturbed telescope; MI355X: those and the perturbed cases.  The
perturbed traces alone: x 0.061, y 0.035, dxdz 0.047, dydz 0.046 of their rounding bounds.)

Mutations (`mutate=`, tests/test_photon_ops.py::test_teeth): every one listed in MUTATIONS is caught on the case named there;
none escapes.  Three needed an input of their own:
* slope_jac_T: slope_jac = (c, d, a, b) / s of fp_to_pix = (a, b, ., c, d, .); its transpose swaps a and d, equal for every
  science CCD (square pixels).  The case optics_aniso uploads a = 100, d = 125 px / mm.
* atan: 1 / (2 k d) = lambda / (4 pi d) ~ 5e-8 / d[m], and atan(x) - x = x^3 / 3 is below one rounding unless d is tens of
  microns.  diff1_norot_zenith plants one pupil point in 32 at 15 .. 30 um from a vane's edge.
* m1_asphere moves the descriptor loop's results by only ~10 of its bounds (0.005 px); it is caught on the perturbed trace, whose
  bound is roundings.
"""
import numpy as np

from imsim_amd import _abi
from photon_source_ref import LD, EPS, TWO_PI, SINCOS_ERR, DEVIATE_ERR, words, w01, gauss_pair

FIELDS = ("x", "y", "flux", "dxdz", "dydz", "wavelength", "pupil_u", "pupil_v", "time")
SLOT_OP = 8                                     # operator k draws from slot SLOT_OP + (k >> 1)
FLAG_CAP = 1.0e-4
OP_TIME, OP_PUPIL, OP_DCR, OP_OPTICS, OP_DIFF, OP_DIFF_OPTICS, OP_FOCUS, OP_REFRACTION, OP_RATIO = 1, 2, 3, 4, 5, 6, 7, 8, 9
OBJ_FAINT = 1
SURF_MIRROR, SURF_REFRACT, SURF_DETECTOR, SURF_BAFFLE = 1, 2, 3, 4
MEDIUM_CONST, MEDIUM_SELLMEIER, MEDIUM_AIR = 0, 1, 2
TRACE_POS_M, TRACE_DIR = LD(5e-9), LD(1.5e-9)   # DESIGN.md 2; tests/test_trace_formulations.py

# name -> the case of photon_ops_cases that catches it
MUTATIONS = {
    "dcr_64.328": "dcr_site", "dcr_29498.1": "dcr_site", "dcr_146": "dcr_site", "dcr_255.4": "dcr_site", "dcr_41": "dcr_site",
    "dcr_1.049": "dcr_site", "dcr_0.0157": "dcr_site", "dcr_720.883": "dcr_site", "dcr_0.003661": "dcr_site",
    "dcr_0.0624": "dcr_cold", "dcr_0.000680": "dcr_cold", "dcr_mmhg": "dcr_site", "dcr_du_sign": "dcr_site",
    "dcr_winv_swap": "dcr_site", "dcr_n2": "dcr_site", "cam_rot_sign": "optics_onaxis", "slope_jac_T": "optics_aniso", "atan": "diff1_norot_zenith",
    "fp_swap": "optics_onaxis", "odd_words": "diff1_norot_zenith", "slot": "diff2_rot_zenith", "no_vz": "diff3_rot_offaxis", "m1_asphere": "optics_onaxis_pert", "sellmeier": "optics_onaxis_pert",
}


def _c(name, value, mutate, to):
    return LD(to) if mutate == name else LD(value)


def lds(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


# ---------------- air ----------------
def air_n_minus_one(wave_nm, p_kpa, t_k, w_kpa, mutate=None):
    """Filippenko (1982) eq. 1-3 / Edlen (1953): sigma in 1 / um, P and W in mmHg, T in deg C"""
    s2 = (LD(1000) / wave_nm) ** 2
    mm = _c("dcr_mmhg", "7.50061683", mutate, "7.5")
    P, T, W = LD(p_kpa) * mm, LD(t_k) - LD("273.15"), LD(w_kpa) * mm
    n6 = (_c("dcr_64.328", "64.328", mutate, "64.329") + _c("dcr_29498.1", "29498.1", mutate, "29498.2") / (_c("dcr_146", 146, mutate, 147) - s2)
          + _c("dcr_255.4", "255.4", mutate, "255.5") / (_c("dcr_41", 41, mutate, 42) - s2))
    tf = 1 + _c("dcr_0.003661", "0.003661", mutate, "0.003662") * T
    n6 = n6 * (P * (1 + (_c("dcr_1.049", "1.049", mutate, "1.050") - _c("dcr_0.0157", "0.0157", mutate, "0.0158") * T) * LD("1e-6") * P)
               / (_c("dcr_720.883", "720.883", mutate, "720.884") * tf))
    n6 = n6 - (_c("dcr_0.0624", "0.0624", mutate, "0.0625") - _c("dcr_0.000680", "0.000680", mutate, "0.000681") * s2) * W / tf
    return n6 * LD("1e-6")


def refraction_r0(nm1, mutate=None):
    n2 = (1 + nm1) ** 2
    return (n2 if mutate == "dcr_n2" else n2 - 1) / (2 * n2)


def dcr_derived(p):
    """what ims_fill_derived_op must put into p[5], p[6], p[7], and the bound of each"""
    mm = LD("7.50061683")
    P, T, W = LD(p[1]) * mm, LD(p[2]) - LD("273.15"), LD(p[3]) * mm
    tf = 1 + LD("0.003661") * T
    air_p = LD("1e-6") * (P * (1 + (LD("1.049") - LD("0.0157") * T) * LD("1e-6") * P) / (LD("720.883") * tf))
    air_w = W * LD("1e-6") / tf
    r0 = refraction_r0(air_n_minus_one(LD(p[0]), p[1], p[2], p[3]))
    return [(v, 16 * EPS * abs(v)) for v in (air_p, air_w, r0)]


def snell_slopes(a, b, n):
    """slopes (dx/dz, dy/dz) of a ray entering a medium of relative index n through the plane z = const"""
    norm = np.sqrt(a * a + b * b + 1)
    ux, uy = a / norm, b / norm                         # unit vector; the tangential part shrinks by n
    tx, ty = ux / n, uy / n
    tz = np.sqrt(1 - tx * tx - ty * ty)
    return tx / tz, ty / tz


def ratio_lookup(table, wl_min, wl_step, wl):
    """linear interpolation on the knots wl_min + i wl_step, the end values outside; returns (value, bound factor)"""
    v = lds(table)
    n = len(v)
    f = (wl - LD(wl_min)) / LD(wl_step)
    i = np.clip(np.floor(f).astype(np.int64), 0, n - 2)
    a = np.clip(f - i, 0, 1)
    # the argument f = (wl - wl_min) / wl_step is rounded at its own size (hundreds of steps), and so is the fraction a = f - i
    return v[i] + a * (v[i + 1] - v[i]), np.maximum(np.abs(v[i]), np.abs(v[i + 1])) + np.abs(f) * np.abs(v[i + 1] - v[i])


# ---------------- TAN-SIP ----------------
class TanSip:
    def __init__(self, w):
        self.crpix = lds(w.crpix)
        self.cd = lds(w.cd).reshape(2, 2)
        det = self.cd[0, 0] * self.cd[1, 1] - self.cd[0, 1] * self.cd[1, 0]
        self.cdinv = np.array([[self.cd[1, 1], -self.cd[0, 1]], [-self.cd[1, 0], self.cd[0, 0]]], dtype=LD) / det
        self.rot = lds(w.rot).reshape(3, 3)
        self.order = int(w.order)
        self.a, self.b = lds(w.a).reshape(5, 5), lds(w.b).reshape(5, 5)
        self.cdmax = float(np.abs(self.cd).sum(axis=1).max())
        fro2 = (self.cd * self.cd).sum()
        self.cdmin = np.sqrt((fro2 - np.sqrt(fro2 * fro2 - 4 * det * det)) / 2)         # smallest singular value of cd [rad / px]

    def sip_gradient(self, x, y):
        """the largest |df/du| + |df/dv| + |dg/du| + |dg/dv| over the points: how far the SIP bends the linear map"""
        if self.order == 0 or not len(x):
            return LD(0)
        u, v = x - self.crpix[0], y - self.crpix[1]
        return np.max(sum(np.abs(self.sip(c, u, v, du, dv)) for c in (self.a, self.b) for du, dv in ((1, 0), (0, 1))))

    def sip(self, c, u, v, du=0, dv=0):
        """sum over p + q <= order of c[p][q] u^p v^q, or its derivative"""
        out = np.zeros_like(u)
        for p in range(self.order + 1):
            for q in range(self.order + 1 - p):
                if p < du or q < dv or c[p, q] == 0:
                    continue
                fac = (p if du else 1) * (q if dv else 1)
                out = out + fac * c[p, q] * u ** (p - du) * v ** (q - dv)
        return out

    def pix_to_vec(self, x, y):
        u, v = x - self.crpix[0], y - self.crpix[1]
        if self.order > 0:
            u, v = u + self.sip(self.a, u, v), v + self.sip(self.b, u, v)
        xi, eta = self.cd[0, 0] * u + self.cd[0, 1] * v, self.cd[1, 0] * u + self.cd[1, 1] * v
        p = [self.rot[0, k] + xi * self.rot[1, k] + eta * self.rot[2, k] for k in range(3)]
        nrm = np.sqrt(p[0] ** 2 + p[1] ** 2 + p[2] ** 2)
        return [c / nrm for c in p]

    def vec_to_pix(self, p):
        t = [self.rot[k, 0] * p[0] + self.rot[k, 1] * p[1] + self.rot[k, 2] * p[2] for k in range(3)]
        xi, eta = t[1] / t[0], t[2] / t[0]
        U, V = self.cdinv[0, 0] * xi + self.cdinv[0, 1] * eta, self.cdinv[1, 0] * xi + self.cdinv[1, 1] * eta
        u, v = U.copy(), V.copy()
        if self.order > 0:
            for _ in range(40):
                r0, r1 = u + self.sip(self.a, u, v) - U, v + self.sip(self.b, u, v) - V
                j00, j01 = 1 + self.sip(self.a, u, v, 1, 0), self.sip(self.a, u, v, 0, 1)
                j10, j11 = self.sip(self.b, u, v, 1, 0), 1 + self.sip(self.b, u, v, 0, 1)
                det = j00 * j11 - j01 * j10
                du, dv = (j11 * r0 - j01 * r1) / det, (j00 * r1 - j10 * r0) / det
                u, v = u - du, v - dv
                if np.all(np.abs(du) + np.abs(dv) <= LD(2.0) ** -60 * (np.abs(u) + np.abs(v) + 1)):
                    break
        return u + self.crpix[0], v + self.crpix[1]


# ---------------- media and surfaces ----------------
def medium_index(kind, c, wave_nm, mutate=None):
    if kind == MEDIUM_CONST:
        return np.full(len(wave_nm), LD(c[0]))
    if kind == MEDIUM_SELLMEIER:
        l2 = (wave_nm / LD(1000)) ** 2
        b0 = LD(c[0]) * (1 + LD("1e-4")) if mutate == "sellmeier" else LD(c[0])
        return np.sqrt(1 + b0 * l2 / (l2 - LD(c[3])) + LD(c[1]) * l2 / (l2 - LD(c[4])) + LD(c[2]) * l2 / (l2 - LD(c[5])))
    return 1 + air_n_minus_one(wave_nm, c[0], c[1], c[2])


class Surf:
    def __init__(self, S, F, index, mutate):
        self.kind, self.obsc_kind = int(S.kind), int(S.obsc_kind)
        self.medium_kind, self.medium_c = int(S.medium_kind), [float(v) for v in S.medium_c]
        self.z0, self.R, self.k = LD(S.z0), LD(S.R), LD(S.conic)
        self.c = 1 / self.R if S.R != 0.0 else LD(0)
        self.asph = [LD(S.asph[m]) for m in range(int(S.n_asphere))]
        if mutate == "m1_asphere" and index == 0:
            m = max(k for k, a in enumerate(self.asph) if a != 0)
            self.asph[m] = self.asph[m] * (1 + LD("1e-3"))
        self.obsc_i2, self.obsc_o2 = LD(S.obsc_inner) ** 2, LD(S.obsc_outer) ** 2
        self.obsc_i, self.obsc_o = LD(S.obsc_inner), LD(S.obsc_outer)
        self.origin, self.rot, self.fig = np.array([0, 0, self.z0], dtype=LD), None, None
        if F is not None:
            if F.moved:
                self.origin, self.rot = lds(F.origin), lds(F.rot).reshape(3, 3)
            if F.fig_deg > 0:
                self.fig = (int(F.fig_deg), LD(F.fig_inv_r), lds(F.fig))
        self.size = float(max(abs(S.z0), abs(S.R), 10.0))

    def sag(self, x, y):
        """z(x, y) of the surface about its vertex, its gradient, and the conic's radicand"""
        r2 = x * x + y * y
        rad = 1 - (1 + self.k) * self.c * self.c * r2
        root = np.sqrt(np.where(rad > 0, rad, 1))
        z = self.c * r2 / (1 + root)
        dz = self.c / root                                  # d(conic) / d(r^2) * 2 = c / root; gradient = (c / root) (x, y)
        gx, gy = dz * x, dz * y
        rp = r2
        for m, a in enumerate(self.asph):                   # a r^(2m + 4)
            gx, gy = gx + a * (2 * m + 4) * rp * x, gy + a * (2 * m + 4) * rp * y
            rp = rp * r2
            z = z + a * rp
        if self.fig is not None:
            deg, inv_r, co = self.fig
            u, v = x * inv_r, y * inv_r
            up, vp = [np.ones_like(u)], [np.ones_like(v)]
            for _ in range(deg):
                up.append(up[-1] * u)
                vp.append(vp[-1] * v)
            for p in range(deg + 1):
                for q in range(deg + 1 - p):
                    cpq = co[_abi.fig_row(p) + q]
                    if cpq == 0:
                        continue
                    z = z + cpq * up[p] * vp[q]
                    if p:
                        gx = gx + cpq * p * up[p - 1] * vp[q] * inv_r
                    if q:
                        gy = gy + cpq * q * up[p] * vp[q - 1] * inv_r
        return z, gx, gy, rad

    def vignetted(self, r2, tol):
        """(vignetted, near the edge) by the rules of include/imsim_hip.h"""
        i2, o2 = self.obsc_i2, self.obsc_o2
        k = self.obsc_kind
        near = np.zeros(len(r2), dtype=bool)
        if k == 0:
            return near.copy(), near
        if k in (1, 4):
            near |= np.abs(r2 - i2) <= tol
        near |= np.abs(r2 - o2) <= tol
        if k == 1:
            return ~((r2 >= i2) & (r2 <= o2)), near
        if k == 2:
            return ~(r2 <= o2), near
        if k == 3:
            return r2 < o2, near
        return (r2 >= i2) & (r2 < o2), near


class Optics:
    """the uploaded ims_optics_t (or ims_optics_perturbed_t) in long double"""

    def __init__(self, o, mutate=None):
        self.mutate = mutate
        self.perturbed = isinstance(o, _abi.OpticsPerturbed)
        self.img, self.field = TanSip(o.img_wcs), TanSip(o.icrf_to_field)
        self.in_kind, self.in_c = int(o.in_medium_kind), [float(v) for v in o.in_medium_c]
        self.stop_z = LD(o.stop_z)
        self.surf = [Surf(o.surf[k], o.pert.surf[k] if self.perturbed else None, k, mutate) for k in range(int(o.n_surfaces))]
        self.cam_rot, self.fp, self.sj = lds(o.cam_rot), lds(o.fp_to_pix), lds(o.slope_jac)
        self.lines = lds([list(o.lines[k]) for k in range(int(o.n_lines))]).reshape(-1, 4)
        self.circles = lds([list(o.circles[k]) for k in range(int(o.n_circles))]).reshape(-1, 3)
        self.e_z0, self.e_focal = lds(o.e_z0), lds(o.e_focal)
        self.cos_lat, self.sin_lat, self.omega = LD(o.cos_lat), LD(o.sin_lat), LD(o.omega)
        self.size = max(s.size for s in self.surf)

    # -- pixel <-> direction --
    def xy_to_field(self, x, y):
        return self.field.vec_to_pix(self.img.pix_to_vec(x, y))

    def field_to_xy(self, thx, thy):
        return self.img.vec_to_pix(self.field.pix_to_vec(thx, thy))

    # -- imsim/diffraction.py --
    def field_rotation(self, t):
        """cos, sin of field_rotation_matrix, and 1 / (|e_focal x e_z| |e_focal x e_z0|)"""
        ez = np.stack([self.cos_lat * np.cos(self.omega * t), self.cos_lat * np.sin(self.omega * t), np.full(len(t), self.sin_lat)], axis=1)
        eh = np.cross(self.e_focal[None, :], ez)
        eh0 = np.cross(self.e_focal, self.e_z0)
        nrm = np.sqrt((eh * eh).sum(axis=1)) * np.sqrt((eh0 * eh0).sum())
        return (eh * eh0[None, :]).sum(axis=1) / nrm, (ez * eh0[None, :]).sum(axis=1) / nrm, 1 / nrm

    def directed_dist(self, px, py, tie_tol):
        dl = np.stack([np.abs(np.abs(L[0] * px + L[1] * py - L[2]) - L[3]) for L in self.lines])
        dc = np.stack([np.abs(np.sqrt((px - Cc[0]) ** 2 + (py - Cc[1]) ** 2) - Cc[2]) for Cc in self.circles])
        il, ic = np.argmin(dl, axis=0), np.argmin(dc, axis=0)
        col = np.arange(len(px))
        ml, mc = dl[il, col], dc[ic, col]
        line = ml < mc
        ex, ey = self.circles[ic, 0] - px, self.circles[ic, 1] - py
        nr = np.sqrt(ex * ex + ey * ey)
        nr = np.where(nr > 0, nr, 1)
        nx, ny = np.where(line, self.lines[il, 0], ex / nr), np.where(line, self.lines[il, 1], ey / nr)
        alld = np.sort(np.concatenate([dl, dc]), axis=0)
        tie = (alld[1] - alld[0]) <= tie_tol
        return np.where(line, ml, mc), nx, ny, tie

    # -- textbook sequential trace --
    def to_pixels(self, pos, d, st):
        """cam_rot, the mm and axis swap, fp_to_pix, slope_jac; a failed ray gives zeros"""
        mutate = self.mutate
        cr, sr = self.cam_rot[0], (-self.cam_rot[1] if mutate == "cam_rot_sign" else self.cam_rot[1])
        rx, ry = cr * pos[:, 0] + sr * pos[:, 1], -sr * pos[:, 0] + cr * pos[:, 1]
        rvx, rvy = cr * d[:, 0] + sr * d[:, 1], -sr * d[:, 0] + cr * d[:, 1]
        fpx, fpy = ry * 1000, rx * 1000                                         # focal_to_pixel(ray.y * 1e3, ray.x * 1e3)
        if mutate == "fp_swap":
            fpx, fpy = fpy, fpx
        X, Y = self.fp[0] * fpx + self.fp[1] * fpy + self.fp[2], self.fp[3] * fpx + self.fp[4] * fpy + self.fp[5]
        sj = self.sj[[0, 2, 1, 3]] if mutate == "slope_jac_T" else self.sj
        A, Bs = (sj[0] * rvx + sj[1] * rvy) / d[:, 2], (sj[2] * rvx + sj[3] * rvy) / d[:, 2]
        return tuple(np.where(st == 2, 0, q) for q in (X, Y, A, Bs))

    def surface_conditioning(self, pos, d, wave_nm):
        """For every surface k but the last: the largest change of (x, y, dxdz, dydz) per metre of displacement (Kp[k]) and per
        radian of tilt (Kv[k]) of the ray as it leaves surface k, by one-sided differences of this trace over the sample rays
        (displacements along x, y, z, tilts along x, y); k = -1 is the ray at the stop.  Rays whose status changes are left out."""
        base_pos, base_d, st0 = self.trace(pos, d, wave_nm, False)[:3]
        base = self.to_pixels(base_pos, base_d, st0)
        hp, hv = LD(1e-7), LD(1e-8)
        Kp, Kv = {}, {}
        for k in range(-1, len(self.surf) - 1):
            for K, h, dirs, what in ((Kp, hp, 3, "pos"), (Kv, hv, 2, "dir")):
                worst = [LD(0)] * 4
                for axis in range(dirs):
                    e = np.zeros(3, dtype=LD)
                    e[axis] = h
                    pp, dd_, st = self.trace(pos, d, wave_nm, False, inject=(k, what, e))[:3]
                    got = self.to_pixels(pp, dd_, st)
                    ok = (st == st0) & (st0 != 2)
                    worst = [max(w, np.max(np.abs(a - c_)[ok] / h, initial=LD(0))) for w, a, c_ in zip(worst, got, base)]
                K[k] = worst
        return Kp, Kv

    def trace(self, pos, d, wave_nm, loose, inject=None):
        """pos [n][3], d unit [n][3]; returns pos, d (in the last surface's frame if perturbed), status, near-geometry, near-edge.
        inject = (k, "pos" | "dir", vector): the ray leaving surface k (-1: the stop) is displaced or tilted by it"""
        def nudge(pos, d):
            if inject[1] == "pos":
                return pos + inject[2][None, :], d
            d = d + inject[2][None, :]
            return pos, d / np.sqrt((d * d).sum(axis=1))[:, None]
        if inject is not None and inject[0] == -1:
            pos, d = nudge(pos, d)
        n = len(wave_nm)
        n_cur = medium_index(self.in_kind, self.in_c, wave_nm, self.mutate)
        fail, vig = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        near_geo, near_edge = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        tiny = LD(2.0) ** -20
        for k, S in enumerate(self.surf):
            last = k == len(self.surf) - 1
            p, v = pos - S.origin[None, :], d
            if S.rot is not None:
                p, v = p @ S.rot, d @ S.rot                                     # R^T (a - o): rows of a times R
            px, py, pz, vx, vy, vz = p[:, 0], p[:, 1], p[:, 2], v[:, 0], v[:, 1], v[:, 2]
            if S.R != 0:
                k1 = 1 + S.k
                A = S.c * (vx * vx + vy * vy + k1 * vz * vz)
                B = 2 * (S.c * (px * vx + py * vy + k1 * pz * vz) - vz)
                Cq = S.c * (px * px + py * py + k1 * pz * pz) - 2 * pz
                disc = B * B - 4 * A * Cq
                near_geo |= np.abs(disc) <= tiny * (B * B + np.abs(4 * A * Cq))
                fail |= disc < 0
                q = -(B + np.where(B < 0, -1, 1) * np.sqrt(np.where(disc > 0, disc, 0))) / 2
                t = Cq / np.where(q != 0, q, 1)
            else:
                t = -pz / vz
            rad = np.ones(n, dtype=LD)
            for _ in range(60):
                x, y, z = px + t * vx, py + t * vy, pz + t * vz
                zs, gx, gy, rad = S.sag(x, y)
                dt = (z - zs) / (vz - gx * vx - gy * vy)
                dt = np.where(fail | (rad <= 0), 0, dt)
                t = t - dt
                if np.all(np.abs(dt) <= LD(2.0) ** -62 * np.abs(t)):
                    break
            x, y, z = px + t * vx, py + t * vy, pz + t * vz
            zs, gx, gy, rad = S.sag(x, y)
            near_geo |= np.abs(rad) <= tiny
            fail |= rad <= 0
            r2 = x * x + y * y
            r = np.sqrt(r2)
            v_here, e_here = S.vignetted(r2, 2 * r * ((LD(1e-8) if loose else LD(1e-12)) + 64 * EPS * r))
            vig |= v_here & ~fail
            near_edge |= e_here & ~fail
            p = np.stack([x, y, z], axis=1)
            if S.kind in (SURF_MIRROR, SURF_REFRACT):
                nn = np.sqrt(gx * gx + gy * gy + 1)
                N = np.stack([-gx / nn, -gy / nn, 1 / nn], axis=1)
                vn = (v * N).sum(axis=1)
                if S.kind == SURF_MIRROR:
                    v = v - 2 * vn[:, None] * N
                else:
                    n2 = medium_index(S.medium_kind, S.medium_c, wave_nm, self.mutate)
                    eta = n_cur / n2
                    N = np.where((vn > 0)[:, None], -N, N)                  # against the ray
                    cosi = -(v * N).sum(axis=1)
                    kk = 1 - eta * eta * (1 - cosi * cosi)
                    near_geo |= np.abs(kk) <= tiny
                    fail |= kk < 0
                    v = eta[:, None] * v + (eta * cosi - np.sqrt(np.where(kk > 0, kk, 0)))[:, None] * N
                    n_cur = n2
                v = v / np.sqrt((v * v).sum(axis=1))[:, None]
            if self.perturbed and last:
                pos, d = p, v
            else:
                if S.rot is not None:
                    p, v = p @ S.rot.T, v @ S.rot.T
                pos, d = p + S.origin[None, :], v
            pos = np.where(fail[:, None], 0, pos)
            d = np.where(fail[:, None], np.array([0, 0, -1], dtype=LD)[None, :], d)
            if inject is not None and inject[0] == k:
                pos, d = nudge(pos, d)
        return pos, d, np.where(fail, 2, np.where(vig, 1, 0)), near_geo, near_edge & ~fail


class Result:
    """fields[f], bounds[f]: per photon; flag_geo: x, y, slopes, flux are left out; flag_flux: flux is left out; status: of the
    last tracing operator (0 ok, 1 vignetted, 2 failed; -1 where none ran)"""


def _rubin(O, kind, p, op_index, seed, o, k, f, b, loose, cond):
    """one Rubin operator on the photons of one object; f, b: dicts of the object's fields / bounds (updated in place).
    Returns status, flag_geo, flag_flux"""
    mutate = O.mutate
    n = len(k)

    def run(x, y, pu, pv, idx=slice(None)):
        wl, time, kk_, n = f["wavelength"][idx], f["time"][idx], k[idx], len(x)
        zero = np.zeros(n, dtype=bool)
        thx, thy = O.xy_to_field(x, y)
        gam = 1 / np.sqrt(1 + thx * thx + thy * thy)
        n_in = medium_index(O.in_kind, O.in_c, wl, mutate)
        v = np.stack([thx * gam, thy * gam, -gam], axis=1) / n_in[:, None]       # gnomonicToDirCos over the index
        tie, kerr = zero, np.zeros(n, dtype=LD)
        if kind != OP_OPTICS:
            slot = SLOT_OP + (op_index if mutate == "slot" else op_index >> 1)
            w = words(seed, int(o["obj_id"]), kk_, slot)
            odd = (op_index & 1) and mutate != "odd_words"
            g, _, grad = gauss_pair(w[2] if odd else w[0], w[3] if odd else w[1])
            c, s, inv_nrm = (LD(1), LD(0), LD(0))
            if not (p[1] != 0.0):
                c, s, inv_nrm = O.field_rotation(time)
            qx, qy = c * pu - s * pv, s * pu + c * pv                           # R^T pos
            pr = np.sqrt(pu * pu + pv * pv)
            dd = 32 * EPS * (pr + 1) + pr * 32 * EPS * inv_nrm + b["pupil_u"][idx] + b["pupil_v"][idx]
            dist, nx, ny, tie = O.directed_dist(qx, qy, 2 * dd)
            kw = TWO_PI / (wl * LD("1e-9"))
            arg = 1 / (2 * kw * dist)
            phi = arg if mutate == "atan" else np.arctan(arg)
            vz = -v[:, 2]
            if mutate == "no_vz":
                vz = np.ones(n, dtype=LD)
            sx, sy = g * phi * vz * nx, g * phi * vz * ny
            rx, ry = c * sx + s * sy, -s * sx + c * sy                          # R shift
            before = np.sqrt((v * v).sum(axis=1))
            v = v + np.stack([rx, ry, np.zeros(n, dtype=LD)], axis=1)
            v = v * (before / np.sqrt((v * v).sum(axis=1)))[:, None]
            dphi = arg / dist / (1 + arg * arg)
            # error of the kick as a tilt of the direction [rad]: v is 1 / n_in long
            kerr = n_in * vz * (grad * phi * DEVIATE_ERR + np.abs(g) * (phi * (8 * EPS + 32 * EPS * inv_nrm) + dphi * dd))
        if kind == OP_DIFF:
            iz = -1 / v[:, 2]
            X, Y = O.field_to_xy(v[:, 0] * iz, v[:, 1] * iz)
            return (X, Y, f["dxdz"][idx], f["dydz"][idx]), np.zeros(n, dtype=np.int64), tie, zero, kerr, None
        pos = np.stack([pu, pv, np.full(n, O.stop_z)], axis=1)
        pos, d, st, near_geo, near_edge = O.trace(pos, v / np.sqrt((v * v).sum(axis=1))[:, None], wl, loose)
        return O.to_pixels(pos, d, st), st, tie | near_geo, near_edge, kerr, d

    x, y, pu, pv = f["x"], f["y"], f["pupil_u"], f["pupil_v"]
    out, st, flag_geo, flag_edge, kerr, d_out = run(x, y, pu, pv)
    names = ("x", "y", "dxdz", "dydz")
    own = {q: np.zeros(n, dtype=LD) for q in names}
    # the reference's own central differences against the pixel position and against the pupil position, on every eighth
    # photon of the object; the largest of them stands for the object, doubled for the photons in between (the operator is
    # smooth over an object: its photons share a few pixels of the CCD)
    J = {}
    idx = np.arange(0, n, 8)
    hx, hp = LD(0.5), LD(1e-4)
    for key, (dx, dy, du, dv) in (("x", (hx, 0, 0, 0)), ("y", (0, hx, 0, 0)), ("pu", (0, 0, hp, 0)), ("pv", (0, 0, 0, hp))):
        if key in ("pu", "pv") and kind == OP_DIFF and not np.any(b["pupil_u"] > 0):
            J[key] = [np.zeros(n, dtype=LD)] * 4            # (exact pupil points: nothing to carry)
            continue
        hi, st_hi = run(x[idx] + dx, y[idx] + dy, pu[idx] + du, pv[idx] + dv, idx)[:2]
        lo, st_lo = run(x[idx] - dx, y[idx] - dy, pu[idx] - du, pv[idx] - dv, idx)[:2]
        h = 2 * (dx + dy + du + dv)
        ok = (st_hi != 2) & (st_lo != 2)
        J[key] = [np.full(n, 2 * np.max(np.abs(a - c_)[ok] / h, initial=0)) for a, c_ in zip(hi, lo)]
    # field angle [rad]: 64 roundings at the size of its operands, th itself and cd times the pixel coordinates
    thx, thy = O.xy_to_field(x, y)
    th_err = 64 * EPS * (np.abs(thx) + np.abs(thy) + LD(O.img.cdmax) * (np.abs(x) + np.abs(y) + np.abs(O.img.crpix).sum()))
    tilt = th_err + kerr
    # a tilt of delta rad is a displacement of the pixel position by at most delta / (sigma_min(cd) (1 - |grad SIP|)) px
    px_per_rad = 1 / (O.img.cdmin * (1 - O.img.sip_gradient(x, y)))
    for i, q in enumerate(names):
        k_tilt = (J["x"][i] + J["y"][i]) * px_per_rad
        own[q] = own[q] + k_tilt * tilt + J["x"][i] * b["x"] + J["y"][i] * b["y"] + J["pu"][i] * b["pupil_u"] + J["pv"][i] * b["pupil_v"]
        if kind == OP_DIFF:
            if q in ("x", "y"):
                own[q] = own[q] + 256 * EPS * (np.abs(x) + np.abs(y) + np.abs(O.img.crpix).sum())
            else:
                own[q] = b[q]
        elif loose:
            fpn = np.abs(O.fp[[0, 1, 3, 4]]).reshape(2, 2).sum(axis=1).max() * 1000
            sjn = np.abs(O.sj).reshape(2, 2).sum(axis=1).max()
            rho2 = (d_out[:, 0] ** 2 + d_out[:, 1] ** 2) / d_out[:, 2] ** 2
            # slope = (s . n_xy) / n_z of the unit direction n, each component within TRACE_DIR: (|s|_inf + |slope|) / |n_z|
            own[q] = own[q] + (TRACE_POS_M * fpn if q in ("x", "y") else TRACE_DIR * (sjn + np.abs(out[i])) * np.sqrt(1 + rho2))
        else:
            Kp, Kv = cond
            # 64 roundings per surface at the size of its operands, through the conditioning of the ray leaving that surface
            # (Optics.surface_conditioning; doubled, the sample being one ray in 128)
            own[q] = own[q] + 8 * EPS * np.abs(out[i]) + 2 * 64 * EPS * sum(
                Kp[m][i] * (LD(O.surf[m].size) if m >= 0 else LD(O.size)) + Kv[m][i] for m in Kp)
        own[q] = np.where(st == 2, 0, own[q])
    for i, q in enumerate(names):
        f[q], b[q] = out[i], own[q]
    f["flux"] = np.where(st != 0, 0, f["flux"])
    b["flux"] = np.where(st != 0, 0, b["flux"])
    return st, flag_geo, flag_edge


def apply(ops, blocks, objects, pool_in, mutate=None, loose=True):
    """ops: [(kind, table, p)] as the user gave them; blocks: dict(seed, optics, ratio_tables, ratio_wl_min, ratio_wl_step);
    objects: OBJECT_DTYPE rows; pool_in: {field: float64[n]} in pool order.  loose: the trace under test stops Newton at
    |G| <= 1e-8 (descriptor loop, unrolled layout); ignored for a perturbed descriptor, which resolves to f64."""
    n_tot = int(objects["n_phot"].sum())
    res = Result()
    res.fields = {q: lds(pool_in[q]) for q in FIELDS}
    res.bounds = {q: np.zeros(n_tot, dtype=LD) for q in FIELDS}
    res.flag_geo, res.flag_flux = np.zeros(n_tot, dtype=bool), np.zeros(n_tot, dtype=bool)
    res.status = np.full(n_tot, -1, dtype=np.int64)
    O = Optics(blocks["optics"], mutate) if blocks.get("optics") is not None and any(op[0] in (4, 5, 6) for op in ops) else None
    cond = None
    if O is not None and O.perturbed:
        loose = False
        if any(op[0] in (OP_OPTICS, OP_DIFF_OPTICS) for op in ops):
            pick = np.arange(0, n_tot, 128)                 # a sample of the planted rays: positions, pupil points, wavelengths
            sx, sy, swl = (res.fields[q][pick] for q in ("x", "y", "wavelength"))
            thx, thy = O.xy_to_field(sx, sy)
            gam = 1 / np.sqrt(1 + thx * thx + thy * thy)
            spu, spv = res.fields["pupil_u"][pick], res.fields["pupil_v"][pick]
            inside = (spu * spu + spv * spv) < 4.5 ** 2        # (not the rays planted to miss)
            pos0 = np.stack([spu, spv, np.full(len(pick), O.stop_z)], axis=1)[inside]
            d0 = np.stack([thx * gam, thy * gam, -gam], axis=1)[inside]
            cond = O.surface_conditioning(pos0, d0, swl[inside])
    seed = int(blocks["seed"])
    pos = 0
    for o in objects:
        n = int(o["n_phot"])
        sl = slice(pos, pos + n)
        pos += n
        k = int(o["phot_first"]) + np.arange(n, dtype=np.int64)
        f = {q: res.fields[q][sl] for q in FIELDS}
        b = {q: res.bounds[q][sl] for q in FIELDS}
        winv = [LD(v) for v in o["winv"]]
        if mutate == "dcr_winv_swap":
            winv[1], winv[2] = winv[2], winv[1]
        wnorm = max(abs(winv[0]) + abs(winv[1]), abs(winv[2]) + abs(winv[3]))
        faint = bool(int(o["flags"]) & OBJ_FAINT)
        for op_index, (kind, table, p) in enumerate(ops):
            p = list(p) + [0.0] * (8 - len(p))
            if kind == OP_RATIO:
                val, mag = ratio_lookup(blocks["ratio_tables"][table], blocks["ratio_wl_min"], blocks["ratio_wl_step"], f["wavelength"])
                b["flux"] = b["flux"] * np.abs(val) + 8 * EPS * np.abs(f["flux"]) * mag
                f["flux"] = f["flux"] * val
                continue
            if faint:
                continue                                    # a faint row skips every operator but BandpassRatio
            if kind in (OP_TIME, OP_PUPIL):
                w = words(seed, int(o["obj_id"]), k, SLOT_OP + (op_index >> 1))
                wa, wb = (w[2], w[3]) if op_index & 1 else (w[0], w[1])
                if kind == OP_TIME:
                    f["time"], b["time"] = LD(p[0]) + w01(wa) * LD(p[1]), np.full(n, 4 * EPS * (abs(LD(p[0])) + abs(LD(p[1]))))
                else:
                    ro2, ri2 = LD(p[0]) ** 2, LD(p[1]) ** 2
                    r = np.sqrt(ri2 + w01(wa) * (ro2 - ri2))
                    a = TWO_PI * w01(wb)
                    f["pupil_u"], f["pupil_v"] = r * np.cos(a), r * np.sin(a)
                    b["pupil_u"] = b["pupil_v"] = (SINCOS_ERR + 8 * EPS) * r
            elif kind == OP_DCR:
                r0 = refraction_r0(air_n_minus_one(f["wavelength"], p[1], p[2], p[3], mutate), mutate)
                rb = refraction_r0(air_n_minus_one(LD(p[0]), p[1], p[2], p[3], mutate), mutate)
                shift = (r0 - rb) * LD(o["dcr_tanz"]) * LD(p[4])
                du, dv = -shift * LD(o["dcr_sinp"]), shift * LD(o["dcr_cosp"])
                if mutate == "dcr_du_sign":
                    du = -du
                own = wnorm * 64 * EPS * (np.abs(r0) + abs(rb)) * abs(LD(o["dcr_tanz"]) * LD(p[4])) * (abs(LD(o["dcr_sinp"])) + abs(LD(o["dcr_cosp"])))
                if float(o["dcr_tanz"]) == 0.0:
                    own = own * 0                           # x + (+-0): the bits of x
                for q, dq in (("x", winv[0] * du + winv[1] * dv), ("y", winv[2] * du + winv[3] * dv)):
                    b[q] = b[q] + own + (8 * EPS * np.abs(f[q]) if float(o["dcr_tanz"]) != 0.0 else 0)
                    f[q] = f[q] + dq
            elif kind == OP_FOCUS:
                depth = LD(p[0])
                for q, sq in (("x", "dxdz"), ("y", "dydz")):
                    if depth != 0:
                        b[q] = b[q] + abs(depth) * b[sq] + 4 * EPS * (np.abs(f[q]) + np.abs(f[sq] * depth))
                    f[q] = f[q] + f[sq] * depth
            elif kind == OP_REFRACTION:
                a0, b0 = f["dxdz"], f["dydz"]
                f["dxdz"], f["dydz"] = snell_slopes(a0, b0, LD(p[0]))
                carried = (b["dxdz"] + b["dydz"]) / LD(p[0])          # |d out / d in| <= 1 / n for both inputs
                for q in ("dxdz", "dydz"):
                    b[q] = carried + 8 * EPS * np.abs(f[q])
            elif kind in (OP_OPTICS, OP_DIFF, OP_DIFF_OPTICS):
                st, fg, fe = _rubin(O, kind, p, op_index, seed, o, k, f, b, loose, cond)
                if kind != OP_DIFF:
                    res.status[sl] = st
                res.flag_geo[sl] |= fg
                res.flag_flux[sl] |= fe
            else:
                raise ValueError(f"operator kind {kind} is outside the chain restated here")
        b["flux"] = b["flux"] + 2 * EPS * np.abs(f["flux"])
        for q in FIELDS:
            res.fields[q][sl], res.bounds[q][sl] = f[q], b[q]
    return res


def flagged_share(res):
    return float((res.flag_geo | res.flag_flux).sum()) / max(len(res.flag_geo), 1)


def assert_matches(res, got, what, ratios=None):
    """got: {field: float64 array} of a pool (the oracle's or the renderer's) after the chain"""
    n = len(res.fields["x"])
    flagged = res.flag_geo | res.flag_flux
    assert flagged.sum() <= FLAG_CAP * n, f"{what}: {flagged.sum()} of {n} photons near a decision"
    worst = {}
    for q in FIELDS:
        value = np.asarray(got[q])
        assert value.shape == res.fields[q].shape, f"{what}: {q} has shape {value.shape}"
        assert np.all(np.isfinite(value)), f"{what}: {q} is not finite"
        keep = ~flagged if q == "flux" else (~res.flag_geo if q in ("x", "y", "dxdz", "dydz") else np.ones(n, dtype=bool))
        err = np.abs(value.astype(LD) - res.fields[q])[keep]
        bd = res.bounds[q][keep]
        ratio = np.where(err == 0, LD(0), err / np.where(bd > 0, bd, LD(1e-300)))
        worst[q] = float(ratio.max()) if ratio.size else 0.0
    traced = res.status >= 0
    if traced.any():
        st = np.where((got["flux"] == 0) & (got["x"] == 0) & (got["y"] == 0) & (got["dxdz"] == 0) & (got["dydz"] == 0), 2,
                      np.where(got["flux"] == 0, 1, 0))
        # (a photon planted with flux 0 cannot show its status; the cases plant none)
        differ = traced & ~flagged & (st != res.status)
        assert not differ.any(), f"{what}: status differs for {int(differ.sum())} photons, first {np.flatnonzero(differ)[:5]}"
    if ratios is not None:
        for q, v in worst.items():
            ratios[q] = max(ratios.get(q, 0.0), v)
    print(f"{what}: error / bound " + " ".join(f"{q}={v:.3g}" for q, v in worst.items()))
    bad = {q: v for q, v in worst.items() if not v <= 1.0}
    assert not bad, f"{what}: error exceeds the bound: {bad}"
    return worst
