"""The `opd` extra output restated in np.longdouble, independently of imsim_amd.opd, tests/opd_numpy.py, oracle/ and the kernels.

Inputs are only the uploaded optics block (optics.make_optics: an ims_optics_t or ims_optics_perturbed_t, read through the ctypes
layout of imsim_amd._abi) and the call's own numbers; everything else follows the conventions written in the docstring of
imsim_amd/opd.py and the field descriptions of ims_opd_t, ims_optics_t and ims_optics_perturbed_t (include/imsim_hip.h).  The
surface model (explicit sag, its gradient, obscuration rules) and the media are those of tests/photon_ops_ref.py.

* Rays.  nx x nx pupil points x_i = (i - (nx - 1) / 2) dx, y_j likewise, dx the binary64 value of 2 r_outer / nx, array[j, i] the
  ray (x_i, y_j, stop_z), and one chief ray from (0, 0, stop_z).  Field (u, v) -> unit direction: postel sin(r) (u, v) / r with
  r = hypot(u, v), gnomonic (u, v, 1) / norm, zemax (tan u, tan v, 1) / norm, z negated.  Starting phase n_in (d . r).
* Trace.  Surface by surface: into the surface's frame (R^T (a - o)), the conic root of smaller |t|, Newton on z - sag(x, y) to
  long-double resolution (sag = conic + even asphere + figure polynomial), obscuration by the local r^2, reflection / Snell on
  unit vectors, back to telescope coordinates (o + R a).  Every segment adds n_before x signed length, the length taken between
  the two hits in telescope coordinates, negative when the hit lies behind the ray.  The chief ray is traced like any other,
  an obscuration does not stop it.  Status: 0, 1 vignetted, 2 lost (missed conic, sag radicand <= 0, total reflection).
* Sphere.  Reference point: the chief ray's detector hit (`chief`) or the mean hit of the status-0 pixel rays (`mean`).  Back
  from the hit along the ray by s = -b - sqrt(b^2 - c) < 0, b = w . d, c = w . w - R^2, w = hit - ref; t = path + n_det s.
  OPD = (t0 - t) 1e9 nm, t0 the chief ray's t or the mean t of the status-0 rays; NaN where status != 0 or the ray misses the
  sphere, all NaN where the reference point does not exist.
* Basis.  Noll's sequence (n ascending, |m| ascending within n, the even index takes the cosine), radial polynomials by
  Gram-Schmidt of rho^|m|, rho^(|m| + 2), ... under the weight 2 rho / (1 - eps^2) on [eps, 1] in fractions.Fraction (Mahajan's
  annular polynomials), normalised to unit mean square over the annulus with sqrt 2 for m != 0, positive at rho = 1, evaluated
  in long double with cos / sin of m atan2(y, x).
* Fit.  A_pj = Z_j(pixel p) over the finite pixels of this reference's own map; A^T A and A^T w; the coefficients are the
  minimum-norm least-squares solution from a Householder QR of A followed by a one-sided Jacobi SVD, all in long double.
  Singular values below SV_CUT of the largest are zero (imsim_amd/opd.py states the same rule on A^T A); the CPU test checks
  that every case keeps its singular values clear of the cut, so the rank is never a matter of rounding.

Bounds (EPS = 2^-52 per rounding: every fma, sqrt and division of the kernels is within one unit of that), in metres until the
last step, each from the case's own numbers:

* Path.  The kernel's sum is the optical length of the polygon through its STORED hits P_k.  Against the true ray that polygon
  differs, by Fermat, at second order in any displacement of a hit along its surface, and at first order only in a hit's
  distance eta_k off its surface, by at most (n_before + n_after) eta_k.  eta_k =
    stored rounding: EPS (|x| + |y| + |z_local| + |P_z|) coaxial; 4 EPS (|x| + |y| + |z_local|) + EPS |P|_1 through frame_out;
    closed conic (no asphere, no figure): the root of A t^2 + 2 hb t + C moves by (dA t^2 + 2 dhb |t| + dC) / (2 sqrt(hb^2 - A C))
      with dA, dhb, dC 3, 4, 4 EPS of the sums of the magnitudes of their terms, plus 4 EPS |t| for sqrt, sum and quotient;
    Newton (trace_step<-1, -1, true>, surf_hit_local: stop once |dt| <= 2^-51 |t|, the step still applied, so what is left is
      the noise of G = c (r2 + k1 w^2) - 2 w): dG / (2 m), dG = 4 EPS (|c| (r2 + |k1| w^2) + 2 |w|) + 2 (1 + |c k1 w|) EPS (|w| + |z|
      + 12 sum |a_k| r^(2k+4) + 48 sum |f_pq u^p v^q|), m = 1 - k1 c w = -dG/dw / 2, plus 4 EPS |t| for the resolution of t.
  Each length: 4 EPS n |len| (three differences, the fma chain, the square root); each accumulation EPS times the running sum
  of |n len|; a Sellmeier or air index 16 EPS n |len|; the starting phase 4 EPS n_in (|d_x x| + |d_y y| + |d_z z|).
* Sphere.  n_det (4 EPS R + 4 EPS |w| + 64 K EPS |w|) (R R and the radicand round at R^2; the direction carries 64 EPS per
  surface, K surfaces, and enters through b = w . d) plus EPS |t| for the fma.  OPD: the ray's bound plus the chief ray's
  (`chief`), 2 EPS of the difference, times 1e9, plus 2 EPS |OPD|; the uploaded direction is a binary64 vector, 4 EPS per
  component, a tilt n_in 8 EPS (|x| + |y|) of the map.
* Mean reference.  A stored detector hit is off by at most 4 sum_k (16 EPS L_k + eta_k): the ray leaving surface k carries a
  direction error of 16 EPS (normal, dot product and the three fma of the bend) over the remaining geometric length L_k, and the
  surfaces after it magnify neither that nor the hit's own error by more than 4 in these telescopes.  The mean adds 20 EPS max
  |hit| (the fixed tree and the partials).  |dt / dref| <= n_det (1 + (|b| + |w|) / sqrt(b^2 - c)).  The mean of t - t_chief:
  the largest ray bound plus 20 EPS max |t - t_chief|.
* A^T A, A^T w.  A factor Z_j is off by EPS ((22 + 4) S_j + 4 D_j + (4 |m| + 3) |R_j|), S_j = sum |a_k| rho^k (Horner over the 11
  coefficients, gamma_22; 4 EPS for the table's own roundings), D_j = sum k |a_k| rho^k (rho = sqrt(fma) / r_outer: 4 EPS),
  the angle recurrence |m| steps of 4 EPS from x / r, y / r (3 EPS).  Entry (k, l): sum_p (|Z_k| dZ_l + |Z_l| dZ_k) + N EPS sum_p
  |Z_k Z_l| with N = min(npix, 4096) + chunks (the fma chain of a chunk, then the chunks in order); A^T w likewise with the
  map's own bound for dw.
* Coefficients.  |(A^T A)^+| (|d A^T w| + |d A^T A|_F |z|) + 8 cond(A^T A) EPS |z| for the binary64 solve, norms and condition from
  this reference's singular values; times 3 cond where A is rank deficient (Wedin's bound for a pseudo-inverse under a
  perturbation that keeps the rank, which the cut guarantees).  One number per field, applied to every coefficient.

Near a decision (flagged): r^2 within 2 r (1e-12 + 64 EPS r) of an obscuration edge; a conic discriminant, a sag radicand or a Snell
radicand within 2^-20 of its operands (the rules of photon_ops_ref.Optics.trace).  Flagged rays are left out of the mask and
value comparisons; tests/test_opd_ref.py checks on the reference alone that their share is at most FLAG_CAP and exactly zero
in every `mean` case and every case whose Zernike sums are compared.

Observed worst error / bound per quantity (every case of tests/opd_cases.py on an MI355X; a ratio above 1 fails the test;
records, not thresholds):

    quantity   MI355X
    map        0.0591    (`chief` cases up to 0.0591, `mean` cases up to 0.0065: their bound carries the mean hit's)
    zk_ata     0.00967
    zk_atw     0.0118
    AZ_jjj     0.015     (the rank-deficient nx = 5 grid 0.00016, the all-NaN fields exactly 0)

Mutations (`mutate=`, tests/test_opd_ref.py::test_teeth): no_phase, n_after, local_frame, s_sign, no_sqrt2, swap_projection;
each moves some case by more than its bound.
"""
from fractions import Fraction

import numpy as np

from imsim_amd import _abi                              # the struct layouts: the one import from the product
from photon_ops_ref import Surf, medium_index, lds, SURF_MIRROR, SURF_REFRACT, MEDIUM_CONST
from photon_source_ref import LD, EPS

FLAG_CAP = 1.0e-3
SV_CUT = 1.0e-5                 # singular values of A below this fraction of the largest are zero
MUTATIONS = ("no_phase", "n_after", "local_frame", "s_sign", "no_sqrt2", "swap_projection")
NAN = LD("nan")


# ---------------- rays ----------------
def field_direction(thx, thy, projection, mutate=None):
    thx, thy = LD(thx), LD(thy)
    if mutate == "swap_projection":
        projection = {"gnomonic": "zemax", "zemax": "gnomonic"}.get(projection, projection)
    if projection == "postel":
        r = np.sqrt(thx * thx + thy * thy)
        k = np.sin(r) / r if r > 0 else LD(1)
        return np.array([k * thx, k * thy, -np.cos(r)], dtype=LD)
    if projection == "gnomonic":
        v = np.array([thx, thy, LD(1)], dtype=LD)
    elif projection == "zemax":
        v = np.array([np.tan(thx), np.tan(thy), LD(1)], dtype=LD)
    else:
        raise ValueError(projection)
    v = v / np.sqrt((v * v).sum())
    v[2] = -v[2]
    return v


def grid(nx, r_outer):
    """(x [nx nx], y [nx nx], dx): the pupil points in array order, and the binary64 spacing the call carries"""
    dx = LD(np.float64(2.0 * float(r_outer)) / np.float64(nx))
    c = (np.arange(nx).astype(LD) - LD(nx - 1) / 2) * dx
    X, Y = np.meshgrid(c, c)
    return X.ravel(), Y.ravel(), dx


# ---------------- the telescope ----------------
class Tel:
    """the uploaded ims_optics_t / ims_optics_perturbed_t in long double"""

    def __init__(self, o):
        pert = isinstance(o, _abi.OpticsPerturbed)
        self.in_kind, self.in_c = int(o.in_medium_kind), [float(v) for v in o.in_medium_c]
        self.stop_z = LD(o.stop_z)
        self.surf = [Surf(o.surf[k], o.pert.surf[k] if pert else None, k, None) for k in range(int(o.n_surfaces))]
        for k, S in enumerate(self.surf):
            S.moved = bool(pert and o.pert.surf[k].moved)

    def rigidly_moved(self, G, centre):
        """this telescope turned as one body by the rotation G about `centre` (telescope coordinates)"""
        import copy
        T = copy.copy(self)
        T.surf = []
        G, centre = lds(G), lds(centre)
        for S in self.surf:
            S2 = copy.copy(S)
            R0 = S.rot if S.rot is not None else np.eye(3, dtype=LD)
            S2.origin, S2.rot, S2.moved = centre + G @ (S.origin - centre), G @ R0, True
            T.surf.append(S2)
        return T


def _fig_abs(S, x, y):
    if S.fig is None:
        return np.zeros(len(x), dtype=LD)
    deg, inv_r, co = S.fig
    u, v = np.abs(x * inv_r), np.abs(y * inv_r)
    out = np.zeros(len(x), dtype=LD)
    for p in range(deg + 1):
        for q in range(deg + 1 - p):
            c = co[_abi.fig_row(p) + q]
            if c != 0:
                out = out + abs(c) * u ** p * v ** q
    return out


class Traced:
    """hit [n, 3], d [n, 3] (telescope coordinates), path, n_det, status, near; bound: of the path; eta_sum, lever: the parts of
    the detector hit's bound"""


def trace(T, pos, d, wave_nm, mutate=None):
    n = len(pos)
    wl = np.array([wave_nm], dtype=LD)
    n_cur = medium_index(T.in_kind, T.in_c, wl)[0]
    cur_const = T.in_kind == MEDIUM_CONST
    tiny = LD(2.0) ** -20
    lost, vig, near = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    path = n_cur * (pos * d).sum(axis=1)
    bound = 4 * EPS * n_cur * np.abs(pos * d).sum(axis=1)
    if mutate == "no_phase":
        path = path * 0
    run = np.abs(path)
    lens, etas = [], []
    with np.errstate(all="ignore"):
        for S in T.surf:
            p, v = pos - S.origin[None, :], d
            if S.rot is not None:
                p, v = p @ S.rot, d @ S.rot
            px, py, pz, vx, vy, vz = p[:, 0], p[:, 1], p[:, 2], v[:, 0], v[:, 1], v[:, 2]
            k1 = 1 + S.k
            disc = np.ones(n, dtype=LD)
            if S.R != 0:
                A = S.c * (vx * vx + vy * vy + k1 * vz * vz)
                B = 2 * (S.c * (px * vx + py * vy + k1 * pz * vz) - vz)
                Cq = S.c * (px * px + py * py + k1 * pz * pz) - 2 * pz
                disc = B * B - 4 * A * Cq
                near |= np.abs(disc) <= tiny * (B * B + np.abs(4 * A * Cq))
                lost |= disc < 0
                q = -(B + np.where(B < 0, -1, 1) * np.sqrt(np.where(disc > 0, disc, 0))) / 2
                t = Cq / np.where(q != 0, q, 1)
            else:
                t = -pz / vz
            t = np.where(lost, 0, t)
            for _ in range(40):
                x, y, z = px + t * vx, py + t * vy, pz + t * vz
                zs, gx, gy, rad = S.sag(x, y)
                dt = (z - zs) / (vz - gx * vx - gy * vy)
                dt = np.where(lost | (rad <= 0) | ~np.isfinite(dt), 0, dt)
                t = t - dt
                if np.all(np.abs(dt) <= LD(2.0) ** -58 * np.abs(t)):
                    break
            x, y = px + t * vx, py + t * vy
            zs, gx, gy, rad = S.sag(x, y)
            near |= (np.abs(rad) <= tiny) & ~lost
            lost |= rad <= 0
            r2 = x * x + y * y
            r = np.sqrt(r2)
            v_here, e_here = S.vignetted(r2, 2 * r * (LD(1e-12) + 64 * EPS * r))
            vig |= v_here & ~lost
            near |= e_here & ~lost
            loc = np.stack([x, y, zs], axis=1)
            n_next, next_const = n_cur, cur_const
            if S.kind in (SURF_MIRROR, SURF_REFRACT):
                nn = np.sqrt(gx * gx + gy * gy + 1)
                N = np.stack([-gx / nn, -gy / nn, 1 / nn], axis=1)
                vn = (v * N).sum(axis=1)
                if S.kind == SURF_MIRROR:
                    v = v - 2 * vn[:, None] * N
                else:
                    n_next = medium_index(S.medium_kind, S.medium_c, wl)[0]
                    next_const = S.medium_kind == MEDIUM_CONST
                    eta_ = n_cur / n_next
                    N = np.where((vn > 0)[:, None], -N, N)
                    cosi = -(v * N).sum(axis=1)
                    kk = 1 - eta_ * eta_ * (1 - cosi * cosi)
                    near |= (np.abs(kk) <= tiny) & ~lost
                    lost |= kk < 0
                    v = eta_ * v + (eta_ * cosi - np.sqrt(np.where(kk > 0, kk, 0)))[:, None] * N
                v = v / np.sqrt((v * v).sum(axis=1))[:, None]
            new, vout = loc, v
            if S.rot is not None:
                vout = v @ S.rot.T
                if mutate != "local_frame":
                    new = loc @ S.rot.T
            new = new + S.origin[None, :]
            step = new - pos
            ln = np.sqrt((step * step).sum(axis=1)) * np.where((step * d).sum(axis=1) < 0, -1, 1)
            n_seg = n_next if mutate == "n_after" else n_cur
            path = path + n_seg * ln
            # ---- the bound of this surface (module docstring) ----
            ax, ay, az = np.abs(x), np.abs(y), np.abs(zs)
            if S.moved:
                store = EPS * (4 * (ax + ay + az) + np.abs(new).sum(axis=1))
            else:
                store = EPS * (ax + ay + az + np.abs(new[:, 2]))
            if S.asph or S.fig is not None:
                w = S.c * r2 / (1 + np.sqrt(np.where(rad > 0, rad, 1)))
                rp, pabs = r2, np.zeros(n, dtype=LD)
                for a in S.asph:
                    rp = rp * r2
                    pabs = pabs + abs(a) * rp
                dG = (4 * EPS * (abs(S.c) * (r2 + abs(k1) * w * w) + 2 * np.abs(w))
                      + 2 * (1 + np.abs(S.c * k1 * w)) * EPS * (np.abs(w) + az + 12 * pabs + 48 * _fig_abs(S, x, y)))
                eta = dG / (2 * (1 - k1 * S.c * w)) + 4 * EPS * np.abs(t)
            elif S.R != 0:
                aR = abs(S.R)
                dA = 3 * EPS * (vx * vx + vy * vy + abs(k1) * vz * vz)
                dhb = 4 * EPS * (np.abs(px * vx) + np.abs(py * vy) + np.abs(k1 * vz * pz) + aR * np.abs(vz))
                dC = 4 * EPS * (px * px + py * py + np.abs(pz) * (np.abs(k1 * pz) + 2 * aR))
                sqK = aR * np.sqrt(np.where(disc > 0, disc, 1)) / 2
                eta = (dA * t * t + 2 * dhb * np.abs(t) + dC) / (2 * sqK) + 4 * EPS * np.abs(t)
            else:
                eta = np.zeros(n, dtype=LD)
            eta = eta + store
            run = run + np.abs(n_seg * ln)
            bound = bound + (n_cur + n_next) * eta + 4 * EPS * n_cur * np.abs(ln) + EPS * run
            if not cur_const:
                bound = bound + 16 * EPS * n_cur * np.abs(ln)
            lens.append(np.abs(ln))
            etas.append(eta)
            n_cur, cur_const = n_next, next_const
            pos = np.where(lost[:, None], 0, new)
            d = np.where(lost[:, None], np.array([0, 0, -1], dtype=LD)[None, :], vout)
    out = Traced()
    out.hit, out.d, out.path, out.n_det = pos, d, path, n_cur
    out.status = np.where(lost, 2, np.where(vig, 1, 0))
    out.near = near
    out.bound = bound
    rem = np.zeros(n, dtype=LD)
    hit_bound = np.zeros(n, dtype=LD)
    for ln, eta in zip(reversed(lens), reversed(etas)):         # surface k: L_k = the lengths after it
        hit_bound = hit_bound + 4 * (16 * EPS * rem + eta)
        rem = rem + ln
    out.hit_bound = hit_bound + 4 * 16 * EPS * rem              # (the ray as it leaves the stop)
    out.n_surf = len(T.surf)
    return out


# ---------------- sphere and map ----------------
def _sphere(tr, ref, R, mutate):
    """t on the reference sphere about `ref`, its bound, and |dt / dref|"""
    w = tr.hit - ref[None, :]
    b = (w * tr.d).sum(axis=1)
    c = (w * w).sum(axis=1) - R * R
    disc = b * b - c
    with np.errstate(all="ignore"):
        sq = np.sqrt(np.where(disc >= 0, disc, NAN))
        s = -b + sq if mutate == "s_sign" else -b - sq
        t = tr.path + tr.n_det * s
        wn = np.sqrt((w * w).sum(axis=1))
        bound = tr.bound + tr.n_det * (4 * EPS * R + 4 * EPS * wn + 64 * tr.n_surf * EPS * wn) + EPS * np.abs(t)
        dref = tr.n_det * (1 + (np.abs(b) + wn) / sq)
    t = np.where(tr.status == 2, NAN, t)
    return t, bound, dref


class Field:
    """one field: opd [nx, nx] (nm, NaN), bound [nx, nx], flagged [nx, nx], status [nx, nx]"""


def opd_field(T, d, nx, r_outer, wave_nm, R, reference, mutate=None):
    X, Y, dx = grid(nx, r_outer)
    npix = nx * nx
    pos = np.stack([np.append(X, LD(0)), np.append(Y, LD(0)), np.full(npix + 1, T.stop_z)], axis=1)
    n_in = medium_index(T.in_kind, T.in_c, np.array([wave_nm], dtype=LD))[0]
    tr = trace(T, pos, np.tile(d[None, :], (npix + 1, 1)), LD(wave_nm), mutate)
    R = LD(R)
    good = tr.status[:npix] == 0
    F = Field()
    F.status, F.flagged = tr.status[:npix].reshape(nx, nx), tr.near[:npix].reshape(nx, nx)
    F.chief_status, F.chief_near = int(tr.status[npix]), bool(tr.near[npix])
    nan_map = np.full(npix, NAN)
    F.opd, F.bound = nan_map.reshape(nx, nx), np.zeros((nx, nx), dtype=LD)
    tilt = n_in * 8 * EPS * (np.abs(X) + np.abs(Y))
    if reference == "chief":
        if tr.status[npix] == 2:
            return F
        t, bt, _ = _sphere(tr, tr.hit[npix], R, mutate)
        off = t[npix] - t[:npix]
        b = bt[:npix] + bt[npix] + 2 * EPS * np.abs(off)
    else:
        if not good.any():
            return F
        hits = tr.hit[:npix][good]
        ref = hits.sum(axis=0) / good.sum()
        ref_bound = tr.hit_bound[:npix][good].max() + 20 * EPS * np.abs(hits).max()
        t, bt, dref = _sphere(tr, ref, R, mutate)
        bt = bt + dref * ref_bound
        fin = good & np.isfinite(t[:npix])
        # the kernel averages t - t_chief; the chief ray's value is common to both terms and leaves the difference
        tc = t[npix] if np.isfinite(t[npix]) else LD(0)
        v = t[:npix] - tc
        t0 = v[fin].sum() / fin.sum()
        off = t0 - v
        b = bt[:npix] + bt[:npix][fin].max() + 20 * EPS * np.abs(v[fin]).max() + 2 * EPS * (np.abs(off) + np.abs(v))
    opd = np.where(good, off, NAN) * LD(1e9)
    with np.errstate(all="ignore"):
        F.opd = opd.reshape(nx, nx)
        F.bound = np.where(np.isfinite(opd), (b + tilt) * LD(1e9) + 2 * EPS * np.abs(opd), 0).reshape(nx, nx)
    return F


# ---------------- annular Zernikes ----------------
def noll_sequence(jmax):
    """[(n, m)] of j = 1 .. jmax: m > 0 the cosine term, m < 0 the sine term"""
    out = []
    n = 0
    while len(out) < jmax:
        for am in range(n % 2, n + 1, 2):
            if am == 0:
                out.append((n, 0))
            else:
                j = len(out) + 1                                # the even index of the pair is the cosine
                out += [(n, am), (n, -am)] if j % 2 == 0 else [(n, -am), (n, am)]
        n += 1
    return out[:jmax]


def _frac_to_ld(f):
    hi = float(f)
    return LD(hi) + LD(float(f - Fraction(hi)))


def radial_polynomials(n_max, eps):
    """{(n, |m|): long-double coefficients of rho^0 .. rho^n}, unit mean square of R over the annulus, R(1) > 0"""
    e2 = Fraction(float(eps)) ** 2

    def moment(k):                                              # mean of rho^k over the annulus, k even
        return (1 - e2 ** (k // 2 + 1)) / ((k // 2 + 1) * (1 - e2))

    def dot(a, b):
        return sum(ca * cb * moment(pa + pb) for pa, ca in a.items() for pb, cb in b.items())

    out = {}
    for m in range(n_max + 1):
        done = []
        for n in range(m, n_max + 1, 2):
            p = {n: Fraction(1)}
            for q, qq in done:
                c = dot({n: Fraction(1)}, q) / qq
                for k, val in q.items():
                    p[k] = p.get(k, Fraction(0)) - c * val
            pp = dot(p, p)
            done.append((p, pp))
            s = -1 if sum(p.values()) < 0 else 1
            norm = np.sqrt(_frac_to_ld(pp))
            co = np.zeros(n + 1, dtype=LD)
            for k, val in p.items():
                co[k] = s * _frac_to_ld(val) / norm
            out[(n, m)] = co
    return out


class Basis:
    def __init__(self, jmax, eps, mutate=None):
        self.nm = noll_sequence(jmax)
        self.rad = radial_polynomials(max(n for n, _ in self.nm), eps)
        self.root2 = LD(1) if mutate == "no_sqrt2" else np.sqrt(LD(2))

    def __call__(self, x, y, r_outer):
        """Z [n_points, jmax] and its per-point bound dZ (module docstring)"""
        rho = np.sqrt(x * x + y * y) / LD(r_outer)
        th = np.arctan2(y, x)
        Z, dZ = np.empty((len(x), len(self.nm)), dtype=LD), np.empty((len(x), len(self.nm)), dtype=LD)
        for j, (n, m) in enumerate(self.nm):
            co = self.rad[(n, abs(m))] * (self.root2 if m else LD(1))
            val, S, D = np.zeros(len(x), dtype=LD), np.zeros(len(x), dtype=LD), np.zeros(len(x), dtype=LD)
            rp = np.ones(len(x), dtype=LD)
            for k, a in enumerate(co):
                val, S, D = val + a * rp, S + abs(a) * rp, D + k * abs(a) * rp
                rp = rp * rho
            ang = np.cos(m * th) if m > 0 else np.sin(-m * th) if m < 0 else np.ones(len(x), dtype=LD)
            Z[:, j] = val * ang
            dZ[:, j] = EPS * (26 * S + 4 * D + (4 * abs(m) + 3) * np.abs(val))
        return Z, dZ


# ---------------- long-double least squares ----------------
def householder_r(A, b):
    """R [J, J] and the first J entries of Q^T b, for A [N, J] with N >= J"""
    A, b = A.copy(), b.copy()
    N, J = A.shape
    for k in range(J):
        x = A[k:, k]
        nx_ = np.sqrt((x * x).sum())
        if nx_ == 0:
            continue
        v = x.copy()
        v[0] = v[0] + (nx_ if x[0] >= 0 else -nx_)
        vv = (v * v).sum()
        A[k:, k:] = A[k:, k:] - np.outer(v, (2 / vv) * (v @ A[k:, k:]))
        b[k:] = b[k:] - v * ((2 / vv) * (v @ b[k:]))
    return np.triu(A[:J]), b[:J]


def jacobi_svd(M):
    """one-sided Jacobi: M V = W with orthogonal columns; returns (W, V, s) with s the column norms of W"""
    W = M.copy()
    J = M.shape[1]
    V = np.eye(J, dtype=LD)
    floor = (W * W).sum() * LD(2.0) ** -120
    for _ in range(60):
        moved = False
        for p in range(J - 1):
            for q in range(p + 1, J):
                a, b_, g = (W[:, p] * W[:, p]).sum(), (W[:, q] * W[:, q]).sum(), (W[:, p] * W[:, q]).sum()
                if abs(g) <= LD(2.0) ** -61 * np.sqrt(a * b_) + floor:
                    continue
                moved = True
                z = (b_ - a) / (2 * g)
                t = (1 if z >= 0 else -1) / (abs(z) + np.sqrt(1 + z * z))
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                W[:, p], W[:, q] = c * W[:, p] - s * W[:, q], s * W[:, p] + c * W[:, q]
                V[:, p], V[:, q] = c * V[:, p] - s * V[:, q], s * V[:, p] + c * V[:, q]
        if not moved:
            break
    return W, V, np.sqrt((W * W).sum(axis=0))


def lstsq_min_norm(A, b):
    """(z, singular values of A): the minimum-norm least-squares solution, singular values below SV_CUT of the largest zero"""
    N, J = A.shape
    if N == 0:
        return np.zeros(J, dtype=LD), np.zeros(J, dtype=LD)
    M, rhs = householder_r(A, b) if N > J else (A, b)
    W, V, s = jacobi_svd(M)
    keep = s > LD(SV_CUT) * s.max()
    coef = np.where(keep, (W.T @ rhs) / np.where(keep, s * s, 1), 0)
    return V @ coef, s


class Fit:
    """ata [J, J], atw [J], their bounds d_ata, d_atw, zk [J], zk_bound (scalar), sv (singular values of A), n_finite"""


def fit(F, nx, r_outer, eps, jmax, mutate=None, basis=None):
    X, Y, _ = grid(nx, r_outer)
    w_all, bw_all = F.opd.ravel(), F.bound.ravel()
    fin = np.isfinite(w_all)
    basis = basis or Basis(jmax, eps, mutate)
    Z, dZ = basis(X[fin], Y[fin], r_outer)
    w, bw = w_all[fin], bw_all[fin]
    out = Fit()
    out.n_finite = int(fin.sum())
    npix = nx * nx
    nacc = (min(npix, 4096) + (npix + 4095) // 4096) * EPS
    aZ = np.abs(Z)
    out.ata, out.atw = Z.T @ Z, Z.T @ w
    cross = aZ.T @ dZ
    out.d_ata = cross + cross.T + nacc * (aZ.T @ aZ)
    out.d_atw = aZ.T @ bw + dZ.T @ np.abs(w) + nacc * (aZ.T @ np.abs(w))
    out.zk, out.sv = lstsq_min_norm(Z, w)
    live = out.sv[out.sv > LD(SV_CUT) * out.sv.max()] if out.n_finite else np.zeros(0, dtype=LD)
    out.rank = len(live)
    if out.rank == 0:
        out.zk_bound = LD(0)
        return out
    inv, cond = 1 / live.min() ** 2, (live.max() / live.min()) ** 2
    zn = np.sqrt((out.zk * out.zk).sum())
    b = inv * (np.sqrt((out.d_atw ** 2).sum()) + np.sqrt((out.d_ata ** 2).sum()) * zn) + 8 * cond * EPS * zn
    out.zk_bound = b * (3 * cond if out.rank < jmax else 1)
    return out


# ---------------- a whole call ----------------
class Result:
    """fields [Field], fits [Fit or None]"""


def compute(o, fields, wave_nm, nx, r_outer, projection, sphere_radius, reference, eps, jmax, mutate=None, do_fit=True):
    T = Tel(o)
    res = Result()
    res.dirs = [field_direction(a, b, projection, mutate) for a, b in fields]
    res.fields = [opd_field(T, d, nx, r_outer, wave_nm, sphere_radius, reference, mutate) for d in res.dirs]
    basis = Basis(jmax, eps, mutate) if do_fit and jmax > 0 else None
    res.fits = [fit(F, nx, r_outer, eps, jmax, mutate, basis) if basis else None for F in res.fields]
    return res


def flagged_share(res):
    tot = sum(F.flagged.size + 1 for F in res.fields)
    return (sum(int(F.flagged.sum()) + int(F.chief_near) for F in res.fields)) / tot


def ratio(got, want, bound):
    """max |got - want| / bound over the entries (0 where they agree exactly)"""
    err = np.abs(np.asarray(got).astype(LD) - want)
    bound = np.broadcast_to(np.asarray(bound, dtype=LD), err.shape)
    r = np.where(err == 0, LD(0), err / np.where(bound > 0, bound, LD(1e-300)))
    return float(r.max()) if r.size else 0.0
