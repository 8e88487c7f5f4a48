"""The photon source restated in plain numpy, independently of oracle/, the kernels and imsim_amd's samplers.

"Photon source" = everything that makes a photon before the operator chain sees it: the wavelength draw, the profile sample
(radial table, box, knots, FITS stamp) and the PSF kicks (Gaussian, double Gaussian, radial table, chromatic scaling,
phase-screen gradient).  Inputs are only the data the product uploads (object rows, Scene.psf tuples, the radial / SED / image
tables, the screens and the fields of atmosphere_struct()) and the written spec.  After the integer words of
Philox4x32-10 everything is np.longdouble with libm's logl / cosl / sinl / powl; the periodic wrap is Python's % on int64;
the bins of every table are chosen by exact comparisons (np.searchsorted on the table's own doubles).

Nothing here is taken from the kernels' or the oracle's output: `shoot` returns, next to every field, a per-photon bound
computed from the case's own numbers.

Bounds (spec v6, asserted by tests/test_oracle_math.py: sin / cos of a word within 1.5e-11, log of a word within 2.5e-12 relative):

* x, y:  |winv|_inf * sum over the sampled stages of (stage scale) * (radius drawn) * 1.7e-11  (1.5e-11 from sin / cos, plus
  half the log's 2.5e-12 for a Gaussian radius sqrt(-2 ln u)), plus 64 * 2^-52 * (|x0| + the sum of the magnitudes of the
  products that are added up): the roundings happen at the size of the operands, not of the result that may cancel.
  A chromatic stage adds its magnitude * (4e-15 * (1 + |alpha ln(wl / base)|) + |alpha| * 8 * 2^-52), the second term being
  the wavelength's own bound passed through (wl / base)^alpha.
  The x offset of a quintic image profile is drawn from the in-pixel fraction f, a computed double with relative error 2^-52:
  through the inverse cumulative |K| it moves the offset by f * 2^-51 * (kx[i + 1] - kx[i]) / (kcdf[i + 1] - kcdf[i]) of the
  bin i it falls in (the slope is large where |K| is small); that term is added for those photons.
  Table and box stages add only ulps: r2 = a + f (b - a) with 0 <= a <= b has relative error <= 2^-50, its root half of that.
* wavelength: 8 * 2^-52 * max(|v[i]|, |v[i + 1]|) (three roundings of the linear interpolation).
* pupil_u, pupil_v: (1.5e-11 + 8 * 2^-52) * r.   time: 4 * 2^-52 * (|t0| + exptime).   flux: 2 * 2^-52 * |flux|.
* screen gradient, per component: inv_scale * sum over layers of
      4 max|S_l| * 2^-50 * (1 + max|fx|)      f64 roundings of the sums and of the cell fraction at the largest coordinate seen
    + M_l * 1.5e-11 * r_outer * inv_scale     M_l = the largest mixed second difference |S11 - S10 - S01 + S00| of layer l:
  the second term is not in the first statement of the bound and is derived here: the gradient is taken AT the pupil point, which
  the kernel forms with the spec's series (r cos, r sin within 1.5e-11 r_outer metres = 1.5e-11 r_outer inv_scale cells), and
  inside a cell d(gx)/d(ay) = d(gy)/d(ax) = S11 - S10 - S01 + S00.  The same displacement (6.3e-10 cells for the 4.18 m pupil) is
  why photons within 1e-9 cells of a cell edge (this module's own distance) are left out of the gradient and x, y comparisons:
  there the gradient jumps.  Nothing else is left out, and the share is capped at 1e-4 of a case's photons.

Observed worst error / bound per field (every case of tests/photon_source_cases.py; a ratio above 1 fails the test):

    field        oracle (CPU)   MI355X
    x            0.363          0.363
    y            0.369          0.369
    flux         0              0
    wavelength   0.058          0.058
    pupil_u      0.461          0.462
    pupil_v      0.462          0.462
    time         0              0
    kick         -              0.0265

(kick: the gradients the phase-screen pre-pass stores; the oracle keeps no such array, its gradients are checked through x, y.)
"""
import numpy as np

LD = np.longdouble
U64 = np.uint64
M32 = U64(0xFFFFFFFF)
EPS = LD(2.0) ** -52
TWO_PI = 2 * np.arctan2(LD(0), LD(-1))
SINCOS_ERR, DEVIATE_ERR, EDGE = LD(1.5e-11), LD(1.7e-11), 1.0e-9
SLOT_SHOOT, SLOT_KNOT, SLOT_PSF, SLOT_PSF_TIME = 0, 1, 2, 20
PSF_GAUSSIAN, PSF_RADIAL, PSF_SCREENS, PSF_DOUBLE_GAUSSIAN = 1, 2, 3, 4
PROF_POINT, PROF_BOX, PROF_KNOTS, PROF_IMAGE = -1, -2, -3, -4
FIELDS = ("x", "y", "flux", "wavelength", "pupil_u", "pupil_v", "time")


# ---------------- Philox4x32-10 (Salmon et al. 2011) in integer arithmetic ----------------
def philox4x32_10(ctr, key):
    """ctr: four, key: two arrays (or ints) of 32-bit values; returns the four output words as uint64 arrays"""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=U64)) & M32 for c in ctr)
    k0, k1 = (np.atleast_1d(np.asarray(k, dtype=U64)) & M32 for k in key)
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c0, U64(0xCD9E8D57) * c2           # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> U64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + U64(0x9E3779B9)) & M32, (k1 + U64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def words(seed, obj_id, photon, slot):
    """the block of (seed, object, photon, slot): counter = (photon lo, photon hi, slot, obj_id lo), key = (seed lo,
    seed hi ^ obj_id hi)"""
    photon = np.atleast_1d(np.asarray(photon, dtype=np.int64)).astype(U64)
    seed, obj_id = int(seed) & (2 ** 64 - 1), int(obj_id) & (2 ** 64 - 1)
    n = len(photon)
    return philox4x32_10((photon & M32, photon >> U64(32), np.full(n, slot, dtype=U64), np.full(n, obj_id & 0xFFFFFFFF, dtype=U64)),
                         (np.full(n, seed & 0xFFFFFFFF, dtype=U64), np.full(n, (seed >> 32) ^ (obj_id >> 32), dtype=U64)))


def w01(w):
    """(w + 1/2) / 2^32"""
    return (w.astype(LD) + LD(0.5)) / LD(2.0 ** 32)


def gauss_pair(w0, w1):
    """sqrt(-2 ln u0) (cos, sin)(2 pi u1); also the radius"""
    r = np.sqrt(-2 * np.log(w01(w0)))
    a = TWO_PI * w01(w1)
    return r * np.cos(a), r * np.sin(a), r


# ---------------- table samplers ----------------
def table_bin(cdf, u, exact=True):
    """largest i in [0, len(cdf) - 2] with cdf[i] <= u.  exact: u is a deviate of the spec, an exact double, and so are the
    knots -- the comparison is the kernel's.  (Not exact: the in-pixel fraction that the quintic interpolant's x offset is drawn
    from, a computed number; its table is continuous, so a neighbouring bin at a knot gives the same offset.)"""
    if not exact:
        return np.clip(np.searchsorted(np.asarray(cdf).astype(LD), u, side="right") - 1, 0, len(cdf) - 2)
    uu = np.asarray(u).astype(np.float64)
    assert np.all(uu.astype(LD) == u), "a deviate of the spec is an exact double"
    return np.clip(np.searchsorted(cdf, uu, side="right") - 1, 0, len(cdf) - 2)


def inverse_cdf(cdf, val, u, exact=True):
    """val at the inverse of the piecewise linear cdf; a bin of no width gives its lower knot.  Returns (value, bin, fraction)"""
    i = table_bin(cdf, u, exact)
    c0, wd = cdf[i].astype(LD), cdf[i + 1].astype(LD) - cdf[i].astype(LD)
    f = np.where(wd > 0, (u - c0) / np.where(wd > 0, wd, 1), LD(0))
    a = val[i].astype(LD)
    return a + f * (val[i + 1].astype(LD) - a), i, f


def radial_r2(r2, cdf, u):
    """r^2 of a radial table: uniform surface density per annulus = linear in r^2 inside a bin"""
    return inverse_cdf(cdf, r2, u)[0]


def lin_lookup(v, u):
    """linear table over u in [0, 1] on len(v) equidistant points; returns (value, bound)"""
    n = len(v)
    f = u * (n - 1)
    i = np.clip(np.floor(f).astype(np.int64), 0, n - 2)
    a = f - i
    lo, hi = v[i].astype(LD), v[i + 1].astype(LD)
    return lo + a * (hi - lo), 8 * EPS * np.maximum(np.abs(lo), np.abs(hi))


def image_nearest(cdf, w, h, u, u2):
    """pixel by the image's cumulative distribution, uniform inside it; position in pixels from the image centre"""
    i = table_bin(cdf, u)
    c0, wd = cdf[i].astype(LD), cdf[i + 1].astype(LD) - cdf[i].astype(LD)
    f = np.where(wd > 0, (u - c0) / np.where(wd > 0, wd, 1), LD(0))
    return (i % w) + f - LD(w) / 2, (i // w) + u2 - LD(h) / 2, i, f


def interp_offset(kx, kcdf, neg, u, exact=True):
    """offset drawn from |K| of the interpolant, and whether K is negative there; also the slope d(offset) / du of its bin"""
    d, i, _ = inverse_cdf(kcdf, kx, u, exact)
    ad = np.abs(d)
    negative = ((ad > neg[0]) & (ad < neg[1])) | ((ad > neg[2]) & (ad < neg[3]))
    wd = kcdf[i + 1].astype(LD) - kcdf[i].astype(LD)
    slope = np.where(wd > 0, (kx[i + 1].astype(LD) - kx[i].astype(LD)) / np.where(wd > 0, wd, 1), LD(0))
    return d, negative, slope


# ---------------- phase screens ----------------
class Atmosphere:
    """the fields of atmosphere_struct() and the screens [n_layers][npix][npix]"""

    def __init__(self, A, screens):
        self.n_layers, self.npix = int(A.n_layers), int(A.npix)
        self.scale, self.x0, self.t0, self.exptime = (LD(v) for v in (A.scale, A.x0, A.t0, A.exptime))
        self.r_outer, self.r_inner = LD(A.aper_r_outer), LD(A.aper_r_inner)
        self.vx = [LD(A.vx[l]) for l in range(self.n_layers)]
        self.vy = [LD(A.vy[l]) for l in range(self.n_layers)]
        self.alt = [LD(A.alt[l]) for l in range(self.n_layers)]
        s = np.asarray(screens.cpu().numpy() if hasattr(screens, "cpu") else screens)
        assert s.dtype == np.float32 and s.shape == (self.n_layers, self.npix, self.npix)
        self.screens = s
        d = s.astype(np.float64)
        self.smax = [float(np.abs(d[l]).max()) for l in range(self.n_layers)]
        mixed = np.roll(d, (-1, -1), (1, 2)) - np.roll(d, -1, 1) - np.roll(d, -1, 2) + d
        self.mixed = [float(np.abs(mixed[l]).max()) for l in range(self.n_layers)]
        self.max_fx = 0.0                                         # the largest |coordinate in cells| any photon had

    def gradient(self, pu, pv, t, tanx, tany):
        """sum over the layers, in order, of the gradient of the periodic bilinear interpolant at (p - t v + alt tan) [nm / m];
        also the distance (in cells) of each photon to the nearest cell edge over layers and axes"""
        n = self.npix
        sx, sy = np.zeros(len(pu), dtype=LD), np.zeros(len(pu), dtype=LD)
        edge = np.full(len(pu), np.inf)
        for l in range(self.n_layers):
            fx = (pu - t * self.vx[l] + self.alt[l] * LD(tanx) - self.x0) / self.scale
            fy = (pv - t * self.vy[l] + self.alt[l] * LD(tany) - self.x0) / self.scale
            flx, fly = np.floor(fx), np.floor(fy)
            ax, ay = fx - flx, fy - fly
            ix, iy = flx.astype(np.int64) % n, fly.astype(np.int64) % n
            ix1, iy1 = (ix + 1) % n, (iy + 1) % n
            S = self.screens[l]
            f00, f10, f01, f11 = (S[iy, ix].astype(LD), S[iy, ix1].astype(LD), S[iy1, ix].astype(LD), S[iy1, ix1].astype(LD))
            sx = sx + ((f10 - f00) * (1 - ay) + (f11 - f01) * ay)
            sy = sy + ((f01 - f00) * (1 - ax) + (f11 - f10) * ax)
            for a in (ax, ay):
                edge = np.minimum(edge, np.minimum(a, 1 - a).astype(np.float64))
            if len(pu):
                self.max_fx = max(self.max_fx, float(np.abs(fx).max()), float(np.abs(fy).max()))
        return sx / self.scale, sy / self.scale, edge

    def gradient_bound(self):
        """per component of the gradient; call after every photon of the case went through `gradient` (max_fx)"""
        inv_scale = 1 / self.scale
        dp = SINCOS_ERR * self.r_outer * inv_scale
        return inv_scale * sum(4 * LD(self.smax[l]) * LD(2.0) ** -50 * (1 + LD(self.max_fx)) + LD(self.mixed[l]) * dp
                               for l in range(self.n_layers))


# ---------------- the source ----------------
class Source:
    """What the product uploads for a scene.  image_cdfs: the cumulative distributions of scene.image_profiles as uploaded
    (w * h + 1 knots each); interp: None for the nearest interpolant, or (kx, kcdf, norm, neg) of the quintic one."""

    def __init__(self, scene, image_cdfs=(), interp=None):
        self.seed = int(scene.seed)
        self.psf = [tuple(c) + (0.0,) * (7 - len(c)) for c in scene.psf]       # (kind, table, p0, chrom_alpha, chrom_base, p1, p2)
        self.r2 = None if scene.radial_r2 is None else np.atleast_2d(np.asarray(scene.radial_r2, dtype=np.float64))
        self.cdf = None if scene.radial_cdf is None else np.atleast_2d(np.asarray(scene.radial_cdf, dtype=np.float64))
        self.sed = None if scene.sed_tables is None else np.atleast_2d(np.asarray(scene.sed_tables, dtype=np.float64))
        self.image_cdfs = [np.asarray(c, dtype=np.float64) for c in image_cdfs]
        self.image_sizes = [(im.shape[1], im.shape[0]) for im in (scene.image_profiles or [])]
        self.interp = interp
        self.atm = None if scene.atm is None else Atmosphere(scene.atm.atmosphere_struct(), scene.atm.screens)


class Shot:
    """fields[f], bounds[f]: per photon, np.longdouble, in pool order; kick, kick_bound: the screen gradient [n][2] and its
    bound (None without a screen component); edge: distance to the nearest cell edge; near_edge = edge < 1e-9"""


def shoot(src, objects):
    """every photon of the object rows, in pool order (object after object, photon phot_first + j at offset + j)"""
    n_tot = int(objects["n_phot"].sum())
    out = Shot()
    out.fields = {f: np.zeros(n_tot, dtype=LD) for f in FIELDS}
    out.bounds = {f: np.zeros(n_tot, dtype=LD) for f in FIELDS}
    has_screens = any(int(c[0]) == PSF_SCREENS for c in src.psf)
    out.kick = np.zeros((n_tot, 2), dtype=LD) if has_screens else None
    out.edge = np.full(n_tot, np.inf)
    screen_terms = []                                   # (slice, |winv|, scale magnitude): bound filled in when max_fx is known
    pos = 0
    for o in objects:
        n = int(o["n_phot"])
        sl = slice(pos, pos + n)
        pos += n
        k = int(o["phot_first"]) + np.arange(n, dtype=np.int64)
        oid = int(o["obj_id"])
        jac, winv = [LD(v) for v in o["jac"]], [LD(v) for v in o["winv"]]
        wnorm = max(abs(winv[0]) + abs(winv[1]), abs(winv[2]) + abs(winv[3]))
        jnorm = max(abs(jac[0]) + abs(jac[1]), abs(jac[2]) + abs(jac[3]))
        ps, aux, pt = LD(o["prof_scale"]), LD(o["prof_aux"]), int(o["prof_table"])
        w = words(src.seed, oid, k, SLOT_SHOOT)
        # wavelength
        if int(o["sed_table"]) >= 0:
            wl, wl_bound = lin_lookup(src.sed[int(o["sed_table"])], w01(w[0]))
        else:
            wl, wl_bound = np.full(n, LD(o["sed_wave"])), np.zeros(n, dtype=LD)
        # profile
        gu, gv = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
        dev = np.zeros(n, dtype=LD)                     # sum of (stage scale) * (radius drawn), before |winv|
        extra = np.zeros(n, dtype=LD)                   # other derived terms, before |winv|
        flux = np.full(n, LD(o["flux_per_photon"]))
        if pt >= 0:
            r = np.sqrt(radial_r2(src.r2[pt], src.cdf[pt], w01(w[1]))) * ps
            a = TWO_PI * w01(w[2])
            gu, gv = r * np.cos(a), r * np.sin(a)
            dev += jnorm * np.abs(r)
        elif pt == PROF_BOX:
            gu, gv = (w01(w[1]) - LD(0.5)) * ps, (w01(w[2]) - LD(0.5)) * aux
        elif pt == PROF_IMAGE:
            ki = int(o["prof_aux"])
            iw, ih = src.image_sizes[ki]
            gx, gy, pix, f = image_nearest(src.image_cdfs[ki], iw, ih, w01(w[1]), w01(w[2]))
            if src.interp is not None:
                kx, kcdf, norm, neg = src.interp
                dx, nx_, slope = interp_offset(kx, kcdf, neg, f, exact=False)
                dy, ny_, _ = interp_offset(kx, kcdf, neg, w01(w[2]))
                gx = ((pix % iw) + LD(0.5) + dx) - LD(iw) / 2
                gy = ((pix // iw) + LD(0.5) + dy) - LD(ih) / 2
                flux = flux * np.where(nx_ != ny_, -LD(norm), LD(norm))
                extra += jnorm * abs(ps) * slope * f * 2 * EPS
            gu, gv = gx * ps, gy * ps
            # the operands that are added up are as large as half the image, whatever the photon's own position
            extra += 64 * EPS * jnorm * abs(ps) * (LD(max(iw, ih)) + 4)
        elif pt == PROF_KNOTS:
            nk = int(o["prof_aux"])
            m = ((2 * w[1] + U64(1)) * U64(nk)) >> U64(33)            # floor(u n_knots), u = (2 w + 1) / 2^33
            kw = words(src.seed, oid, m.astype(np.int64), SLOT_KNOT)
            g0, g1, rad = gauss_pair(kw[0], kw[1])
            gu, gv = ps * g0, ps * g1
            dev += jnorm * abs(ps) * rad
        pu, pv = jac[0] * gu + jac[1] * gv, jac[2] * gu + jac[3] * gv
        mpu, mpv = abs(jac[0]) * np.abs(gu) + abs(jac[1]) * np.abs(gv), abs(jac[2]) * np.abs(gu) + abs(jac[3]) * np.abs(gv)
        x, y = winv[0] * pu + winv[1] * pv, winv[2] * pu + winv[3] * pv
        mag = wnorm * (mpu + mpv)                        # magnitude of everything added into x or y so far
        # PSF components, in list order
        for c, (kind, table, p0, alpha, base, p1, p2) in enumerate(src.psf):
            kind = int(kind)
            b = words(src.seed, oid, k, SLOT_PSF + (c >> 1))
            wa, wb = b[2 * (c & 1)], b[2 * (c & 1) + 1]
            scale = np.full(n, LD(p0))
            chrom = np.zeros(n, dtype=LD)
            if alpha != 0.0:
                ratio = wl / LD(base)
                scale = scale * np.power(ratio, LD(alpha))
                chrom = LD(4e-15) * (1 + np.abs(LD(alpha) * np.log(ratio))) + abs(LD(alpha)) * wl_bound / np.abs(wl)
            if kind == PSF_GAUSSIAN:
                g0, g1, rad = gauss_pair(wa, wb)
                ku, kv = scale * g0, scale * g1
                dev += np.abs(scale) * rad
            elif kind == PSF_DOUBLE_GAUSSIAN:
                pick = w01(words(src.seed, oid, k, SLOT_PSF_TIME + c)[0]) < LD(p2)
                sigma = np.where(pick, scale, LD(p1))
                chrom = np.where(pick, chrom, LD(0))
                g0, g1, rad = gauss_pair(wa, wb)
                ku, kv = sigma * g0, sigma * g1
                dev += np.abs(sigma) * rad
            elif kind == PSF_SCREENS:
                A = src.atm
                ro2, ri2 = A.r_outer * A.r_outer, A.r_inner * A.r_inner
                r = np.sqrt(ri2 + w01(wa) * (ro2 - ri2))
                a = TWO_PI * w01(wb)
                ppu, ppv = r * np.cos(a), r * np.sin(a)
                t = A.t0 + w01(words(src.seed, oid, k, SLOT_PSF_TIME + c)[0]) * A.exptime
                gx, gy, edge = A.gradient(ppu, ppv, t, o["atm_tan_x"], o["atm_tan_y"])
                ku, kv = scale * gx, scale * gy
                out.kick[sl, 0], out.kick[sl, 1] = gx, gy
                out.edge[sl] = edge
                screen_terms.append((sl, wnorm, np.abs(scale)))
                for f, v, bd in (("pupil_u", ppu, (SINCOS_ERR + 8 * EPS) * r), ("pupil_v", ppv, (SINCOS_ERR + 8 * EPS) * r),
                                 ("time", t, np.full(n, 4 * EPS * (abs(A.t0) + A.exptime)))):
                    out.fields[f][sl], out.bounds[f][sl] = v, bd
            elif kind == PSF_RADIAL:
                r = np.sqrt(radial_r2(src.r2[int(table)], src.cdf[int(table)], w01(wa))) * scale
                a = TWO_PI * w01(wb)
                ku, kv = r * np.cos(a), r * np.sin(a)
                dev += np.abs(r)
            else:
                raise ValueError(f"PSF kind {kind} is outside the photon source restated here")
            x, y = x + (winv[0] * ku + winv[1] * kv), y + (winv[2] * ku + winv[3] * kv)
            m = wnorm * (np.abs(ku) + np.abs(kv))
            mag = mag + m
            extra += (np.abs(ku) + np.abs(kv)) * chrom
        x, y = LD(o["x0"]) + x, LD(o["y0"]) + y
        ulp = 64 * EPS * (max(abs(LD(o["x0"])), abs(LD(o["y0"]))) + mag)
        for f, v in (("x", x), ("y", y)):
            out.fields[f][sl] = v
            out.bounds[f][sl] = wnorm * (dev * DEVIATE_ERR + extra) + ulp
        out.fields["flux"][sl], out.bounds["flux"][sl] = flux, 2 * EPS * np.abs(flux)
        out.fields["wavelength"][sl], out.bounds["wavelength"][sl] = wl, wl_bound
    out.kick_bound = None
    if has_screens:
        out.kick_bound = src.atm.gradient_bound()
        for sl, wnorm, scale in screen_terms:
            for f in ("x", "y"):
                out.bounds[f][sl] += wnorm * scale * 2 * out.kick_bound          # |ku| + |kv| of the kick's error
    out.near_edge = out.edge < EDGE
    return out


# ---------------- the one assertion both test files use ----------------
EDGE_SHARE_CAP = 1.0e-4


def assert_matches(shot, got, what, kick=None, ratios=None):
    """got: {field: float64 array} of a photon pool (the oracle's or the renderer's); kick: optionally the pre-pass's gradients
    [n][2].  Photons within 1e-9 cells of a cell edge are left out of x, y and the gradient (their share asserted first), nothing
    else anywhere.  ratios: a dict that collects the worst error / bound per field."""
    n = len(shot.fields["x"])
    assert shot.near_edge.sum() <= EDGE_SHARE_CAP * n, f"{what}: {shot.near_edge.sum()} of {n} photons within 1e-9 of a cell edge"
    worst = {}

    def check(name, value, ref, bound, keep):
        value = np.asarray(value)
        assert value.shape == ref.shape, f"{what}: {name} has shape {value.shape}, expected {ref.shape}"
        assert np.all(np.isfinite(value)), f"{what}: {name} is not finite"
        err = np.abs(value.astype(LD) - ref)[keep]
        bd = bound[keep] if np.ndim(bound) else np.full(err.shape, bound)
        ratio = np.where(err == 0, LD(0), err / np.where(bd > 0, bd, LD(1e-300)))
        worst[name] = max(worst.get(name, 0.0), float(ratio.max()) if ratio.size else 0.0)

    everything = np.ones(n, dtype=bool)
    for f in FIELDS:
        check(f, got[f], shot.fields[f], shot.bounds[f], ~shot.near_edge if f in ("x", "y") else everything)
    if kick is not None:
        assert shot.kick is not None
        check("kick", np.asarray(kick).reshape(-1, 2), shot.kick, shot.kick_bound, ~shot.near_edge)
    if ratios is not None:
        for f, v in worst.items():
            ratios[f] = max(ratios.get(f, 0.0), v)
    print(f"{what}: error / bound " + " ".join(f"{f}={v:.3g}" for f, v in worst.items()))
    bad = {f: v for f, v in worst.items() if not v <= 1.0}
    assert not bad, f"{what}: error exceeds the bound: {bad}"
    return worst
