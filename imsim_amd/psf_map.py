"""Moments of the delivered PSF at a table of field points (`output.psf_map`; ims_psf_moments).

The photons of a point are the photons a render would shoot for it -- the PSF components of the scene (AtmosphericPSF with its
second kick and optical screen, Gaussian, Kolmogorov, DoubleGaussian) and, in stage "ops", the photon-operator chain up to the
position the sensor would receive -- but they are reduced on the GPU to six weighted sums and two counts per point instead of
being landed or stored.  This module holds the moments' own host half: the two launches' buffers, and the moments formed from the
sums; the point rows, the launch base and the common head of the config key are psf_probe's, shared with psf_profile and psf_image.

Units: stage "psf" leaves the offsets as the PSF kicks make them, in arcsec (+u west, +v north: the rows' local WCS is the
identity); stage "ops" gives focal-plane pixels of the scene's CCD relative to the point's pixel position."""
import ctypes as C
import math
import os

import numpy as np

from . import _abi, fits_io, psf_probe
from .psf_probe import STAGES, _as_scene, grid_points, point_rows, renderer_for        # noqa: F401  (psf_map.<name> is their public home)

FWHM_PER_SIGMA = 2.3548200450309493
MOMENTS_DTYPE = np.dtype([("flux", "<f8"), ("n_used", "<i8"), ("n_dropped", "<i8"), ("xbar", "<f8"), ("ybar", "<f8"),
                          ("Ixx", "<f8"), ("Iyy", "<f8"), ("Ixy", "<f8"), ("sigma", "<f8"), ("e1", "<f8"), ("e2", "<f8"),
                          ("fwhm", "<f8")])
# the planes of the FITS cube, in order, with the comment of their header card
PLANES = (("flux", "sum of the photon weights"), ("n_used", "photons that arrived"),
          ("n_dropped", "photons vignetted or lost in the trace"), ("xbar", "centroid x - nominal"), ("ybar", "centroid y - nominal"),
          ("Ixx", "central second moment"), ("Iyy", "central second moment"), ("Ixy", "central second moment"),
          ("sigma", "(Ixx Iyy - Ixy^2)^(1/4)"), ("e1", "(Ixx - Iyy) / (Ixx + Iyy)"), ("e2", "2 Ixy / (Ixx + Iyy)"),
          ("fwhm", "Gaussian-equivalent width 2.3548 sigma"))
MAP_REQ = ("file_name",)
MAP_OPT = ("dir", "nx", "n_photons", "stage", "moments", "guess_sigma", "tolerance", "max_iter")
MOMENT_KINDS = ("unweighted", "adaptive")
ADAPTIVE_KEYS = ("guess_sigma", "tolerance", "max_iter")
# adaptive moments (ims_psf_adaptive): status 0 converged, 1 still running / max_iter reached, 2 failed, 3 no photon arrived
CONVERGED, RUNNING, FAILED, EMPTY = 0, 1, 2, 3
ADAPTIVE_ROUNDS = 16                # rounds enqueued between two looks at the statuses
ADAPTIVE_DTYPE = np.dtype([("status", "<i4"), ("iter", "<i4"), ("xbar", "<f8"), ("ybar", "<f8"), ("Mxx", "<f8"), ("Myy", "<f8"),
                           ("Mxy", "<f8"), ("sigma", "<f8"), ("e1", "<f8"), ("e2", "<f8"), ("rho4", "<f8"), ("fwhm", "<f8"),
                           ("n_used", "<i8"), ("n_dropped", "<i8"), ("flux", "<f8")])
# the planes `moments: adaptive` appends to the cube (PLANE13 ...), with the comment of their header card
ADAPTIVE_PLANES = (("a_status", "0 converged 1 max_iter 2 failed 3 no photon"), ("a_iter", "weight updates applied"),
                   ("a_xbar", "adaptive centroid x - nominal"), ("a_ybar", "adaptive centroid y - nominal"),
                   ("a_Mxx", "adaptive weight matrix"), ("a_Myy", "adaptive weight matrix"), ("a_Mxy", "adaptive weight matrix"),
                   ("a_sigma", "(Mxx Myy - Mxy^2)^(1/4)"), ("a_e1", "(Mxx - Myy) / (Mxx + Myy)"), ("a_e2", "2 Mxy / (Mxx + Myy)"),
                   ("a_rho4", "weighted radial 4th moment; 2 for a Gaussian"), ("a_fwhm", "Gaussian-equivalent width 2.3548 a_sigma"))


def moments_from_sums(sums, counts):
    """sums [n][6] = sum w, w x, w y, w x^2, w x y, w y^2 and counts [n][2] = used, dropped -> MOMENTS_DTYPE rows.  A point without
    a photon that arrived (n_used == 0) has flux 0 and NaN everywhere else; nothing raises.  `fwhm` is the width of the Gaussian
    with the same sigma, 2.3548200450309493 sigma -- not a measurement of the profile's half maximum."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 6)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(len(sums), dtype=MOMENTS_DTYPE)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(counts[:, 0] > 0, sums[:, 0], np.nan)
        xbar, ybar = sums[:, 1] / w, sums[:, 2] / w
        ixx = sums[:, 3] / w - xbar * xbar
        ixy = sums[:, 4] / w - xbar * ybar
        iyy = sums[:, 5] / w - ybar * ybar
        sigma = np.sqrt(np.sqrt(ixx * iyy - ixy * ixy))
        tr = ixx + iyy
        out["e1"], out["e2"] = (ixx - iyy) / tr, 2.0 * ixy / tr
    out["flux"], out["n_used"], out["n_dropped"] = sums[:, 0], counts[:, 0], counts[:, 1]
    out["xbar"], out["ybar"], out["Ixx"], out["Iyy"], out["Ixy"] = xbar, ybar, ixx, iyy, ixy
    out["sigma"], out["fwhm"] = sigma, FWHM_PER_SIGMA * sigma
    return out


class Prepared(psf_probe.FieldPointLaunch):
    """The rows of one launch resident on the device: call it to enqueue ims_psf_moments, result() to fetch the moments."""

    def __init__(self, renderer, rows, stage):
        psf_probe.check_stage("psf_map", stage)
        super().__init__(renderer, rows, stage)
        r, torch = renderer, renderer.torch
        self.partial = torch.empty(max(8 * self.n_segments, 1), dtype=torch.float64, device=r.device)
        self.sums = torch.zeros((max(self.n, 1), 6), dtype=torch.float64, device=r.device)
        self.counts = torch.zeros((max(self.n, 1), 2), dtype=torch.int64, device=r.device)

    def __call__(self):
        r = self.renderer
        _abi.check(r.lib.ims_psf_moments(C.byref(self.params), self.stage, self.partial.data_ptr(), self.sums.data_ptr(),
                                         self.counts.data_ptr(), r._stream()), "ims_psf_moments")

    def raw(self):
        """(sums [n][6], counts [n][2]) on the host"""
        return self.fetch(self.sums, self.counts)

    def result(self):
        return moments_from_sums(*self.raw())


def compute(scene_or_psf, points, n_photons=None, stage="psf", wavelength=None, seed=None, device="cuda:0", renderer=None):
    """Moments of the PSF the scene delivers at `points`: MOMENTS_DTYPE rows, one per point, in the points' order.

    scene_or_psf: an engine.Scene, or a list of PSF component tuples (stage "psf" only).
    points: pixel positions [n][2] on the scene's CCD (rows made by point_rows), or ready OBJECT_DTYPE rows (n_photons None: the
    rows' own counts; phot_first is the base of the 64-bit photon index).
    stage: "psf" -- shoot + PSF, offsets in arcsec; "ops" -- also the scene's photon operators, focal-plane pixels relative to
    the point.  seed: the random seed (default: the scene's).  A point all of whose photons are vignetted has n_used 0 and NaN
    moments.  The result does not depend on which other points share the call, nor on their order."""
    psf_probe.check_stage("psf_map", stage)
    scene = _as_scene(scene_or_psf)
    rows = psf_probe.probe_rows("psf_map", scene, points, n_photons, stage, wavelength)
    if len(rows) == 0:
        return np.zeros(0, dtype=MOMENTS_DTYPE)
    r = renderer if renderer is not None else renderer_for(scene, seed, device)
    run = Prepared(r, rows, stage)
    run()
    return run.result()


# ---------------- adaptive moments (ims_psf_adaptive) ----------------
def adaptive_from_state(state, status, aux):
    """state [n][5] = x0, y0, Mxx, Mxy, Myy; status [n][2] = status, iter; aux [n][4] = rho4, sum w, used, dropped ->
    ADAPTIVE_DTYPE rows.  sigma = det^(1/4), e1 = (Mxx - Myy) / (Mxx + Myy), e2 = 2 Mxy / (Mxx + Myy), fwhm = 2.3548200450309493
    sigma (the width of the Gaussian with that sigma, not a measurement of the half maximum).  A row no photon of which arrived
    (status 3) has flux 0 and NaN everywhere else; nothing raises."""
    state = np.asarray(state, dtype=np.float64).reshape(-1, 5)
    status = np.asarray(status, dtype=np.int32).reshape(-1, 2)
    aux = np.asarray(aux, dtype=np.float64).reshape(-1, 4)
    out = np.zeros(len(state), dtype=ADAPTIVE_DTYPE)
    empty = status[:, 0] == EMPTY
    st = np.where(empty[:, None], np.nan, state)
    mxx, mxy, myy = st[:, 2], st[:, 3], st[:, 4]
    with np.errstate(divide="ignore", invalid="ignore"):
        sigma = np.sqrt(np.sqrt(mxx * myy - mxy * mxy))
        tr = mxx + myy
        out["e1"], out["e2"] = (mxx - myy) / tr, 2.0 * mxy / tr
    out["status"], out["iter"] = status[:, 0], status[:, 1]
    out["xbar"], out["ybar"], out["Mxx"], out["Myy"], out["Mxy"] = st[:, 0], st[:, 1], mxx, myy, mxy
    out["sigma"], out["fwhm"] = sigma, FWHM_PER_SIGMA * sigma
    out["rho4"] = np.where(empty, np.nan, aux[:, 0])
    out["flux"], out["n_used"], out["n_dropped"] = aux[:, 1], aux[:, 2].astype(np.int64), aux[:, 3].astype(np.int64)
    return out


def adaptive_start(moments, guess_centre=None, guess_sigma=None):
    """The start of every row from its unweighted moments (MOMENTS_DTYPE): (state [n][5], status [n]).  Default: the unweighted
    centroid and M = (Ixx + Iyy) / 2 times the identity.  guess_centre ([n][2] or one pair) and guess_sigma (a scalar or [n])
    override it.  A row without a photon that arrived is EMPTY (NaN state); a row whose start is not a finite centre and a
    finite positive M -- a single photon without guess_sigma -- is FAILED; every other row is RUNNING."""
    n = len(moments)
    state = np.zeros((n, 5), dtype=np.float64)
    state[:, 0], state[:, 1] = moments["xbar"], moments["ybar"]
    state[:, 2] = state[:, 4] = 0.5 * (moments["Ixx"] + moments["Iyy"])
    if guess_centre is not None:
        state[:, :2] = np.broadcast_to(np.asarray(guess_centre, dtype=np.float64), (n, 2))
    if guess_sigma is not None:
        gs = np.broadcast_to(np.asarray(guess_sigma, dtype=np.float64), (n,))
        if not np.all(np.isfinite(gs) & (gs > 0.0)):
            raise ValueError("psf_map: guess_sigma must be positive and finite")
        state[:, 2] = state[:, 4] = gs * gs
    status = np.full(n, RUNNING, dtype=np.int32)
    ok = np.isfinite(state).all(axis=1) & (state[:, 2] > 0.0)
    status[~ok] = FAILED
    empty = moments["n_used"] == 0
    status[empty] = EMPTY
    state[empty] = np.nan
    return state, status


class PreparedAdaptive(psf_probe.FieldPointLaunch):
    """The rows of one adaptive-moments run resident on the device, with the state the iteration starts from: call it to iterate
    (rounds are enqueued in batches of ADAPTIVE_ROUNDS, the statuses read between batches, until no row is running or max_iter
    rounds are done), result() to fetch the rows.  rounds(k) enqueues k rounds and reads nothing back."""

    def __init__(self, renderer, rows, stage, state, status, aux=None, tol=1e-6, max_iter=100):
        psf_probe.check_stage("psf_map", stage)
        if not (tol > 0.0 and math.isfinite(tol)):
            raise ValueError("psf_map: tol must be positive and finite")
        if int(max_iter) < 1:
            raise ValueError("psf_map: max_iter must be at least 1")
        super().__init__(renderer, rows, stage)
        r, torch = renderer, renderer.torch
        self.tol, self.max_iter, self.done = float(tol), int(max_iter), 0
        n = self.n
        st2 = np.zeros((max(n, 1), 2), dtype=np.int32)
        st2[:n, 0] = np.asarray(status, dtype=np.int32).reshape(n)
        s5 = np.zeros((max(n, 1), 5), dtype=np.float64)
        s5[:n] = np.asarray(state, dtype=np.float64).reshape(n, 5)
        a4 = np.zeros((max(n, 1), 4), dtype=np.float64)
        a4[:, 0] = np.nan
        if aux is not None:
            a4[:n] = np.asarray(aux, dtype=np.float64).reshape(n, 4)
        self.partial = torch.empty(max(10 * self.n_segments, 1), dtype=torch.float64, device=r.device)
        self.state = torch.from_numpy(s5).to(r.device)
        self.status = torch.from_numpy(st2).to(r.device)
        self.aux = torch.from_numpy(a4).to(r.device)

    def rounds(self, k):
        r = self.renderer
        _abi.check(r.lib.ims_psf_adaptive(C.byref(self.params), self.stage, int(k), self.tol, self.partial.data_ptr(),
                                          self.state.data_ptr(), self.status.data_ptr(), self.aux.data_ptr(), r._stream()),
                   "ims_psf_adaptive")
        self.done += int(k)

    def running(self):
        self.renderer.synchronize()
        return int((self.status[:self.n, 0] == RUNNING).sum().item())

    def __call__(self):
        while self.n and self.done < self.max_iter and self.running():
            self.rounds(min(ADAPTIVE_ROUNDS, self.max_iter - self.done))

    def raw(self):
        """(state [n][5], status [n][2], aux [n][4]) on the host"""
        return self.fetch(self.state, self.status, self.aux)

    def result(self):
        return adaptive_from_state(*self.raw())


def adaptive(scene_or_psf, points, n_photons=None, stage="psf", guess_centre=None, guess_sigma=None, tol=1e-6, max_iter=100,
             wavelength=None, seed=None, device="cuda:0", renderer=None):
    """Adaptive moments of the PSF the scene delivers at `points`: ADAPTIVE_DTYPE rows, one per point, in the points' order.

    The moments are those of the elliptical Gaussian weight that matches the profile: the weight's centre and matrix are iterated
    until the weighted centroid sits on the centre and the weighted second moments are half the matrix (Bernstein & Jarvis 2002;
    Hirata & Seljak 2003) -- the published scheme of GalSim's `hsm` module, its corrections clipped to a quarter per step.  GalSim
    is not installed beside this package and no call into it confirms the numbers: they are held to an independent numpy statement
    of the same iteration (tests/adaptive_moments_ref.py) and to closed forms.  Unlike the unweighted moments of compute(), which
    the 1/r^2 halo and the spikes of the rendered PSF dominate, these describe the core: `sigma`, `e1`, `e2` in the convention of
    image measurements, `rho4` the weighted radial fourth moment (2 for a Gaussian).

    scene_or_psf, points, n_photons, stage, wavelength, seed, renderer: as for compute().  Every round shoots the points' photons
    again from their counters (nothing is stored) -- the cost is one ims_psf_moments call for the start plus one per round.
    The start of a row is its unweighted centroid and M = (Ixx + Iyy) / 2 times the identity; guess_centre ([n][2] or one pair)
    and guess_sigma (a scalar or [n]) override it.  tol: the iteration stops when the largest correction, in units of the weight's
    minor axis times the axis ratio, is below it; max_iter: rounds at most.
    status: 0 converged; 1 max_iter reached; 2 failed (the weight stopped being positive definite, or the row has no usable start:
    a single photon without guess_sigma); 3 no photon arrived (NaN).  The result does not depend on which other points share the
    call, nor on their order."""
    psf_probe.check_stage("psf_map", stage)
    scene = _as_scene(scene_or_psf)
    rows = psf_probe.probe_rows("psf_map", scene, points, n_photons, stage, wavelength)
    if len(rows) == 0:
        return np.zeros(0, dtype=ADAPTIVE_DTYPE)
    r = renderer if renderer is not None else renderer_for(scene, seed, device)
    first = Prepared(r, rows, stage)
    first()
    m = first.result()
    state, status = adaptive_start(m, guess_centre, guess_sigma)
    aux = np.stack([np.full(len(m), np.nan), m["flux"], m["n_used"].astype(np.float64), m["n_dropped"].astype(np.float64)], axis=1)
    run = PreparedAdaptive(r, rows, stage, state, status, aux, tol=tol, max_iter=max_iter)
    run()
    return run.result()


# ---------------- output.psf_map ----------------
def parse_config(cfg, ev):
    """`output.psf_map: {file_name, dir, nx: 8, n_photons: 100000, stage: psf}` -> (nx, n_photons, stage).  file_name and dir stay
    unevaluated: they may differ per CCD.  With `moments: adaptive` (default `unweighted`) the result also holds moments and
    the iteration's guess_sigma (None: the unweighted start), tolerance (1e-6) and max_iter (100)."""
    from .lsst_image import GalSimConfigError
    kw = psf_probe.parse_head("psf_map", cfg, ev, MAP_REQ, MAP_OPT, nx=8, n_photons=100000)
    moments = str(ev.value(cfg.get("moments", "unweighted")))
    if moments not in MOMENT_KINDS:
        raise GalSimConfigError(f"output.psf_map.moments must be one of {list(MOMENT_KINDS)}, not {moments}")
    if moments == "unweighted":
        for k in ADAPTIVE_KEYS:
            if k in cfg:
                raise GalSimConfigError(f"output.psf_map.{k} is given without moments: adaptive")
        return kw
    guess_sigma = float(ev.value(cfg["guess_sigma"])) if "guess_sigma" in cfg else None
    tolerance = float(ev.value(cfg.get("tolerance", 1e-6)))
    max_iter = int(ev.value(cfg.get("max_iter", 100)))
    if guess_sigma is not None and not (guess_sigma > 0.0 and math.isfinite(guess_sigma)):
        raise GalSimConfigError("output.psf_map.guess_sigma must be positive and finite")
    if not (tolerance > 0.0 and math.isfinite(tolerance)):
        raise GalSimConfigError("output.psf_map.tolerance must be positive and finite")
    if max_iter < 1:
        raise GalSimConfigError("output.psf_map.max_iter must be at least 1")
    return dict(kw, moments=moments, guess_sigma=guess_sigma, tolerance=tolerance, max_iter=max_iter)


def cube(moments, n):
    """MOMENTS_DTYPE rows of grid_points(.., n) -> f64 [plane][ny][nx], the planes in the order of PLANES"""
    return np.stack([np.asarray(moments[name], dtype=np.float64).reshape(n, n) for name, _ in PLANES])


def adaptive_cube(rows, n):
    """ADAPTIVE_DTYPE rows of grid_points(.., n) -> f64 [plane][ny][nx], the planes in the order of ADAPTIVE_PLANES"""
    return np.stack([np.asarray(rows[name[2:]], dtype=np.float64).reshape(n, n) for name, _ in ADAPTIVE_PLANES])


def make_header(det_name, stage, wavelength, n_photons, nx_ccd, ny_ccd, n, sampled=False, adaptive=None):
    """wavelength [nm]: the photons' one wavelength, or with sampled the effective wavelength of the bandpass they sample.
    adaptive: None, or (tolerance, max_iter) of a cube that carries the ADAPTIVE_PLANES behind the PLANES"""
    h = psf_probe.probe_header(det_name, stage, wavelength, n_photons, nx_ccd, ny_ccd, n, sampled)
    for k, (name, comment) in enumerate(PLANES, 1):
        h[f"PLANE{k}"] = (name, comment)
    if adaptive is not None:
        for k, (name, comment) in enumerate(ADAPTIVE_PLANES, len(PLANES) + 1):
            h[f"PLANE{k}"] = (name, comment)
        h["TOL"] = (float(adaptive[0]), "adaptive moments: convergence threshold")
        h["MAXITER"] = (int(adaptive[1]), "adaptive moments: rounds at most")
    return h


def write(file_name, hdus):
    """hdus: [(cube, header)], one image HDU per CCD, the first one primary"""
    os.makedirs(os.path.dirname(file_name) or ".", exist_ok=True)
    fits_io.write_fits(file_name, [(dict(h), np.asarray(c, dtype=np.float64)) for c, h in hdus])


def ccd_map(scene, det_name, nx, n_photons, stage, wavelength=None, wl_eff=None, device="cuda:0", moments="unweighted",
            guess_sigma=None, tolerance=1e-6, max_iter=100):
    """The map of one CCD: (cube, header) for an nx x nx grid over the scene's pixels.  wavelength None: the photons sample the
    scene's bandpass, whose effective wavelength wl_eff goes into the header.  moments "adaptive": the adaptive moments of the
    same points behind the 12 unweighted planes, which stay what they are without it."""
    pts = grid_points(scene.nx, scene.ny, nx)
    m = compute(scene, pts, n_photons, stage=stage, wavelength=wavelength, device=device)
    sampled = wavelength is None
    wl = wl_eff if sampled else wavelength
    if moments == "unweighted":
        return cube(m, nx), make_header(det_name, stage, wl, n_photons, scene.nx, scene.ny, nx, sampled)
    a = adaptive(scene, pts, n_photons, stage=stage, guess_sigma=guess_sigma, tol=tolerance, max_iter=max_iter, wavelength=wavelength,
                 device=device)
    return (np.concatenate([cube(m, nx), adaptive_cube(a, nx)]),
            make_header(det_name, stage, wl, n_photons, scene.nx, scene.ny, nx, sampled, adaptive=(tolerance, max_iter)))
