"""Radial and azimuthal histograms of the delivered PSF at a table of field points (`output.psf_profile`; ims_psf_profile).

The photons of a point are those of psf_map (ims_psf_moments): what a render would shoot for it, in stage "psf" after the PSF
components [arcsec], in stage "ops" after the photon-operator chain [pixels relative to the point].  Here they are reduced on the
GPU to counts in radial bins and azimuthal sectors instead of to second moments: the faint `1/r^2` halo, the diffraction spikes
and the encircled-energy radii, none of which the second moments see.  This module holds the profile's own host half: the edges
and sector directions, the launch's buffers, and the estimators formed from the counts; the rows, the launch base, the centre and
the file layout are psf_probe's.

Layout of the counts of a point, [n_r + 2][n_phi + 1]: radial index 0 holds the photons inside the first edge, 1 .. n_r the bins
[r_{i-1}, r_i), n_r + 1 the photons at or beyond the last edge; sector b is the wedge from direction phi0 + 2 pi b / n_phi
counter-clockwise to the next, the last column the photons no sector claims (on the centre, or in a rounding gap)."""
import ctypes as C
import dataclasses
import math

import numpy as np

from . import _abi, psf_probe
from .psf_probe import STAGES, summary_header        # noqa: F401  (psf_profile.summary_header: the SUMMARY table's header)

FLUX_STAGES = ("ops",)              # the stages that run the operator chain, whose photons must leave with equal flux
MAX_R, MAX_PHI = 64, 64
PROFILE_REQ = ("file_name", "r_min", "r_max")
PROFILE_OPT = ("dir", "nx", "n_photons", "stage", "n_r", "spacing", "n_phi", "phi0", "centre")
SUMMARY = ("n_used", "n_dropped", "EE50", "EE80", "EE95")


@dataclasses.dataclass
class Profile:
    """counts int64 [n][n_r + 2][n_phi + 1]; n_used, n_dropped int64 [n]; r_edges f64 [n_r + 1] (radii), r2_edges their squares as
    the device got them; dirs f64 [n_phi][2] = (cos, sin) of the sectors' start directions; centre f64 [n][2] or None"""
    counts: np.ndarray
    n_used: np.ndarray
    n_dropped: np.ndarray
    r_edges: np.ndarray
    r2_edges: np.ndarray
    dirs: np.ndarray
    phi0: float = 0.0
    stage: str = "psf"
    centre: object = None

    @property
    def n_r(self):
        return len(self.r_edges) - 1

    @property
    def n_phi(self):
        return len(self.dirs)


def check_bins(r_edges, n_phi):
    """the radii as f64 [n_r + 1], checked: 1 .. 64 bins, finite, not negative, their squares strictly ascending"""
    r = np.array(r_edges, dtype=np.float64).reshape(-1)
    if not 1 <= len(r) - 1 <= MAX_R:
        raise ValueError(f"psf_profile: r_edges must hold 2 .. {MAX_R + 1} radii (n_r 1 .. {MAX_R}), not {len(r)}")
    if not np.all(np.isfinite(r)) or r[0] < 0.0 or not np.all(np.diff(r * r) > 0.0):
        raise ValueError("psf_profile: r_edges must be finite, not negative and strictly ascending")
    n_phi = int(n_phi)
    if n_phi != 0 and not 3 <= n_phi <= MAX_PHI:
        raise ValueError(f"psf_profile: n_phi must be 0 or 3 .. {MAX_PHI}, not {n_phi}")
    return r, n_phi


def sector_dirs(n_phi, phi0=0.0):
    """(cos, sin)(phi0 + 2 pi b / n_phi), b = 0 .. n_phi - 1 -> f64 [n_phi][2]: the array the device gets"""
    a = float(phi0) + 2.0 * math.pi * np.arange(int(n_phi), dtype=np.float64) / max(int(n_phi), 1)
    return np.stack([np.cos(a), np.sin(a)], axis=1).reshape(int(n_phi), 2)


def refuse_flux_operators(scene, stage):
    """The counts are unweighted: a chain whose photons leave with unequal flux cannot be histogrammed"""
    psf_probe.refuse_flux_operators("psf_profile", "profile", FLUX_STAGES, scene, stage)


class Prepared(psf_probe.FieldPointLaunch):
    """The rows and bins of one launch resident on the device: call it to enqueue ims_psf_profile, result() to fetch a Profile."""

    def __init__(self, renderer, rows, stage, r_edges, n_phi=0, phi0=0.0, centre=None, dirs=None, r2_edges=None):
        psf_probe.check_stage("psf_profile", stage)
        r, torch = renderer, renderer.torch
        refuse_flux_operators(r.scene, stage)
        self.r_edges, n_phi = check_bins(r_edges, n_phi if dirs is None else len(dirs))
        # (r2_edges / dirs: exact values for the device in place of the squares and the cosines formed here)
        self.r2_edges = self.r_edges * self.r_edges if r2_edges is None else np.array(r2_edges, dtype=np.float64).reshape(-1)
        if len(self.r2_edges) != len(self.r_edges) or not np.all(np.diff(self.r2_edges) > 0.0):
            raise ValueError("psf_profile: r2_edges must be strictly ascending, one per radius")
        self.dirs = sector_dirs(n_phi, phi0) if dirs is None else np.array(dirs, dtype=np.float64).reshape(n_phi, 2)
        self.phi0 = float(phi0)
        super().__init__(renderer, rows, stage, centre=centre)
        self.edge_t = torch.from_numpy(self.r2_edges).to(r.device)
        self.dir_t = torch.from_numpy(np.ascontiguousarray(self.dirs)).to(r.device) if n_phi else None
        self.spec = _abi.PsfProfile(len(self.r_edges) - 1, n_phi, self.edge_t.data_ptr(), self.dir_t.data_ptr() if n_phi else None)
        self.counts = torch.zeros((max(self.n, 1), len(self.r_edges) + 1, n_phi + 1), dtype=torch.int64, device=r.device)
        self.dropped = torch.zeros(max(self.n, 1), dtype=torch.int64, device=r.device)

    def __call__(self):
        r = self.renderer
        _abi.check(r.lib.ims_psf_profile(C.byref(self.params), self.stage, C.byref(self.spec), self.centre_ptr(), self.counts.data_ptr(),
                                         self.dropped.data_ptr(), r._stream()), "ims_psf_profile")

    def result(self):
        counts, dropped = self.fetch(self.counts, self.dropped)
        return Profile(counts=counts, n_used=counts.sum(axis=(1, 2)), n_dropped=dropped,
                       r_edges=self.r_edges, r2_edges=self.r2_edges, dirs=self.dirs, phi0=self.phi0, stage=self.stage_name,
                       centre=self.centre)


def profile(scene_or_psf, points, n_photons, r_edges, n_phi=0, phi0=0.0, centre=None, stage="psf", wavelength=None, seed=None,
            device="cuda:0", renderer=None):
    """Histograms of the PSF the scene delivers at `points` -> Profile.

    scene_or_psf, points, n_photons, stage, wavelength, seed: as for psf_map.compute (points may be ready OBJECT_DTYPE rows, then
    n_photons may be None).  r_edges: n_r + 1 ascending radii (the host squares them) in the stage's units; n_phi: 0, or 3 .. 64
    sectors starting at phi0 [rad] (the angle of +y against +x, counter-clockwise).  centre: None -- offsets from the point's
    nominal position; "centroid" -- from the centroid psf_map.compute measures for the same rows; an [n][2] array -- from
    nominal + centre.  A chain with a BandpassRatio operator is refused in stage "ops" (ValueError): the counts are unweighted.
    The counts of a point depend on nothing but the point: not on the other points of the call, their order, or the launch."""
    psf_probe.check_stage("psf_profile", stage)
    r_edges, n_phi = check_bins(r_edges, n_phi)
    scene = psf_probe._as_scene(scene_or_psf)
    refuse_flux_operators(scene, stage)
    rows = psf_probe.probe_rows("psf_profile", scene, points, n_photons, stage, wavelength)
    centre = psf_probe.resolve_centre("psf_profile", centre)           # (a string is checked here, before anything ends the call)
    if len(rows) == 0:
        zeros = np.zeros(0, dtype=np.int64)
        return Profile(np.zeros((0, len(r_edges) + 1, n_phi + 1), dtype=np.int64), zeros, zeros, r_edges, r_edges * r_edges,
                       sector_dirs(n_phi, phi0), float(phi0), stage, None)
    r = renderer if renderer is not None else psf_probe.renderer_for(scene, seed, device)
    run = Prepared(r, rows, stage, r_edges, n_phi, phi0, psf_probe.resolve_centre("psf_profile", centre, scene, rows, stage, r))
    run()
    return run.result()


# ---------------- estimators on the counts ----------------
def radial_counts(result):
    """photons per radial index, summed over the sectors -> int64 [n][n_r + 2]"""
    return np.asarray(result.counts).sum(axis=2)


def surface_density(result):
    """counts per unit area per arrived photon in each radial bin -> f64 [n][n_r]; area pi (r_{i+1}^2 - r_i^2), photons n_used
    (NaN rows where none arrived)"""
    r = np.asarray(result.r_edges, dtype=np.float64)
    area = math.pi * (r[1:] * r[1:] - r[:-1] * r[:-1])
    c = radial_counts(result)[:, 1:-1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return c / area[None, :] / np.asarray(result.n_used, dtype=np.float64)[:, None]


def encircled_energy(result):
    """the fraction of the arrived photons inside each edge -> f64 [n][n_r + 1]"""
    c = np.cumsum(radial_counts(result)[:, :-1], axis=1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return c / np.asarray(result.n_used, dtype=np.float64)[:, None]


def ee_radius(result, frac):
    """the radius that encircles `frac` of the arrived photons, linear between the edges -> f64 [n]; NaN where the fraction lies
    outside what the edges reach (below the first edge's, above the last edge's) or no photon arrived"""
    r = np.asarray(result.r_edges, dtype=np.float64)
    ee = encircled_energy(result)
    out = np.full(len(ee), np.nan)
    for i, e in enumerate(ee):
        if not np.all(np.isfinite(e)) or not e[0] <= frac <= e[-1]:
            continue
        k = int(np.searchsorted(e, frac, side="left"))               # the first edge with e >= frac
        if k == 0 or e[k] == frac:
            out[i] = r[k]
        else:
            out[i] = r[k - 1] + (r[k] - r[k - 1]) * (frac - e[k - 1]) / (e[k] - e[k - 1])
    return out


def halo_law(result, r_lo, r_hi):
    """Least-squares line of log10(surface density) against log10(r) over the radial bins that lie inside [r_lo, r_hi] and hold
    at least one photon, r the bin's geometric-mean radius (arithmetic mean for a bin that starts at 0) -> (slope [n],
    intercept [n]): surface density ~ 10^intercept r^slope.  NaN with fewer than two such bins."""
    r = np.asarray(result.r_edges, dtype=np.float64)
    lo, hi = r[:-1], r[1:]
    mid = np.where(lo > 0.0, np.sqrt(lo * hi), 0.5 * (lo + hi))
    inside = (lo >= r_lo) & (hi <= r_hi)
    sd = surface_density(result)
    slope, icpt = np.full(len(sd), np.nan), np.full(len(sd), np.nan)
    for i, s in enumerate(sd):
        use = inside & np.isfinite(s) & (s > 0.0)
        if use.sum() < 2:
            continue
        x, y = np.log10(mid[use]), np.log10(s[use])
        xm, ym = x.mean(), y.mean()
        slope[i] = ((x - xm) * (y - ym)).sum() / ((x - xm) ** 2).sum()
        icpt[i] = ym - slope[i] * xm
    return slope, icpt


def summary(result):
    """f64 [n][5]: n_used, n_dropped, EE50, EE80, EE95 (the columns of SUMMARY; the counts are exact in f64)"""
    return np.stack([np.asarray(result.n_used, dtype=np.float64), np.asarray(result.n_dropped, dtype=np.float64),
                     ee_radius(result, 0.5), ee_radius(result, 0.8), ee_radius(result, 0.95)], axis=1)


# ---------------- output.psf_profile ----------------
def parse_config(cfg, ev):
    """`output.psf_profile: {file_name, dir, nx: 4, n_photons: 1000000, stage: psf, r_min, r_max, n_r: 32, spacing: log | linear,
    n_phi: 0, phi0: 0 deg, centre: nominal | centroid}` -> the keywords of ccd_profile.  file_name and dir stay unevaluated: they
    may differ per CCD."""
    from .lsst_image import GalSimConfigError
    kw = psf_probe.parse_head("psf_profile", cfg, ev, PROFILE_REQ, PROFILE_OPT, nx=4, n_photons=1000000, centre=True)
    n_r, n_phi = int(ev.value(cfg.get("n_r", 32))), int(ev.value(cfg.get("n_phi", 0)))
    r_min, r_max = float(ev.value(cfg["r_min"])), float(ev.value(cfg["r_max"]))
    spacing = str(ev.value(cfg.get("spacing", "log")))
    phi0 = ev.value(cfg.get("phi0", "0 deg"))
    if not 1 <= n_r <= MAX_R:
        raise GalSimConfigError(f"output.psf_profile.n_r must be 1 .. {MAX_R}, not {n_r}")
    if n_phi != 0 and not 3 <= n_phi <= MAX_PHI:
        raise GalSimConfigError(f"output.psf_profile.n_phi must be 0 or 3 .. {MAX_PHI}, not {n_phi}")
    if spacing not in ("log", "linear"):
        raise GalSimConfigError(f"output.psf_profile.spacing must be log or linear, not {spacing}")
    if not (math.isfinite(r_min) and math.isfinite(r_max)) or r_min < 0.0:
        raise GalSimConfigError("output.psf_profile.r_min and r_max must be finite and r_min not negative")
    if r_min >= r_max:
        raise GalSimConfigError(f"output.psf_profile.r_min must be below r_max ({r_min} >= {r_max})")
    if spacing == "log" and r_min <= 0.0:
        raise GalSimConfigError("output.psf_profile.r_min must be positive with spacing: log")
    if isinstance(phi0, bool) or not isinstance(phi0, (int, float)):
        raise GalSimConfigError(f"output.psf_profile.phi0: cannot read {cfg.get('phi0')!r} as an angle")
    return dict(kw, r_edges=radial_edges(r_min, r_max, n_r, spacing), n_phi=n_phi, phi0=float(phi0))


def check_scene(scene, stage):
    """The refusals of profile() as config errors, for config.Process to raise before a CCD is rendered"""
    from .lsst_image import GalSimConfigError
    try:
        refuse_flux_operators(scene, stage)
    except ValueError as e:
        raise GalSimConfigError(f"output.psf_profile: {e}") from None


def radial_edges(r_min, r_max, n_r, spacing="log"):
    """n_r + 1 radii from r_min to r_max, both ends exact, in equal steps of r (linear) or of log r (log)"""
    t = np.arange(n_r + 1, dtype=np.float64) / n_r
    r = r_min + (r_max - r_min) * t if spacing == "linear" else r_min * (r_max / r_min) ** t
    r[0], r[-1] = r_min, r_max
    return r


def make_header(det_name, result, wavelength, n_photons, nx_ccd, ny_ccd, n, centre, sampled=False):
    """the probes' common cards, and the bins: the edges as radii R_EDGE0 .. R_EDGE<n_r>"""
    h = psf_probe.probe_header(det_name, result.stage, wavelength, n_photons, nx_ccd, ny_ccd, n, sampled)
    h["units"] = ("arcsec" if result.stage == "psf" else "pixel", "of the radial edges")
    h["n_r"] = (int(result.n_r), "radial bins; axis 2 holds n_r + 2: under, bins, over")
    h["n_phi"] = (int(result.n_phi), "sectors; axis 1 holds n_phi + 1: the last unassigned")
    h["phi0"] = (float(result.phi0), "(rad) start direction of sector 0, from +x to +y")
    h["centre"] = (str(centre), "offsets from the nominal position or the centroid")
    for k, r in enumerate(result.r_edges):
        h[f"R_EDGE{k}"] = (float(r), "radial edge")
    return h


def write(file_name, hdus):
    """hdus: [(cube, header, summary, summary header)] per CCD -> two HDUs each: the counts as an f64 image
    [point][radial][sector] (exact for counts) and a binary table SUMMARY, one row per point, with the columns of SUMMARY
    (n_used, n_dropped as 64-bit integers, the EE radii as doubles)"""
    psf_probe.write_counts(file_name, hdus, SUMMARY)


def ccd_profile(scene, det_name, nx, n_photons, stage, r_edges, n_phi=0, phi0=0.0, centre="nominal", wavelength=None, wl_eff=None,
                device="cuda:0"):
    """The profiles of one CCD on psf_map's nx x nx grid over the scene's pixels: (cube, header, summary, summary header)"""
    pts = psf_probe.grid_points(scene.nx, scene.ny, nx)
    res = profile(scene, pts, n_photons, r_edges, n_phi=n_phi, phi0=phi0, centre=centre, stage=stage, wavelength=wavelength, device=device)
    sampled = wavelength is None
    h = make_header(det_name, res, wl_eff if sampled else wavelength, n_photons, scene.nx, scene.ny, nx, centre, sampled)
    return res.counts.astype(np.float64), h, summary(res), summary_header(det_name)
