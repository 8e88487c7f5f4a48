"""Postage stamps of the delivered PSF at a table of field points, up to the sensor (`output.psf_image`; ims_psf_image).

The photons of a point are those of psf_map and psf_profile (ims_psf_moments): what a render would shoot for it.  Here they are
binned on the GPU into an image of counts per point -- what `psf.drawImage(method="phot")` hands a GalSim user -- at any cell
size, without a CCD render, without sky, noise or the star's own brighter-fatter effect.

Stages: "psf" -- after the PSF components [arcsec]; "ops" -- after the photon-operator chain [pixels relative to the point];
"sensor" -- after the first half of SiliconSensor.accumulate as well [pixels]: conversion at a wavelength-dependent depth, the
lateral walk of an inclined ray down to that depth, and charge diffusion.  That is the PSF a measurement on the e-image sees; the
other two stop at the sensor's surface.  Stage "sensor" is NOT a render: there is no pixel search.  The stamp bins continuous
positions on a regular grid, and tree rings and the brighter-fatter effect, which move pixel boundaries and not photons, do not
appear in it.

Layout of a point's stamp, counts[iy][ix]: cell ix covers [ix - nx / 2, ix + 1 - nx / 2) * scale around the centre along x,
lower edge included (the binning rule of include/imsim_hip.h); photons beside the stamp are counted in n_outside, lost photons
(vignetted, the ray failed, converted beyond the back of the sensor) in n_dropped.  This module holds the stamps' own host half:
the launch's buffers, the renderer that keeps the sensor, and two small estimators; the rows, the launch base, the centre and the
file layout are psf_probe's."""
import ctypes as C
import dataclasses
import math

import numpy as np

from . import _abi, psf_probe
from .psf_probe import summary_header        # noqa: F401  (psf_image.summary_header: the SUMMARY table's header)

STAGES = {"psf": 1, "ops": 2, "sensor": 3}
FLUX_STAGES = ("ops", "sensor")     # the stages that run the operator chain, whose photons must leave with equal flux
UNITS = {"psf": "arcsec", "ops": "pixel", "sensor": "pixel"}
MAX_SIZE = _abi.PSF_IMAGE_MAX
IMAGE_REQ = ("file_name", "scale")
IMAGE_OPT = ("dir", "nx", "n_photons", "stage", "size", "centre")
SUMMARY = ("x", "y", "n_used", "n_outside", "n_dropped")
MOMENTS_DTYPE = np.dtype([("n", "<i8"), ("xbar", "<f8"), ("ybar", "<f8"), ("Ixx", "<f8"), ("Iyy", "<f8"), ("Ixy", "<f8"),
                          ("sigma", "<f8"), ("e1", "<f8"), ("e2", "<f8")])


@dataclasses.dataclass
class Stamps:
    """counts int64 [n][ny][nx]; n_used (the photons in the stamp), n_outside, n_dropped int64 [n]: per point they add up to its
    photons; scale: the side of a cell in the stage's units, inv_scale its reciprocal as the device got it; centre f64 [n][2]
    (offset of the stamp's centre from the nominal position) or None"""
    counts: np.ndarray
    n_used: np.ndarray
    n_outside: np.ndarray
    n_dropped: np.ndarray
    scale: float
    inv_scale: float
    stage: str = "psf"
    centre: object = None

    @property
    def nx(self):
        return self.counts.shape[2]

    @property
    def ny(self):
        return self.counts.shape[1]


def check_size(size):
    """an int or (nx, ny) -> (nx, ny), each 1 .. 512"""
    if isinstance(size, (int, np.integer)) and not isinstance(size, bool):
        nx = ny = int(size)
    else:
        try:
            nx, ny = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError(f"psf_image: size must be an int or (nx, ny), not {size!r}") from None
    if not (1 <= nx <= MAX_SIZE and 1 <= ny <= MAX_SIZE):
        raise ValueError(f"psf_image: size must be 1 .. {MAX_SIZE} cells along each axis, not {nx} x {ny}")
    return nx, ny


def check_scale(scale):
    scale = float(scale)
    if not (scale > 0.0 and math.isfinite(scale) and math.isfinite(1.0 / scale)):
        raise ValueError(f"psf_image: scale must be positive and finite, not {scale!r}")
    return scale


def check_stage(stage):
    psf_probe.check_stage("psf_image", stage, STAGES)


def refuse_flux_operators(scene, stage):
    """The counts are unweighted: a chain whose photons leave with unequal flux cannot be binned"""
    psf_probe.refuse_flux_operators("psf_image", "stamp", FLUX_STAGES, scene, stage)


def require_sensor(scene, stage):
    if stage == "sensor" and getattr(scene, "sensor", None) is None:
        raise ValueError("psf_image: stage 'sensor' needs a scene with a Silicon sensor (scene.sensor is None)")


def renderer_for(scene, stage, seed=None, device="cuda:0"):
    """psf_map.renderer_for for stages "psf" and "ops"; for "sensor" the same bare one-pixel scene with the sensor's model and
    absorption table kept -- the conversion reads nothing else, so no pixel-boundary state of a CCD is made"""
    if stage != "sensor":
        return psf_probe.renderer_for(scene, seed, device)
    from .engine import Renderer, make_slots
    sensor = dataclasses.replace(scene.sensor, slots=make_slots([(1, 1, 1, 1)]), scratch_cells=0)
    bare = dataclasses.replace(scene, nx=1, ny=1, xmin=1, ymin=1, sensor=sensor, track_static_delta=0,
                               seed=scene.seed if seed is None else int(seed))
    return Renderer(bare, device)


class Prepared(psf_probe.FieldPointLaunch):
    """The rows and the stamp of one launch resident on the device: call it to enqueue ims_psf_image, result() to fetch Stamps."""

    def __init__(self, renderer, rows, stage, size, scale, centre=None, inv_scale=None):
        check_stage(stage)
        r, torch = renderer, renderer.torch
        refuse_flux_operators(r.scene, stage)
        require_sensor(r.scene, stage)
        self.nx, self.ny = check_size(size)
        self.scale = check_scale(scale)
        # (inv_scale: an exact value for the device in place of the quotient formed here)
        self.inv_scale = 1.0 / self.scale if inv_scale is None else float(inv_scale)
        super().__init__(renderer, rows, stage, STAGES, centre)
        self.spec = _abi.PsfImage(self.nx, self.ny, self.inv_scale)
        self.counts = torch.zeros((max(self.n, 1), self.ny, self.nx), dtype=torch.int64, device=r.device)
        self.outside = torch.zeros(max(self.n, 1), dtype=torch.int64, device=r.device)
        self.dropped = torch.zeros(max(self.n, 1), dtype=torch.int64, device=r.device)

    def __call__(self):
        r = self.renderer
        _abi.check(r.lib.ims_psf_image(C.byref(self.params), self.stage, C.byref(self.spec), self.centre_ptr(), self.counts.data_ptr(),
                                       self.outside.data_ptr(), self.dropped.data_ptr(), r._stream()), "ims_psf_image")

    def result(self):
        counts, outside, dropped = self.fetch(self.counts, self.outside, self.dropped)
        return Stamps(counts=counts, n_used=counts.sum(axis=(1, 2)), n_outside=outside, n_dropped=dropped, scale=self.scale,
                      inv_scale=self.inv_scale, stage=self.stage_name, centre=self.centre)


def images(scene_or_psf, points, n_photons, size, scale, stage="psf", centre=None, wavelength=None, seed=None, device="cuda:0",
           renderer=None):
    """Stamps of the PSF the scene delivers at `points` -> Stamps.

    scene_or_psf, points, n_photons, wavelength, seed: as for psf_map.compute (points may be ready OBJECT_DTYPE rows, then
    n_photons may be None).  size: cells, an int or (nx, ny), 1 .. 512 each; scale: the side of a cell -- arcsec in stage "psf",
    pixels in stages "ops" and "sensor".  Stage "sensor" builds its rows as "ops" does and needs a scene with a sensor
    (ValueError otherwise).  centre: None or "nominal" -- the stamp is centred on the point's nominal position; "centroid" -- on
    the centroid psf_map.compute measures for the same rows (stage "sensor": at stage "ops", which the conversion leaves where it
    is on average for normal incidence); an [n][2] array -- on nominal + centre.  A chain with a BandpassRatio operator is
    refused in stages "ops" and "sensor" (ValueError): the counts are unweighted.  The stamp of a point depends on nothing but
    the point: not on the other points of the call, their order, or the launch."""
    check_stage(stage)
    nx, ny = check_size(size)
    scale = check_scale(scale)
    scene = psf_probe._as_scene(scene_or_psf)
    refuse_flux_operators(scene, stage)
    require_sensor(renderer.scene if renderer is not None else scene, stage)
    row_stage = "psf" if stage == "psf" else "ops"
    rows = psf_probe.probe_rows("psf_image", scene, points, n_photons, row_stage, wavelength)
    centre = psf_probe.resolve_centre("psf_image", centre)             # (a string is checked here, before anything ends the call)
    if len(rows) == 0:
        zeros = np.zeros(0, dtype=np.int64)
        return Stamps(np.zeros((0, ny, nx), dtype=np.int64), zeros, zeros, zeros, scale, 1.0 / scale, stage, None)
    r = renderer if renderer is not None else renderer_for(scene, stage, seed, device)
    run = Prepared(r, rows, stage, (nx, ny), scale, psf_probe.resolve_centre("psf_image", centre, scene, rows, row_stage, r))
    run()
    return run.result()


# ---------------- estimators on the counts ----------------
def surface_brightness(result):
    """counts per unit area per photon of the stamp -> f64 [n][ny][nx]: counts / (n_used scale^2), which sums to 1 / scale^2 over
    a stamp (NaN stamps where no photon arrived)"""
    c = np.asarray(result.counts, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return c / (np.asarray(result.n_used, dtype=np.float64)[:, None, None] * (result.scale * result.scale))


def cell_centres(n, scale):
    """the offsets of the n cell centres of one axis from the stamp's centre: (i + 1/2 - n / 2) scale"""
    return (np.arange(n, dtype=np.float64) + 0.5 - 0.5 * n) * scale


def moments(result):
    """Centroid and central second moments of every stamp, each photon taken at its cell's centre -> MOMENTS_DTYPE rows in the
    stage's units, relative to the stamp's centre: n (the photons in the stamp), xbar, ybar, Ixx, Iyy, Ixy, sigma =
    (Ixx Iyy - Ixy^2)^(1/4), e1, e2 as in psf_map.  Binning adds scale^2 / 12 to Ixx and Iyy of a smooth profile, and the
    stamp's edge cuts the halo off: these are the moments of the image, not of the photons.  NaN where the stamp is empty."""
    c = np.asarray(result.counts, dtype=np.float64)
    x, y = cell_centres(c.shape[2], result.scale), cell_centres(c.shape[1], result.scale)
    out = np.zeros(len(c), dtype=MOMENTS_DTYPE)
    n = c.sum(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(n > 0, n, np.nan)
        px, py = c.sum(axis=1), c.sum(axis=2)                          # [n][nx], [n][ny]
        xbar, ybar = (px * x).sum(axis=1) / w, (py * y).sum(axis=1) / w
        ux, uy = x[None, :] - xbar[:, None], y[None, :] - ybar[:, None]
        ixx, iyy = (px * ux * ux).sum(axis=1) / w, (py * uy * uy).sum(axis=1) / w
        ixy = (c * uy[:, :, None] * ux[:, None, :]).sum(axis=(1, 2)) / w
        tr = ixx + iyy
        out["sigma"] = np.sqrt(np.sqrt(ixx * iyy - ixy * ixy))
        out["e1"], out["e2"] = (ixx - iyy) / tr, 2.0 * ixy / tr
    out["n"], out["xbar"], out["ybar"], out["Ixx"], out["Iyy"], out["Ixy"] = n.astype(np.int64), xbar, ybar, ixx, iyy, ixy
    return out


# ---------------- output.psf_image ----------------
def parse_config(cfg, ev):
    """`output.psf_image: {file_name, dir, nx: 4, n_photons: 1000000, stage: psf | ops | sensor, size: 64, scale: <required>,
    centre: nominal | centroid}` -> the keywords of ccd_images.  size: an int or [nx, ny].  file_name and dir stay unevaluated:
    they may differ per CCD."""
    from .lsst_image import GalSimConfigError
    kw = psf_probe.parse_head("psf_image", cfg, ev, IMAGE_REQ, IMAGE_OPT, nx=4, n_photons=1000000, stages=STAGES, centre=True)
    size = cfg.get("size", 64)
    size = [ev.value(v) for v in size] if isinstance(size, (list, tuple)) else ev.value(size)
    try:
        if isinstance(size, float) and size != int(size):
            raise ValueError(f"psf_image: size must be an int or (nx, ny), not {size!r}")
        size = check_size(int(size) if isinstance(size, float) else size)
        scale = check_scale(ev.value(cfg["scale"]))
    except (TypeError, ValueError) as e:
        raise GalSimConfigError(f"output.{str(e).replace('psf_image: ', 'psf_image.', 1)}") from None
    return dict(kw, size=size, scale=scale)


def make_header(det_name, result, wavelength, n_photons, nx_ccd, ny_ccd, n, centre, sampled=False):
    """the probes' common cards (the CCD, the stage, the wavelength, NPHOT and the grid of the points' pixel positions: X_FIRST,
    X_STEP, Y_FIRST, Y_STEP, x fastest along axis 3), and the stamp: UNITS, SCALE, NX, NY, CENTRE"""
    h = psf_probe.probe_header(det_name, result.stage, wavelength, n_photons, nx_ccd, ny_ccd, n, sampled)
    h["stage"] = (str(result.stage), "psf: after the PSF; ops: + operators; sensor: + conversion")
    h["units"] = (UNITS[result.stage], "of SCALE")
    h["scale"] = (float(result.scale), "side of a cell; axis 1 is x, axis 2 is y")
    h["nx"] = (int(result.nx), "cells along x")
    h["ny"] = (int(result.ny), "cells along y")
    h["n_grid"] = (int(n), "points per CCD axis; axis 3 holds n_grid^2, x fastest")
    h["centre"] = (str(centre), "stamps centred on the nominal position or the centroid")
    return h


def summary(result, points):
    """f64 [n][5]: the point's pixel position x, y, and n_used, n_outside, n_dropped (the columns of SUMMARY; exact in f64)"""
    xy = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    return np.stack([xy[:, 0], xy[:, 1]] + [np.asarray(v, dtype=np.float64) for v in (result.n_used, result.n_outside, result.n_dropped)],
                    axis=1)


def write(file_name, hdus):
    """hdus: [(cube, header, summary, summary header)] per CCD -> two HDUs each: the counts as an f64 image [point][ny][nx]
    (exact for counts, psf_profile's number format) and a binary table SUMMARY, one row per point, with the columns of SUMMARY
    (x, y as doubles, the three counts as 64-bit integers)"""
    psf_probe.write_counts(file_name, hdus, SUMMARY)


def ccd_images(scene, det_name, nx, n_photons, stage, size, scale, centre="nominal", wavelength=None, wl_eff=None, device="cuda:0"):
    """The stamps of one CCD on psf_map's nx x nx grid over the scene's pixels: (cube, header, summary, summary header)"""
    pts = psf_probe.grid_points(scene.nx, scene.ny, nx)
    res = images(scene, pts, n_photons, size, scale, stage=stage, centre=centre, wavelength=wavelength, device=device)
    sampled = wavelength is None
    h = make_header(det_name, res, wl_eff if sampled else wavelength, n_photons, scene.nx, scene.ny, nx, centre, sampled)
    return res.counts.astype(np.float64), h, summary(res, pts), summary_header(det_name)
