"""Moments of the delivered PSF at a table of field points (`output.psf_map`; ims_psf_moments).

The photons of a point are the photons a render would shoot for it -- the PSF components of the scene (AtmosphericPSF with its
second kick and optical screen, Gaussian, Kolmogorov, DoubleGaussian) and, in stage "ops", the photon-operator chain up to the
position the sensor would receive -- but they are reduced on the GPU to six weighted sums and two counts per point instead of
being landed or stored.  This module holds the host half: the point rows, the launch, and the moments formed from the sums.

Units: stage "psf" leaves the offsets as the PSF kicks make them, in arcsec (+u west, +v north: the rows' local WCS is the
identity); stage "ops" gives focal-plane pixels of the scene's CCD relative to the point's pixel position."""
import ctypes as C
import dataclasses
import math
import os

import numpy as np

from . import _abi, fits_io
from ._abi import OBJECT_DTYPE

STAGES = {"psf": 1, "ops": 2}
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
MAP_OPT = ("dir", "nx", "n_photons", "stage")


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


def _as_scene(scene_or_psf):
    """a Scene as it is; a list of PSF component tuples becomes a scene of that PSF alone (stage "psf" only: no operators)"""
    from . import configs
    from .engine import Scene
    if isinstance(scene_or_psf, Scene):
        return scene_or_psf
    r2, cdf = configs.standard_tables()
    return Scene(nx=1, ny=1, psf=list(scene_or_psf), ops=[], radial_r2=r2, radial_cdf=cdf)


def point_rows(scene, xy, n_photons, stage="psf", wavelength=None):
    """Object rows for the pixel positions xy [n][2] of the scene's CCD: point sources of unit photon flux, point i on the random
    stream of object id i.  With a WCS on the scene's optics the rows carry the field angle of their position (the atmosphere's
    and the optical screen's `theta`) and, for stage "ops", the local WCS and the DCR angles a catalog object there would get;
    without one the points are on axis.  wavelength [nm]: None samples the scene's first wavelength table."""
    from . import configs
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n = len(xy)
    o = np.zeros(n, dtype=OBJECT_DTYPE)
    o["obj_id"] = np.arange(n)
    o["n_phot"] = np.broadcast_to(np.asarray(n_photons, dtype=np.int64), (n,))
    if np.any(o["n_phot"] < 0):
        raise ValueError("psf_map: negative photon count")
    o["x0"], o["y0"] = xy[:, 0], xy[:, 1]
    o["flux_per_photon"] = 1.0
    o["prof_table"], o["bf_state"] = _abi.IMS_PROF_POINT, -1
    o["jac"] = (1.0, 0.0, 0.0, 1.0)
    o["winv"] = (1.0, 0.0, 0.0, 1.0)
    lim = np.iinfo(np.int32)
    o["stamp_xmin"], o["stamp_xmax"], o["stamp_ymin"], o["stamp_ymax"] = lim.min, lim.max, lim.min, lim.max
    if wavelength is not None:
        o["sed_table"], o["sed_wave"] = -1, float(wavelength)
    elif scene.sed_tables is not None:
        o["sed_table"] = 0
    else:
        raise ValueError("psf_map: the scene has no wavelength table: give `wavelength`")
    optics = scene.optics
    has_wcs = optics is not None and getattr(optics, "img_wcs", None) is not None and getattr(optics, "icrf_to_field", None) is not None
    if has_wcs and n:
        o["atm_tan_x"], o["atm_tan_y"] = configs.field_angles(scene, xy[:, 0], xy[:, 1])
        if stage == "ops":
            winv, p0 = configs.local_wcs_inverse(optics.img_wcs, xy[:, 0], xy[:, 1])
            o["winv"] = winv
            v = configs.VISIT
            o["dcr_tanz"], o["dcr_sinp"], o["dcr_cosp"] = configs.dcr_angles(p0, math.radians(v["latitude"]), math.radians(v["hour_angle"]),
                                                                             math.radians(v["ra"]))
    return o


class Prepared:
    """The rows of one launch resident on the device: call it to enqueue ims_psf_moments, result() to fetch the moments."""

    def __init__(self, renderer, rows, stage):
        if stage not in STAGES:
            raise ValueError(f"psf_map: stage must be one of {sorted(STAGES)}, not {stage!r}")
        r, torch = renderer, renderer.torch
        self.renderer, self.stage = r, STAGES[stage]
        rows, self.obj_t, prefix, self.pre_t = r._upload_objects(rows)
        self.n, self.n_segments = len(rows), int(prefix[-1])
        self.photons = int(rows["n_phot"].sum())
        from .engine import _seg_ptr
        self.params = r.bound.params(self.obj_t.data_ptr(), self.n, self.pre_t.data_ptr(), self.n_segments, r.image.data_ptr(), None,
                                     _seg_ptr(self.pre_t))
        self.partial = torch.empty(max(8 * self.n_segments, 1), dtype=torch.float64, device=r.device)
        self.sums = torch.zeros((max(self.n, 1), 6), dtype=torch.float64, device=r.device)
        self.counts = torch.zeros((max(self.n, 1), 2), dtype=torch.int64, device=r.device)

    def __call__(self):
        r = self.renderer
        _abi.check(r.lib.ims_psf_moments(C.byref(self.params), self.stage, self.partial.data_ptr(), self.sums.data_ptr(),
                                         self.counts.data_ptr(), r._stream()), "ims_psf_moments")

    def raw(self):
        """(sums [n][6], counts [n][2]) on the host"""
        self.renderer.synchronize()
        return self.sums.cpu().numpy()[:self.n], self.counts.cpu().numpy()[:self.n]

    def result(self):
        return moments_from_sums(*self.raw())


def renderer_for(scene, seed=None, device="cuda:0"):
    """A renderer of the scene's PSF, operators and optics without its sensor (which neither stage reaches)"""
    from .engine import Renderer
    bare = dataclasses.replace(scene, nx=1, ny=1, xmin=1, ymin=1, sensor=None, track_static_delta=0,
                               seed=scene.seed if seed is None else int(seed))
    return Renderer(bare, device)


def compute(scene_or_psf, points, n_photons=None, stage="psf", wavelength=None, seed=None, device="cuda:0", renderer=None):
    """Moments of the PSF the scene delivers at `points`: MOMENTS_DTYPE rows, one per point, in the points' order.

    scene_or_psf: an engine.Scene, or a list of PSF component tuples (stage "psf" only).
    points: pixel positions [n][2] on the scene's CCD (rows made by point_rows), or ready OBJECT_DTYPE rows (n_photons None: the
    rows' own counts; phot_first is the base of the 64-bit photon index).
    stage: "psf" -- shoot + PSF, offsets in arcsec; "ops" -- also the scene's photon operators, focal-plane pixels relative to
    the point.  seed: the random seed (default: the scene's).  A point all of whose photons are vignetted has n_used 0 and NaN
    moments.  The result does not depend on which other points share the call, nor on their order."""
    if stage not in STAGES:
        raise ValueError(f"psf_map: stage must be one of {sorted(STAGES)}, not {stage!r}")
    scene = _as_scene(scene_or_psf)
    if isinstance(points, np.ndarray) and points.dtype.names is not None:
        rows = np.ascontiguousarray(points, dtype=OBJECT_DTYPE).copy()
        if n_photons is not None:
            rows["n_phot"] = np.broadcast_to(np.asarray(n_photons, dtype=np.int64), (len(rows),))
    else:
        if n_photons is None:
            raise ValueError("psf_map: n_photons is required with pixel positions")
        rows = point_rows(scene, points, n_photons, stage, wavelength)
    if len(rows) == 0:
        return np.zeros(0, dtype=MOMENTS_DTYPE)
    r = renderer if renderer is not None else renderer_for(scene, seed, device)
    run = Prepared(r, rows, stage)
    run()
    return run.result()


# ---------------- output.psf_map ----------------
def parse_config(cfg, ev):
    """`output.psf_map: {file_name, dir, nx: 8, n_photons: 100000, stage: psf}` -> (nx, n_photons, stage).  file_name and dir stay
    unevaluated: they may differ per CCD."""
    from .lsst_image import GalSimConfigError
    if not isinstance(cfg, dict):
        raise GalSimConfigError("output.psf_map must be a dict")
    for k in cfg:
        if k not in MAP_REQ and k not in MAP_OPT:
            raise GalSimConfigError(f"Unexpected attribute {k} found in output.psf_map")
    for k in MAP_REQ:
        if k not in cfg:
            raise GalSimConfigError(f"Attribute {k} is required in output.psf_map")
    nx = int(ev.value(cfg.get("nx", 8)))
    n_photons = int(ev.value(cfg.get("n_photons", 100000)))
    stage = str(ev.value(cfg.get("stage", "psf")))
    if nx < 1:
        raise GalSimConfigError("output.psf_map.nx must be at least 1")
    if n_photons < 1:
        raise GalSimConfigError("output.psf_map.n_photons must be at least 1")
    if stage not in STAGES:
        raise GalSimConfigError(f"output.psf_map.stage must be one of {sorted(STAGES)}, not {stage}")
    return dict(nx=nx, n_photons=n_photons, stage=stage)


def grid_points(nx_ccd, ny_ccd, n):
    """n x n pixel positions over a CCD of nx_ccd x ny_ccd pixels (pixel centres 1 .. nx_ccd): the centres of n x n equal
    cells, x fastest -> [n * n][2]"""
    gx = 0.5 + (np.arange(n) + 0.5) * (nx_ccd / n)
    gy = 0.5 + (np.arange(n) + 0.5) * (ny_ccd / n)
    X, Y = np.meshgrid(gx, gy)
    return np.stack([X.ravel(), Y.ravel()], axis=1)


def cube(moments, n):
    """MOMENTS_DTYPE rows of grid_points(.., n) -> f64 [plane][ny][nx], the planes in the order of PLANES"""
    return np.stack([np.asarray(moments[name], dtype=np.float64).reshape(n, n) for name, _ in PLANES])


def make_header(det_name, stage, wavelength, n_photons, nx_ccd, ny_ccd, n, sampled=False):
    """wavelength [nm]: the photons' one wavelength, or with sampled the effective wavelength of the bandpass they sample"""
    h = {"det_name": (str(det_name), "CCD"), "stage": (str(stage), "psf: arcsec after the PSF; ops: pixels after the operators"),
         "units": ("arcsec" if stage == "psf" else "pixel", "of the centroids; squared for the moments"),
         "wavelen": (float(wavelength), "(nm) effective; photons sample the bandpass" if sampled else "(nm) of every photon"),
         "nphot": (int(n_photons), "photons per point"),
         "x_first": (float(0.5 + 0.5 * nx_ccd / n), "CCD pixel x of the first column"), "x_step": (float(nx_ccd / n), "pixels per column"),
         "y_first": (float(0.5 + 0.5 * ny_ccd / n), "CCD pixel y of the first row"), "y_step": (float(ny_ccd / n), "pixels per row")}
    for k, (name, comment) in enumerate(PLANES, 1):
        h[f"PLANE{k}"] = (name, comment)
    return h


def write(file_name, hdus):
    """hdus: [(cube, header)], one image HDU per CCD, the first one primary"""
    os.makedirs(os.path.dirname(file_name) or ".", exist_ok=True)
    fits_io.write_fits(file_name, [(dict(h), np.asarray(c, dtype=np.float64)) for c, h in hdus])


def ccd_map(scene, det_name, nx, n_photons, stage, wavelength=None, wl_eff=None, device="cuda:0"):
    """The map of one CCD: (cube, header) for an nx x nx grid over the scene's pixels.  wavelength None: the photons sample the
    scene's bandpass, whose effective wavelength wl_eff goes into the header."""
    pts = grid_points(scene.nx, scene.ny, nx)
    m = compute(scene, pts, n_photons, stage=stage, wavelength=wavelength, device=device)
    sampled = wavelength is None
    return cube(m, nx), make_header(det_name, stage, wl_eff if sampled else wavelength, n_photons, scene.nx, scene.ny, nx, sampled)
