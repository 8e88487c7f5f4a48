"""The host half the PSF probes share (psf_map, psf_profile, psf_image).

A probe shoots the photons a render would shoot for a table of field points and reduces them on the GPU instead of landing them.
What differs between two probes is the reduction: its kernel, its buffers and the estimators formed from them.  Everything else is
here, and a new probe starts from it: the point rows (probe_rows), the launch base that holds them on the device
(FieldPointLaunch), the centre the offsets are taken from (resolve_centre), the refusal of chains with unequal photon flux
(refuse_flux_operators), the common head of an `output.*` key (parse_head) and the counts-cube file (probe_header, summary_header,
write_counts)."""
import dataclasses
import math
import os

import numpy as np

from . import _abi, fits_io
from ._abi import OBJECT_DTYPE

STAGES = {"psf": 1, "ops": 2}


def check_stage(probe, stage, stages=STAGES):
    if stage not in stages:
        raise ValueError(f"{probe}: stage must be one of {sorted(stages)}, not {stage!r}")


def _as_scene(scene_or_psf):
    """a Scene as it is; a list of PSF component tuples becomes a scene of that PSF alone (stage "psf" only: no operators)"""
    from . import configs
    from .engine import Scene
    if isinstance(scene_or_psf, Scene):
        return scene_or_psf
    r2, cdf = configs.standard_tables()
    return Scene(nx=1, ny=1, psf=list(scene_or_psf), ops=[], radial_r2=r2, radial_cdf=cdf)


def renderer_for(scene, seed=None, device="cuda:0"):
    """A renderer of the scene's PSF, operators and optics without its sensor (which stages "psf" and "ops" do not reach)"""
    from .engine import Renderer
    bare = dataclasses.replace(scene, nx=1, ny=1, xmin=1, ymin=1, sensor=None, track_static_delta=0,
                               seed=scene.seed if seed is None else int(seed))
    return Renderer(bare, device)


def grid_points(nx_ccd, ny_ccd, n):
    """n x n pixel positions over a CCD of nx_ccd x ny_ccd pixels (pixel centres 1 .. nx_ccd): the centres of n x n equal
    cells, x fastest -> [n * n][2]"""
    gx = 0.5 + (np.arange(n) + 0.5) * (nx_ccd / n)
    gy = 0.5 + (np.arange(n) + 0.5) * (ny_ccd / n)
    X, Y = np.meshgrid(gx, gy)
    return np.stack([X.ravel(), Y.ravel()], axis=1)


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


def probe_rows(probe, scene, points, n_photons, row_stage, wavelength=None):
    """The OBJECT_DTYPE rows of a probe's call.  points: ready rows (a copy is made; n_photons None keeps the rows' own counts), or
    pixel positions [n][2] on the scene's CCD, which point_rows turns into rows for row_stage and for which n_photons is required"""
    if isinstance(points, np.ndarray) and points.dtype.names is not None:
        rows = np.ascontiguousarray(points, dtype=OBJECT_DTYPE).copy()
        if n_photons is not None:
            rows["n_phot"] = np.broadcast_to(np.asarray(n_photons, dtype=np.int64), (len(rows),))
        return rows
    if n_photons is None:
        raise ValueError(f"{probe}: n_photons is required with pixel positions")
    return point_rows(scene, points, n_photons, row_stage, wavelength)


def resolve_centre(probe, centre, scene=None, rows=None, row_stage=None, renderer=None):
    """The centre a probe takes its offsets from, as its launch wants it: None (the point's nominal position) or f64 [n][2]
    (nominal + centre).  centre: None, "nominal", "centroid" -- the centroid psf_map.compute measures for the same rows at
    row_stage on `renderer` -- or an [n][2] array, which passes through.  Any other string is a ValueError.  Without a renderer
    "centroid" is checked and left as it is: the probes do that before anything else can end the call, then come back with one."""
    if not isinstance(centre, str):
        return centre
    if centre not in ("nominal", "centroid"):
        raise ValueError(f"{probe}: centre must be 'nominal', 'centroid' or an [n][2] array, not {centre!r}")
    if centre == "nominal":
        return None
    if renderer is None:
        return centre
    from . import psf_map
    m = psf_map.compute(scene, rows, stage=row_stage, renderer=renderer)
    return np.stack([m["xbar"], m["ybar"]], axis=1)                  # (NaN where no photon arrived: that row has nothing to bin)


def refuse_flux_operators(probe, noun, stages, scene, stage):
    """A probe that counts photons unweighted cannot reduce a chain whose photons leave with unequal flux.  stages: the stages
    that run the chain; noun: what counts ("profile", "stamp")"""
    if stage in stages:
        for op in getattr(scene, "ops", None) or []:
            if int(op[0]) == _abi.IMS_OP_BANDPASS_RATIO:
                raise ValueError(f"{probe}: the photon-operator chain holds a BandpassRatio operator, whose photons carry unequal "
                                 f"flux; the {noun} counts photons unweighted")


class FieldPointLaunch:
    """The rows of one launch resident on the device, with the render parameters that address them; a probe's Prepared class adds
    its own buffers, its __call__ and its result().  stages: the probe's table, stage name -> the entry point's code (the caller
    has checked the name).  centre: None or [n][2], kept as `centre` and, on the device, `centre_t`."""

    def __init__(self, renderer, rows, stage, stages=STAGES, centre=None):
        from .engine import _seg_ptr
        r = renderer
        self.renderer, self.stage, self.stage_name = r, stages[stage], stage
        rows, self.obj_t, prefix, self.pre_t = r._upload_objects(rows)
        self.n, self.n_segments = len(rows), int(prefix[-1])
        self.photons = int(rows["n_phot"].sum())
        self.params = r.bound.params(self.obj_t.data_ptr(), self.n, self.pre_t.data_ptr(), self.n_segments, r.image.data_ptr(), None,
                                     _seg_ptr(self.pre_t))
        self.centre = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64).reshape(self.n, 2)
        self.centre_t = None if self.centre is None else r.torch.from_numpy(self.centre).to(r.device)

    def centre_ptr(self):
        return None if self.centre_t is None else self.centre_t.data_ptr()

    def fetch(self, *tensors):
        """the tensors' first n rows on the host, after the stream has drained"""
        self.renderer.synchronize()
        return tuple(t.cpu().numpy()[:self.n] for t in tensors)


# ---------------- the common head of an `output.*` key ----------------
def parse_head(name, cfg, ev, req, opt, nx, n_photons, stages=STAGES, centre=False):
    """The checks and values every probe's `output.<name>` shares: cfg is a dict of the keys req + opt with all of req;
    nx (default nx) and n_photons (default n_photons) at least 1; stage (default psf) one of stages; with centre, `centre`
    (default nominal) nominal or centroid -> dict(nx, n_photons, stage[, centre])"""
    from .lsst_image import GalSimConfigError
    if not isinstance(cfg, dict):
        raise GalSimConfigError(f"output.{name} must be a dict")
    for k in cfg:
        if k not in req and k not in opt:
            raise GalSimConfigError(f"Unexpected attribute {k} found in output.{name}")
    for k in req:
        if k not in cfg:
            raise GalSimConfigError(f"Attribute {k} is required in output.{name}")
    kw = dict(nx=int(ev.value(cfg.get("nx", nx))), n_photons=int(ev.value(cfg.get("n_photons", n_photons))),
              stage=str(ev.value(cfg.get("stage", "psf"))))
    if centre:
        kw["centre"] = str(ev.value(cfg.get("centre", "nominal")))
    if kw["nx"] < 1:
        raise GalSimConfigError(f"output.{name}.nx must be at least 1")
    if kw["n_photons"] < 1:
        raise GalSimConfigError(f"output.{name}.n_photons must be at least 1")
    if kw["stage"] not in stages:
        raise GalSimConfigError(f"output.{name}.stage must be one of {sorted(stages)}, not {kw['stage']}")
    if centre and kw["centre"] not in ("nominal", "centroid"):
        raise GalSimConfigError(f"output.{name}.centre must be nominal or centroid, not {kw['centre']}")
    return kw


# ---------------- the files ----------------
def probe_header(det_name, stage, wavelength, n_photons, nx_ccd, ny_ccd, n, sampled=False):
    """The cards every probe's image HDU starts with: the CCD, the stage and its units, the wavelength, the photons per point and
    the grid of the points' pixel positions.  wavelength [nm]: the photons' one wavelength, or with sampled the effective
    wavelength of the bandpass they sample."""
    return {"det_name": (str(det_name), "CCD"), "stage": (str(stage), "psf: arcsec after the PSF; ops: pixels after the operators"),
            "units": ("arcsec" if stage == "psf" else "pixel", "of the centroids; squared for the moments"),
            "wavelen": (float(wavelength), "(nm) effective; photons sample the bandpass" if sampled else "(nm) of every photon"),
            "nphot": (int(n_photons), "photons per point"),
            "x_first": (float(0.5 + 0.5 * nx_ccd / n), "CCD pixel x of the first column"), "x_step": (float(nx_ccd / n), "pixels per column"),
            "y_first": (float(0.5 + 0.5 * ny_ccd / n), "CCD pixel y of the first row"), "y_step": (float(ny_ccd / n), "pixels per row")}


def summary_header(det_name):
    return {"det_name": (str(det_name), "CCD")}


def write_counts(file_name, hdus, summary_names):
    """hdus: [(cube, header, summary, summary header)] per CCD -> two HDUs each: the counts as an f64 image (exact for counts) and
    a binary table SUMMARY, one row per point, with the columns summary_names: those named n_* as 64-bit integers, the others
    as doubles"""
    os.makedirs(os.path.dirname(file_name) or ".", exist_ok=True)
    with open(file_name, "wb") as fobj:
        for k, (cube, h, s, sh) in enumerate(hdus):
            fobj.write(fits_io.hdu_bytes(dict(h), np.asarray(cube, dtype=np.float64), primary=(k == 0)))
            s = np.asarray(s, dtype=np.float64).reshape(-1, len(summary_names))
            cols = [(name, "K" if name.startswith("n_") else "D", s[:, j].astype(np.int64) if name.startswith("n_") else s[:, j])
                    for j, name in enumerate(summary_names)]
            fobj.write(fits_io.bintable_hdu_bytes(cols, header=dict(sh), extname="SUMMARY"))
