"""Per-CCD catalogs of the `output` section: `truth` (GalSim's TruthBuilder: imSim's centroid file,
config/imsim-config.yaml:370-392), `photon_pooling_truth` (imsim/photon_pooling.py:472-510, the same columns with
incident_flux) and `process_info` (imsim/process_info.py).

The rows are the objects the CCD drew (one per object of the truth record config.Process keeps: faint and FFT-drawn ones
included, the ones skipped for zero realized flux not), in catalog order.  The column expressions of the templates are
evaluated once over whole columns: `@name` is a per-object quantity (object_id, nominal_flux, phot_flux, fft_flux,
realized_flux / incident_flux), `$expr` is Python over `image_pos` (x, y), `sky_pos` / `world_pos` (ra, dec as angles
with .deg / .rad, from the CCD's WCS), those quantities and the config's variables.  An expression that cannot be evaluated
is a config error naming the column.

Files are written as galsim.OutputCatalog writes text: a `#` header of the column names, one row per object, 16-wide
fields (floats as %.8e), gzip-compressed when the name ends in .gz."""
import math
import os
import time
import types

import numpy as np

from .lsst_image import GalSimConfigError

TRUTH_KEYS = ("file_name", "dir", "columns")
PROCESS_INFO_KEYS = ("file_name", "dir")
PROCESS_INFO_COLUMNS = ("object_id", "pid", "rss", "uss", "user_time", "unix_time")
FLUX_FIELDS = ("nominal_flux", "phot_flux", "fft_flux", "realized_flux", "incident_flux")
PREC = 8


def parse(cfg, what, keys=TRUTH_KEYS):
    """An extra-output section: None when it is switched off ("" as the pooling template sets output.truth, or no
    file_name, which GalSim skips), else the dict after checking its keys"""
    if cfg in ("", None):
        return None
    if not isinstance(cfg, dict):
        raise GalSimConfigError(f"output.{what} must be a dict")
    for k in cfg:
        if k not in keys:
            raise GalSimConfigError(f"Unexpected attribute {k} found in output.{what}")
    if "columns" in keys and not isinstance(cfg.get("columns", {}), dict):
        raise GalSimConfigError(f"output.{what}.columns must be a dict of name: value")
    if cfg.get("file_name") in ("", None):
        return None
    return cfg


def file_name(cfg, ev, out):
    """dir (else output.dir) + file_name, evaluated for the CCD whose variables ev holds"""
    fn = os.path.join(str(ev.value(cfg.get("dir", out.get("dir", "")))), str(ev.value(cfg["file_name"])))
    if os.path.splitext(fn[:-3] if fn.endswith(".gz") else fn)[1].lower().startswith(".fit"):
        raise GalSimConfigError(f"{fn}: truth catalogs are written as text (.txt, .txt.gz)")
    return fn


class _Angle(np.ndarray):
    """a column of angles [rad] with .deg / .rad, as galsim.Angle offers them"""

    def __new__(cls, rad):
        return np.asarray(rad, dtype=np.float64).view(cls)

    @property
    def rad(self):
        return np.asarray(self)

    @property
    def deg(self):
        return np.degrees(np.asarray(self))


def object_columns(truth, cat, img_wcs):
    """the per-object quantities of a CCD's truth record (config.Process's res.truth entry) and its catalog"""
    from . import wcs as wcsmod
    idx = np.asarray(truth["index"], dtype=np.int64)
    x, y = np.asarray(truth["x"], dtype=np.float64), np.asarray(truth["y"], dtype=np.float64)
    cols = {"object_id": np.asarray(cat["object_id"])[idx].astype(str)}
    for k in FLUX_FIELDS:
        if k in truth:
            cols[k] = np.asarray(truth[k], dtype=np.float64)
    if len(x):
        v = wcsmod.tansip_pix_to_vec(img_wcs, x, y)
        ra, dec = np.arctan2(v[:, 1], v[:, 0]) % (2.0 * math.pi), np.arcsin(np.clip(v[:, 2], -1.0, 1.0))
    else:
        ra = dec = np.zeros(0)
    sky = types.SimpleNamespace(ra=_Angle(ra), dec=_Angle(dec))
    cols["_image_pos"], cols["_sky_pos"] = types.SimpleNamespace(x=x, y=y), sky
    return cols


def evaluate_columns(columns, objs, ev):
    """{name: expression} -> {name: column of len(object_id)}"""
    n = len(objs["object_id"])
    ns = {k: v for k, v in objs.items() if not k.startswith("_")}
    ns.update(image_pos=objs["_image_pos"], sky_pos=objs["_sky_pos"], world_pos=objs["_sky_pos"])
    out = {}
    for name, expr in columns.items():
        try:
            if isinstance(expr, str) and expr.startswith("@") and expr[1:] in ns:
                val = ns[expr[1:]]
            elif isinstance(expr, str) and expr.startswith("$"):
                saved = dict(ev.vars)
                ev.vars.update(ns)
                try:
                    val = ev.value(expr)
                finally:
                    ev.vars.clear()
                    ev.vars.update(saved)
            else:
                val = ev.value(expr)
            if isinstance(val, dict) or isinstance(val, types.SimpleNamespace):
                raise TypeError(f"not a value: {val!r}")
            val = np.asarray(val)
            if val.ndim == 0:
                val = np.full(n, val[()])
            if val.shape != (n,) or val.dtype.kind not in "biufUS":
                raise TypeError(f"gives {val.dtype} of shape {val.shape} for {n} objects")
        except GalSimConfigError:
            raise
        except Exception as e:                                  # noqa: BLE001 -- any failure of the user's expression
            raise GalSimConfigError(f"truth column {name}: cannot evaluate {expr!r} ({type(e).__name__}: {e})") from None
        out[str(name)] = val
    return out


def write(fn, columns, prec=PREC):
    """galsim.OutputCatalog.writeAscii: header '# ' + the names centred in prec+8 columns; integers %{w}d, floats
    %{w}.{prec}e, strings %{w}s; numpy gzips a name ending in .gz"""
    names = list(columns)
    n = len(next(iter(columns.values()))) if names else 0
    width = prec + 8
    dtype, fmt = [], []
    for k in names:
        v = np.asarray(columns[k])
        if v.dtype.kind in "biu":
            dtype.append((k, np.int64))
            fmt.append(f"%{width}d")
        elif v.dtype.kind == "f":
            dtype.append((k, np.float64))
            fmt.append(f"%{width}.{prec}e")
        else:
            v = v.astype(str)
            dtype.append((k, f"U{max(1, max((len(s) for s in v), default=1))}"))
            fmt.append(f"%{width}s")
    data = np.zeros(n, dtype=dtype)
    for k in names:
        data[k] = columns[k]
    header = " ".join(f"{k:^{width}}" for k in names) + " "
    os.makedirs(os.path.dirname(fn) or ".", exist_ok=True)
    np.savetxt(fn, data, fmt=fmt, header=header)


def read(fn):
    """a catalog written by `write`: {name: column}, object_id as strings, the other columns int64 or float64"""
    import gzip
    with (gzip.open(fn, "rt") if fn.endswith(".gz") else open(fn)) as f:
        names = f.readline().lstrip("#").split()
        rows = [line.split() for line in f if line.strip()]
    out = {}
    for j, k in enumerate(names):
        v = [r[j] for r in rows]
        if k == "object_id":
            out[k] = np.array(v, dtype=str)
        else:
            out[k] = np.array(v, dtype=np.int64 if all(s.lstrip("-").isdigit() for s in v) and v else np.float64)
    return out


def process_info_columns(object_id):
    """imsim/process_info.py's columns for the CCD's objects.  Per-object figures cannot be taken inside a batched GPU
    render: one measurement of this process, taken when the CCD is done, is repeated on every row."""
    try:
        import psutil
    except ImportError:
        raise GalSimConfigError("output.process_info needs the psutil package") from None
    proc = psutil.Process(os.getpid())
    mem = proc.memory_full_info()
    n = len(object_id)
    return {"object_id": np.asarray(object_id).astype(str), "pid": np.full(n, os.getpid(), dtype=np.int64),
            "rss": np.full(n, mem.rss / 1024 ** 3), "uss": np.full(n, mem.uss / 1024 ** 3),
            "user_time": np.full(n, float(proc.cpu_times().user)), "unix_time": np.full(n, time.time())}
