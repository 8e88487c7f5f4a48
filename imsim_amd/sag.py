"""Surface sag maps: the `sag` extra output (imsim/sag.py).

For every interface of the telescope (perturbations included) one image of its sag -- the height of the surface along
its local z above its vertex plane, figure terms included -- on an nx x nx grid of local x, y over [-R_outer, R_outer],
NaN outside R_inner <= r <= R_outer and where the interface's obscuration blocks, with the surface's frame in the header
(origin x0, y0, z0 and the rotation R00 .. R22, telescope = origin + R local).  Host work only: a few hundred thousand
evaluations of the same sag the tracers use.
"""
import numpy as np

from . import fits_io, opd as opdmod, optics as opticsmod

HEADER_KEYS = ("units", "dx", "dy", "x0", "y0", "z0", "R00", "R01", "R02", "R10", "R11", "R12", "R20", "R21", "R22", "name",
               "telescop")


def surface_sag(S, x, y):
    """sag of surface S at local (x, y) [m]: conic + asphere + figure; NaN where the conic is not defined"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    z, _, ok = opticsmod._sag(S, x * x + y * y)
    fig = opticsmod.surface_figure_cartesian(S)
    if fig is not None:
        f, _, _ = opticsmod.poly2d_eval(fig[1], x * fig[0], y * fig[0], fig[0])
        z = z + f
    return np.where(ok, z, np.nan)


def compute(tel, nx=255):
    """[(array [nx, nx], header dict)]: one sag map per surface of `tel`, in the telescope's order"""
    nx = int(nx)
    if nx < 2:
        raise ValueError("sag: nx must be at least 2")
    xs = np.linspace(-1.0, 1.0, nx)
    out = []
    for S in tel.surfaces:
        try:
            outer, inner = S.radii()
        except ValueError:
            continue
        xx, yy = np.meshgrid(xs * outer, xs * outer)
        rr = np.hypot(xx, yy)
        arr = np.full((nx, nx), np.nan)
        w = (rr <= outer) & (rr >= inner)
        arr[w] = surface_sag(S, xx[w], yy[w])
        arr[opticsmod._obsc_vig(S, rr)] = np.nan
        dx = (xs[1] - xs[0]) * outer
        o, R = S.frame()
        h = {"units": ("m", "sag units"), "dx": (float(dx), "image scale (m)"), "dy": (float(dx), "image scale (m)"),
             "x0": (float(o[0]), "surface origin (m)"), "y0": (float(o[1]), "surface origin (m)"),
             "z0": (float(o[2]), "surface origin (m)")}
        for i in range(3):
            for j in range(3):
                h[f"R{i}{j}"] = (float(R[i, j]), "surface orientation matrix")
        h["name"] = (f"{tel.name}.{S.item_path}", None)
        h["telescop"] = (str(tel.name), None)
        out.append((arr, h))
    return out


def write(file_name, images):
    """one f64 image HDU per interface, the first one primary, with the maps' OffsetWCS (galsim.fits.writeMulti)"""
    hdus = []
    for arr, hdr in images:
        h = dict(hdr)
        h.update(opdmod.wcs_cards(arr.shape[1], float(hdr["dx"][0])))
        hdus.append((h, np.asarray(arr, dtype=np.float64)))
    fits_io.write_fits(file_name, hdus)

