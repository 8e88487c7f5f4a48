"""Cosmic rays on the e-image (imsim/cosmic_rays.py:16-185): hits harvested from real dark frames, stored as footprints of
serial-direction spans in a FITS binary table (`data/cosmic_rays_itl_2017.fits.gz`, imSim's catalog), painted at random
places of the CCD -- the number per exposure Poisson distributed around exptime x ccd_rate x (image pixels / catalog
sensor pixels).

The reference paints span by span into a numpy array.  Here the hits are drawn on the host in the reference's order, and
`paint_hip` paints them on the device image with `ims_paint_cosmic_rays`: the catalog's spans are uploaded once, each hit is
(footprint, position), and hits whose footprints overlap go to later launches in draw order, so every pixel receives its adds
in the order numpy's would (bit-identical to `paint`, whatever the image values).  `paint_device` keeps the older form: the
span pixels flattened on the host and added in one scatter-add."""
import os
from collections import namedtuple, defaultdict

import numpy as np

from . import fits_io

CR_Span = namedtuple("CR_Span", "x0 y0 pixel_values".split())
DEFAULT_CATALOG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "cosmic_rays_itl_2017.fits.gz")
# the catalog the reference's LSST_CCD output defaults to, looked up in imSim's data directory (imsim/ccd.py:122-124)
REFERENCE_CATALOG = "cosmic_rays_LSSTCam_20260103.fits"


def find_catalog(name=None, data_dir=None):
    """Path of the cosmic-ray catalog `name` (as given, else under data_dir); without a name the packaged catalog, else the
    reference's default under data_dir.  FileNotFoundError when none exists, as imsim/ccd.py:125-126 raises."""
    if name:
        cand = [name] + ([os.path.join(data_dir, name)] if data_dir and not os.path.isabs(name) else [])
    else:
        cand = [DEFAULT_CATALOG] + ([os.path.join(data_dir, REFERENCE_CATALOG)] if data_dir else [])
    for c in cand:
        if os.path.isfile(c):
            return c
    raise FileNotFoundError(f"{name or REFERENCE_CATALOG} not found")


def ccd_rng(seed_ccd):
    """the random stream of one CCD's cosmic rays: seeded by the CCD's seed, apart from its other streams"""
    return np.random.default_rng([int(seed_ccd), 0x4352])


def hit_layers(r0, r1, c0, c1):
    """Layer of each hit, given its bounding box [r0, r1) x [c0, c1) in draw order: one more than the highest layer of the
    earlier hits it overlaps (0 if none).  Hits of one layer are disjoint, and a pixel covered by several hits gets them
    in draw order when the layers are painted in turn."""
    n = len(r0)
    layer = np.zeros(n, dtype=np.int64)
    for k in range(1, n):
        ov = (r0[:k] < r1[k]) & (r0[k] < r1[:k]) & (c0[:k] < c1[k]) & (c0[k] < c1[:k])
        if ov.any():
            layer[k] = layer[:k][ov].max() + 1
    return layer


class CosmicRays(list):
    """Each element is one cosmic ray: a list of CR_Span(x0, y0, pixel_values).  Attributes num_pix (pixels of the
    sensors the hits were taken from), exptime (summed dark time [s]), ccd_rate (hits per second per CCD)."""

    def __init__(self, ccd_rate=None, catalog_file=DEFAULT_CATALOG):
        super().__init__()
        self._read_catalog(catalog_file, ccd_rate)

    @classmethod
    def read_catalog(cls, catalog_file, ccd_rate=None, extname="COSMIC_RAYS"):
        ret = cls.__new__(cls)
        list.__init__(ret)
        ret._read_catalog(catalog_file, ccd_rate, extname=extname)
        return ret

    def _read_catalog(self, catalog_file, ccd_rate, extname="COSMIC_RAYS"):
        table = None
        for hdr, data in fits_io.read_fits(catalog_file):
            if hdr.get("XTENSION") == "BINTABLE" and str(hdr.get("EXTNAME", "")).strip() == extname:
                table, header = data, hdr
        if table is None:
            raise OSError(f"no {extname} table in {catalog_file}")
        self.num_pix = header["NUM_PIX"]
        self.exptime = header["EXPTIME"]
        crs = defaultdict(list)
        for fp, x0, y0, vals in zip(table["fp_id"], table["x0"], table["y0"], table["pixel_values"]):
            crs[int(fp)].append(CR_Span(int(x0), int(y0), np.asarray(vals)))
        self.extend(crs.values())
        self.ccd_rate = float(len(self)) / self.exptime if ccd_rate is None else ccd_rate

    # -- the reference's array interface (used by its tests) --
    def paint_cr(self, image_array, rng, index=None, pixel=None):
        if index is None:
            index = int(rng.random() * len(self))
        cr = self[index]
        if pixel is None:
            pixel = (int(rng.random() * image_array.shape[1]), int(rng.random() * image_array.shape[0]))
        for span in cr:
            for dx, value in enumerate(span.pixel_values):
                row, col = pixel[1] + span.y0 - cr[0].y0, pixel[0] + span.x0 - cr[0].x0 + dx
                if 0 <= row < image_array.shape[0] and 0 <= col < image_array.shape[1]:
                    image_array[row, col] += value
        return image_array

    def draw(self, shape, rng, exptime=30.0, num_crs=None):
        """[hit][catalog index, x, y] of this exposure's hits on an image of `shape`, in the reference's draw order
        (imsim/cosmic_rays.py:44-110): the Poisson count from exptime x ccd_rate x the image's share of the catalog sensors'
        pixels, then per hit its catalog index and its position"""
        ny, nx = shape
        if num_crs is None:
            num_crs = int(rng.poisson(exptime * self.ccd_rate * float(nx * ny) / self.num_pix))
        hits = np.zeros((num_crs, 3), dtype=np.int64)
        for k in range(num_crs):
            index = int(rng.random() * len(self))
            hits[k] = index, int(rng.random() * nx), int(rng.random() * ny)
        return hits

    def draw_hits(self, shape, rng, exptime=30.0, num_crs=None):
        """(flat pixel index, electrons) of every span pixel of this exposure's hits that falls on an image of `shape`"""
        ny, nx = shape
        idx, val = [], []
        for index, px, py in self.draw(shape, rng, exptime, num_crs):
            cr = self[int(index)]
            for span in cr:
                row = py + span.y0 - cr[0].y0
                cols = px + span.x0 - cr[0].x0 + np.arange(len(span.pixel_values))
                ok = (cols >= 0) & (cols < nx) & (0 <= row < ny)
                idx.append(row * nx + cols[ok])
                val.append(np.asarray(span.pixel_values, dtype=np.float64)[ok])
        if not idx:
            return np.zeros(0, dtype=np.int64), np.zeros(0)
        return np.concatenate(idx).astype(np.int64), np.concatenate(val)

    def paint(self, image_array, rng, exptime=30.0, num_crs=None):
        idx, val = self.draw_hits(image_array.shape, rng, exptime, num_crs)
        np.add.at(image_array.reshape(-1), idx, val)
        return image_array

    def paint_device(self, image_dev, rng, exptime=30.0, num_crs=None):
        """the same on a [ny][nx] float64 device tensor: one scatter-add"""
        import torch
        idx, val = self.draw_hits(tuple(image_dev.shape), rng, exptime, num_crs)
        if len(idx):
            image_dev.view(-1).index_add_(0, torch.from_numpy(idx).to(image_dev.device), torch.from_numpy(val).to(image_dev.device))
        return len(idx)

    def device_tables(self, device):
        """The catalog on `device`, uploaded once: spans (ims_cr_span_t rows, relative to each footprint's first span),
        values (f64) and per footprint its spans, pixel count and bounding box.  A footprint that covers a pixel twice is
        painted span by span (each span its own hit), so that no two lanes of one launch add to the same pixel."""
        import torch
        from . import _abi
        key = str(torch.device(device))
        cache = self.__dict__.setdefault("_device_tables", {})
        if key in cache:
            return cache[key]
        n_spans = [len(cr) for cr in self]
        spans = np.zeros(sum(n_spans), dtype=_abi.CR_SPAN_DTYPE)
        values, bbox, n_pix, self_overlap = [], np.zeros((len(self), 4), dtype=np.int64), np.zeros(len(self), np.int64), []
        k, v = 0, 0
        for f, cr in enumerate(self):
            pix, seen = 0, set()
            overlap = False
            for span in cr:
                n = len(span.pixel_values)
                row, col = span.y0 - cr[0].y0, span.x0 - cr[0].x0
                spans[k] = (row, col, n, pix, v)
                for c in range(col, col + n):
                    overlap |= (row, c) in seen
                    seen.add((row, c))
                values.append(np.asarray(span.pixel_values, dtype=np.float64))
                pix, k, v = pix + n, k + 1, v + n
            n_pix[f] = pix
            rows = spans["row"][k - len(cr):k]
            cols, ends = spans["col"][k - len(cr):k], spans["col"][k - len(cr):k] + spans["n"][k - len(cr):k]
            bbox[f] = rows.min(), rows.max() + 1, cols.min(), ends.max()
            self_overlap.append(overlap)
        first = np.concatenate([[0], np.cumsum(n_spans)[:-1]]).astype(np.int64)
        vals = np.concatenate(values) if values else np.zeros(1)
        t = dict(spans=spans, first=first, n_spans=np.asarray(n_spans, np.int64), n_pix=n_pix, bbox=bbox,
                 self_overlap=np.asarray(self_overlap, bool),
                 spans_dev=torch.from_numpy(spans.view(np.uint8).copy()).to(device),
                 values_dev=torch.from_numpy(vals).to(device), n_values=len(vals))
        cache[key] = t
        return t

    def hit_table(self, hits, device):
        """the ims_cr_hit_t rows of drawn hits ([hit][catalog index, x, y]) and the layer offsets of ims_paint_cosmic_rays"""
        from . import _abi
        t = self.device_tables(device)
        rows = []                               # (footprint first span, n spans, n pixels, x0, y0, r0, r1, c0, c1)
        for f, x, y in np.asarray(hits, dtype=np.int64).reshape(-1, 3):
            if not t["self_overlap"][f]:
                b = t["bbox"][f]
                rows.append((t["first"][f], t["n_spans"][f], t["n_pix"][f], x, y, y + b[0], y + b[1], x + b[2], x + b[3]))
                continue
            for s in range(t["first"][f], t["first"][f] + t["n_spans"][f]):
                sp = t["spans"][s]
                rows.append((s, 1, sp["n"], x, y, y + sp["row"], y + sp["row"] + 1, x + sp["col"], x + sp["col"] + sp["n"]))
        r = np.asarray(rows, dtype=np.int64).reshape(-1, 9)
        layer = hit_layers(r[:, 5], r[:, 6], r[:, 7], r[:, 8])
        order = np.argsort(layer, kind="stable")
        table = np.zeros(len(r), dtype=_abi.CR_HIT_DTYPE)
        table["first_span"], table["n_spans"], table["n_pixels"] = r[order, 0], r[order, 1], r[order, 2]
        table["x0"], table["y0"] = r[order, 3], r[order, 4]
        n_layers = int(layer.max()) + 1 if len(layer) else 0
        layer_first = np.searchsorted(layer[order], np.arange(n_layers + 1)).astype(np.int64)
        return table, layer_first

    def paint_hip(self, image_dev, rng, exptime=30.0, num_crs=None):
        """`paint` on a [ny][nx] f64 device tensor (ims_paint_cosmic_rays), bit-identical to it for the same rng state.
        Returns the drawn hits, [hit][catalog index, x, y]."""
        import ctypes as C
        import torch
        from . import _abi
        if image_dev.dtype != torch.float64 or image_dev.dim() != 2 or not image_dev.is_contiguous() or image_dev.device.type != "cuda":
            raise ValueError("paint_hip: the image must be a contiguous [ny][nx] float64 device tensor")
        ny, nx = image_dev.shape
        hits = self.draw((ny, nx), rng, exptime, num_crs)
        if not len(hits):
            return hits
        t = self.device_tables(image_dev.device)
        table, layer_first = self.hit_table(hits, image_dev.device)
        hits_dev = torch.from_numpy(table.view(np.uint8).copy()).to(image_dev.device)
        lib = _abi.load()
        stream = torch.cuda.current_stream(image_dev.device).cuda_stream
        _abi.check(lib.ims_paint_cosmic_rays(image_dev.data_ptr(), nx, ny, t["spans_dev"].data_ptr(), len(t["spans"]),
                                             t["values_dev"].data_ptr(), t["n_values"], hits_dev.data_ptr(),
                                             (C.c_int64 * len(layer_first))(*layer_first.tolist()), len(layer_first) - 1, stream),
                   "ims_paint_cosmic_rays")
        return hits


def write_cosmic_ray_catalog(fp_id, x0, y0, pixel_values, exptime, num_pix, outfile="cosmic_ray_catalog.fits", overwrite=True):
    """FITS binary table of footprint spans (imsim/cosmic_rays.py:147-185)"""
    if os.path.exists(outfile) and not overwrite:
        raise OSError(f"{outfile} exists")
    cols = [("fp_id", "J", np.asarray(fp_id)), ("x0", "I", np.asarray(x0)), ("y0", "I", np.asarray(y0)),
            ("pixel_values", "PJ()", list(pixel_values))]
    with open(outfile, "wb") as f:
        f.write(fits_io.hdu_bytes({}, None, primary=True))
        f.write(fits_io.bintable_hdu_bytes(cols, header=[("EXPTIME", exptime), ("NUM_PIX", num_pix)], extname="COSMIC_RAYS"))
