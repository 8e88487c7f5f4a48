"""Planted inputs of the spike step, shared by tests/test_spike_ref.py (CPU: the oracle against tests/spike_ref.py) and
tests/test_fft_spikes_gpu.py (the kernels against both).  The spike constants go straight into _abi.Spikes -- cos0, sin0, a_lo,
d_alpha from alpha = pi/4 - rot the way the host forms them, scale 577.6 / 622.2, norm the host's stencil_norm --, the
ims_fft_object_t rows and their prefix sums are made by hand, and the real-space buffers are a background of uniform(-2, 10)
(the negatives exercise the clip) with saturated pixels of 2e5 .. 4e5 over a threshold of 1e5.  No FFT draw, no grid above 96."""
import math

import numpy as np

from imsim_amd import _abi, diffraction_fft as dfft

THRESHOLD = 1.0e5
SCALE = 577.6 / 622.2
SEED = 20261020
EMPTY_BOX = (0x7fffffff, -1, 0x7fffffff, -1)

# name -> (rot, d_alpha).  `diagonal` and `axis_swept` sit a few 1e-3 rad off rot = 0 and pi/4: at those angles exactly the offsets
# on the diagonals (axes) lie on the wedge's edge to rounding and a quarter of the stencil would be "near a decision"
# (tests/spike_ref.py).  axis_dyadic is the geometry on which they lie on it EXACTLY, provably (the `<=` of the wedge test).
GEOMETRIES = {
    "near_axis": (math.radians(40.04), 2.2e-3),       # the control of the existing tests
    "generic": (0.698, 2.2e-3),                       # arms between axes and diagonals
    "diagonal": (3.0e-3, 2.2e-3),                     # |cos0| ~ |sin0|, two arms through every row
    "axis_exact": (math.pi / 4, 0.0),                 # sin0 == 0.0: has_s false; table row a = 0 holds 2 cutoff + 1 entries
    "axis_swept": (math.pi / 4 + 2.0e-3, 0.04),       # rows far longer than 16 entries next to the axes
    "axis_dyadic": (math.pi / 4, 2.0 ** -5),          # dth == d_alpha exactly on the four half-axes
    "negative": (2.1, -2.2e-3),                       # the wedge never fires, arc < 0
    "wide": (1.3, 0.3),                               # the wedge dominates the stencil and the zero-sum pruning margin
}

SHAPES = {
    "clip64": tuple(GEOMETRIES),
    "long32": tuple(GEOMETRIES),
    "edge96": ("generic", "axis_exact", "diagonal"),
    "wide_box": ("generic", "axis_swept"),
    "batch": ("generic", "axis_swept", "negative"),
}
CUTOFF = {"clip64": 20, "long32": 200, "edge96": 60, "wide_box": 8, "batch": 24}
CASES = [(shape, geom) for shape, geoms in SHAPES.items() for geom in geoms]

_NORMS = {}


def spikes(geom, cutoff):
    """the ims_spikes_t block of a geometry (no table: tab_* NULL)"""
    rot, d_alpha = GEOMETRIES[geom]
    alpha = math.pi / 4.0 - rot
    cos0, sin0 = math.cos(alpha - d_alpha / 2.0), math.sin(alpha - d_alpha / 2.0)
    if geom == "axis_exact":
        assert sin0 == 0.0 and cos0 == 1.0
    if (geom, cutoff) not in _NORMS:
        _NORMS[geom, cutoff] = dfft.stencil_norm(dfft.SpikeConstants(cos0, sin0, alpha - d_alpha, d_alpha, SCALE, cutoff))
    return _abi.Spikes(1, cutoff, THRESHOLD, cos0, sin0, alpha - d_alpha, d_alpha, SCALE, dfft.SPIKE_R0, _NORMS[geom, cutoff])


def _rows(nffts):
    rows = np.zeros(len(nffts), dtype=_abi.FFT_OBJECT_DTYPE)
    nf = np.asarray(nffts, dtype=np.int64)
    rows["nfft"] = nf
    rows["obj_id"] = np.arange(len(nf))
    rows["r_offset"] = np.concatenate([[0], np.cumsum(nf * nf)])[:-1]
    rows["k_offset"] = np.concatenate([[0], np.cumsum(nf * (nf // 2 + 1))])[:-1]
    return rows


def _stamp(row, x0, y0, left=0, top=0, right=0, bottom=0):
    """grid index (0, 0) at CCD pixel (x0, y0); the stamp is the grid inset by the pads"""
    n = int(row["nfft"])
    row["x0"], row["y0"] = x0, y0
    row["stamp_xmin"], row["stamp_xmax"] = x0 + left, x0 + n - 1 - right
    row["stamp_ymin"], row["stamp_ymax"] = y0 + top, y0 + n - 1 - bottom


def _sat(rng, shape=()):
    return rng.uniform(2.0e5, 4.0e5, shape)


class Case:
    pass


_CASES = {}


def case(shape, geom):
    """name, S (_abi.Spikes), rows, prefix (int64 [n + 1]), rbuf (float64, flat), boxes (the planted rowmin, rowmax, colmin, colmax
    of every object), cached: the tests share the arrays and leave them unchanged"""
    if (shape, geom) in _CASES:
        return _CASES[shape, geom]
    rng = np.random.default_rng([SEED, sorted(SHAPES).index(shape), sorted(GEOMETRIES).index(geom)])
    nffts = {"clip64": [64], "long32": [32], "edge96": [96], "wide_box": [64], "batch": [32, 64, 32, 96, 32]}[shape]
    rows = _rows(nffts)
    grids = [rng.uniform(-2.0, 10.0, (n, n)) for n in nffts]
    boxes = []
    if shape == "clip64":                                    # the whole grid is the stamp; 9 x 9 box off-centre; cutoff < grid
        _stamp(rows[0], 100, 200)
        grids[0][20:29, 37:46] = _sat(rng, (9, 9))
        boxes = [(20, 28, 37, 45)]
    elif shape == "long32":                                  # cutoff 200 >> grid, ONE saturated pixel
        _stamp(rows[0], 5, 7)
        grids[0][13, 21] = _sat(rng)
        boxes = [(13, 13, 21, 21)]
    elif shape == "edge96":                                  # unequal pads, off the CCD (negative CCD coordinates), box on the last column
        _stamp(rows[0], -30, -12, left=10, top=7, right=0, bottom=5)
        grids[0][40, 79], grids[0][42, 95] = _sat(rng), _sat(rng)     # opposite corners of a 3 x 17 box of otherwise unsaturated pixels
        grids[0][3, 50] = _sat(rng)                                   # above the stamp: not in the box, only clipped
        assert grids[0][40:43, 79:96].min() < 0.0                     # a negative pixel INSIDE the box (source_not_clipped)
        boxes = [(40, 42, 79, 95)]
    elif shape == "wide_box":                                # 20 x 20 box, cutoff 8: sources beyond the cutoff of every target
        _stamp(rows[0], 0, 0)
        grids[0][10:30, 30:50] = _sat(rng, (20, 20))
        boxes = [(10, 29, 30, 49)]
    elif shape == "batch":
        _stamp(rows[0], 10, 10)                              # 1: nothing saturated
        _stamp(rows[1], 300, 40)                             # 2: a 5 x 7 box
        grids[1][30:35, 20:27] = _sat(rng, (5, 7))
        _stamp(rows[2], 500, 500, 3, 3, 3, 3)                # 3: every pixel of the stamp saturated
        grids[2][3:29, 3:29] = _sat(rng, (26, 26))
        _stamp(rows[3], 700, 90, 8, 8, 8, 8)                 # 4: saturated pixels outside the stamp only
        grids[3][2, 5], grids[3][94, 90] = _sat(rng), _sat(rng)
        _stamp(rows[4], 0, 0)                                # 5: one pixel in the grid's corner
        grids[4][0, 0] = _sat(rng)
        boxes = [EMPTY_BOX, (30, 34, 20, 26), (3, 28, 3, 28), EMPTY_BOX, (0, 0, 0, 0)]
    c = Case()
    c.name, c.shape, c.geom = f"{shape}/{geom}", shape, geom
    c.S = spikes(geom, CUTOFF[shape])
    c.rows = rows
    nf = rows["nfft"].astype(np.int64)
    c.prefix = np.concatenate([[0], np.cumsum(nf * nf)]).astype(np.int64)
    c.rbuf = np.concatenate([g.ravel() for g in grids])
    c.boxes = np.array(boxes, dtype=np.int64)
    for a in (c.rows, c.prefix, c.rbuf, c.boxes):
        a.setflags(write=False)
    _CASES[shape, geom] = c
    return c


def raw_buffer(c):
    """a raw (unnormalised) real-space buffer for rbuf_raw = 1 and the image it stands for: raw = image nfft^2, rounded;
    image = fl64(raw fl64(1 / nfft^2)) as the ABI comment promises (96 is the grid whose 1 / n^2 is not a power of two)"""
    raw, image = np.empty_like(c.rbuf), np.empty_like(c.rbuf)
    for o in c.rows:
        n, off = int(o["nfft"]), int(o["r_offset"])
        raw[off:off + n * n] = c.rbuf[off:off + n * n] * float(n * n)
        image[off:off + n * n] = raw[off:off + n * n] * (np.float64(1.0) / (np.float64(n) * np.float64(n)))
    return raw, image
