"""Small slots and charge fields for the tests of the brighter-fatter boundary update (tests/test_bf_update.py on the oracle,
tests/test_bf_update_gpu.py on the device).  Every slot is tens of pixels on a side, so the exact reference of
tests/bf_update_ref.py runs in seconds.  A case is a named tuple: sensor model, qdist, the regions (region 0 is the CCD, the
static slot; further ones are private regions), the slots one launch updates, and the charge fields -- each field is one launch,
{slot: [(i, j, electrons)]} in slot-local pixel indices.

Charges are a few hundred to a few thousand electrons, distinct and no powers of two, so that every tap with a non-zero table
entry moves its point by more than 100 bounds (bf_update_ref.FACTOR; tests/test_bf_update.py asserts it for every case and
field).  The taps that do not are named in EXCEPTIONS with the impulse case of larger charge that covers them."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name model qdist regions first_slot n_slots fields")

# the tree rings of the initial points (a linear table, as in tests/test_independent_fill.py)
TR_DR, TR_CENTER = 3.0, (-40.0, 25.0)
TR_TABLE = 0.01 * np.sin(np.arange(0, 200) * 3.0 / 7.0)


def _charge(k):
    return 1003 + 37 * k                                    # odd, distinct, between 2^9 and 2^11


def _impulses(nx, ny):
    """one charged pixel per field: a tile's interior, tile-local 0 and 15 in x and y (the window and its extra row / column cross a
    16-cell seam), the four corners and the middle of each edge"""
    places = [(8, 24), (15, 15), (16, 16), (15, 16), (16, 31), (31, 16),
              (0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (nx // 2, 0), (0, ny // 2), (nx - 1, ny // 2), (nx // 2, ny - 1)]
    return [{0: [(i, j, _charge(k))]} for k, (i, j) in enumerate(places)]


def _dense(nx, ny):
    return [{0: [(i, j, 311 + 7 * (j * nx + i)) for j in range(ny) for i in range(nx)]}]


def _sparse(nx, ny):
    """50 x 40 pixels = 4 x 3 tiles of owner cells: a cluster in rows 0 .. 4 of the first tile row (its reach ends at cell row 8: the
    wavefront of rows 12 .. 15 has nothing to do), scattered pixels left of x = 30 from row 20 up, nothing right of x = 30 (the
    last tile column, cells 48 .. 50, is out of every reach); 3 % of the pixels"""
    rng = np.random.default_rng(20261020)
    cells = {(int(i), int(j)) for i, j in zip(rng.integers(2, 12, 14), rng.integers(0, 5, 14))}
    cells |= {(int(i), int(j)) for i, j in zip(rng.integers(0, 30, 46), rng.integers(20, ny, 46))}
    return [{0: [(i, j, 1501 + 53 * k) for k, (i, j) in enumerate(sorted(cells))]}]


def _fractional(nx, ny):
    rng = np.random.default_rng(7)
    cells = sorted({(int(i), int(j)) for i, j in zip(rng.integers(0, nx, 30), rng.integers(0, ny, 30))})
    frac = [{0: [(i, j, 700.0 + 0.37 * k + 1.0 / (3 + k)) for k, (i, j) in enumerate(cells)]}]
    # a pair of opposite sign side by side: their contributions to the points between them nearly cancel
    pair = [{0: [(10, 9, 2000.5), (11, 9, -1999.75)]}, {0: [(15, 15, 1800.25), (15, 16, -1800.75)]}]
    return frac + pair


def _three_regions():
    """slots 1 .. 3 in one launch: wider than tall, taller than wide, 16 x 16 cells exactly"""
    return [{1: [(0, 0, 1009), (39, 11, 1213), (15, 5, 907), (16, 6, 1511), (30, 0, 1117)],
             2: [(11, 39, 1301), (0, 16, 1409), (5, 15, 811), (6, 31, 1019)],
             3: [(14, 14, 1607), (0, 14, 709), (7, 7, 1901)]}]


def _many_regions(n):
    """n one-tile regions in one launch; charge in the first, the last and a few between"""
    f = {}
    for k, s in enumerate((1, 2, 17, 33, 64, 65, n - 1, n)):
        f[s] = [((3 * k) % 10, (7 * k) % 10, 1103 + 61 * k), ((3 * k + 5) % 10, (7 * k + 4) % 10, 1721 + 29 * k)]
    return [f]


def _generic_fields(nx, ny):
    imp = [{0: [(i, j, _charge(20 + k))]} for k, (i, j) in enumerate([(15, 15), (0, 0), (nx - 1, ny - 1), (16, 8), (nx - 1, 0)])]
    rng = np.random.default_rng(11)
    cells = sorted({(int(i), int(j)) for i, j in zip(rng.integers(0, nx, 24), rng.integers(0, ny, 24))})
    return imp + [{0: [(i, j, 1301 + 43 * k) for k, (i, j) in enumerate(cells)]}]


N_MANY = 70                                                 # 65 .. 128 tiles: the late-table form of the DPP update


@functools.lru_cache(maxsize=None)
def _catalogue():
    many = [(1, 1, 24, 24)] + [(2 + 3 * (k % 7), 2 + 2 * (k // 7), 10, 10) for k in range(N_MANY)]
    cases = [Case("impulses_33x47_e2v4", "lsst_e2v_50_4", 3, [(1, 1, 33, 47)], 0, 1, _impulses(33, 47)),
             Case("impulses_47x33_itl8", "lsst_itl_50_8", 3, [(1, 1, 47, 33)], 0, 1, _impulses(47, 33)),
             Case("dense_20x36_e2v4", "lsst_e2v_50_4", 3, [(1, 1, 20, 36)], 0, 1, _dense(20, 36)),
             Case("sparse_50x40_itl4", "lsst_itl_50_4", 3, [(1, 1, 50, 40)], 0, 1, _sparse(50, 40)),
             Case("fractional_and_opposite_24x20_e2v8", "lsst_e2v_50_8", 3, [(1, 1, 24, 20)], 0, 1, _fractional(24, 20)),
             Case("three_regions_e2v4", "lsst_e2v_50_4", 3, [(1, 1, 40, 40), (3, 5, 40, 12), (20, 2, 12, 40), (10, 10, 15, 15)], 1, 3,
                  _three_regions()),
             Case("many_regions_itl4", "lsst_itl_50_4", 3, many, 1, N_MANY, _many_regions(N_MANY)),
             Case("generic_e2v32_q3", "lsst_e2v_50_32", 3, [(1, 1, 18, 17)], 0, 1, _generic_fields(18, 17)),
             Case("generic_e2v4_q2", "lsst_e2v_50_4", 2, [(1, 1, 33, 18)], 0, 1, _generic_fields(33, 18)),
             Case("generic_itl8_q4", "lsst_itl_50_8", 4, [(1, 1, 18, 33)], 0, 1, _generic_fields(18, 33))]
    return {c.name: c for c in cases}


NAMES = ["impulses_33x47_e2v4", "impulses_47x33_itl8", "dense_20x36_e2v4", "sparse_50x40_itl4", "fractional_and_opposite_24x20_e2v8",
         "three_regions_e2v4", "many_regions_itl4", "generic_e2v32_q3", "generic_e2v4_q2", "generic_itl8_q4"]
Q3_FAST = NAMES[:7]                                          # 4 and 8 vertices per edge with qdist 3: k_update_distortions_q3
GENERIC = NAMES[7:]                                          # k_update_distortions
# (case, what) whose taps cannot move their point by FACTOR bounds at these charges, and the impulse case that covers them
EXCEPTIONS = {}


def case(name):
    return _catalogue()[name]


def tiles(c):
    """16 x 16 tiles of owner cells in the case's launch"""
    return sum(((nx + 1 + 15) // 16) * ((ny + 1 + 15) // 16) for _, _, nx, ny in c.regions[c.first_slot:c.first_slot + c.n_slots])


def offsets(c):
    """owner-cell offset of every region, packed in order (engine.make_slots)"""
    off, out = 0, []
    for _, _, nx, ny in c.regions:
        out.append(off)
        off += (nx + 1) * (ny + 1)
    return out, off


def slots(c):
    """the regions as the dicts shapes_ref.slot_view reads"""
    off, _ = offsets(c)
    return [dict(xmin=x, ymin=y, nx=nx, ny=ny, offset=o) for (x, y, nx, ny), o in zip(c.regions, off)]


def delta_of(c, field):
    """the delta array of all regions [total cells] for one field"""
    off, total = offsets(c)
    d = np.zeros(total)
    for s, rows in field.items():
        _, _, nx, ny = c.regions[s]
        for i, j, e in rows:
            assert 0 <= i < nx and 0 <= j < ny and c.first_slot <= s < c.first_slot + c.n_slots
            d[off[s] + j * (nx + 1) + i] = e
    return d


def scene(c, track_static_delta=0, seed=77):
    """the case as a renderer takes it: a bare Gaussian-PSF scene on region 0 with the case's model, qdist and regions"""
    import os
    from imsim_amd import _abi, configs, sensor as sensormod
    from imsim_amd.engine import Scene, SensorSetup, make_slots
    x, y, nx, ny = c.regions[0]
    sc = Scene(nx=nx, ny=ny, xmin=x, ymin=y, seed=seed, psf=[(_abi.IMS_PSF_GAUSSIAN, 0, 0.3, 0.0, 1.0)], ops=[])
    m = sensormod.load_silicon_model(os.path.join(configs.DATA_DIR, "sensor_models", c.model), qdist=c.qdist)
    sc.sensor = SensorSetup(model=m, abs_wl=np.array([300.0, 1100.0]), abs_len=np.array([1.0, 1.0]), tr_table=TR_TABLE, tr_dr=TR_DR,
                            tr_center=TR_CENTER, slots=make_slots(list(c.regions)))
    sc.track_static_delta = track_static_delta
    return sc


# ---------------- a real round: the device deposits the charge and writes its own tile marks ----------------
ROUND_REGION = (1, 1, 64, 40)                               # 65 x 41 owner cells: 5 x 3 tiles
# (x, y) of the object of each round: charge in the last cells of tile (0, 0) that moves points of tiles (1, 0), (0, 1), (1, 1);
# then inside tile (2, 1) (the stamp of eleven pixels keeps it there).  The last tile column stays out of reach in both rounds.
ROUND_PLACES = [(15.6, 15.4), (40.4, 24.6)]


def round_case(track_static_delta):
    c = Case("round_64x40_e2v4", "lsst_e2v_50_4", 3, [ROUND_REGION], 0, 1, [])
    return c, scene(c, track_static_delta=track_static_delta)


def round_objects(k, n_phot=6000):
    from imsim_amd._abi import OBJECT_DTYPE
    x, y = ROUND_PLACES[k]
    obj = np.zeros(1, dtype=OBJECT_DTYPE)
    obj["obj_id"], obj["n_phot"], obj["x0"], obj["y0"], obj["flux_per_photon"] = 5 + k, n_phot, x, y, 1.0
    obj["jac"], obj["winv"] = (1, 0, 0, 1), (1 / 0.3, 0, 0, 1 / 0.3)
    obj["prof_table"], obj["sed_table"], obj["sed_wave"] = -1, -1, 600.0
    cx, cy = int(np.floor(x + 0.5)), int(np.floor(y + 0.5))
    obj["stamp_xmin"], obj["stamp_xmax"], obj["stamp_ymin"], obj["stamp_ymax"] = cx - 5, cx + 5, cy - 5, cy + 5
    return obj
