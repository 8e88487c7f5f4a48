"""Hand-made sensors, scenes and object tables for the sensor-conversion and tree-ring tests (tests/test_sensor_convert.py on
the oracle, tests/test_sensor_convert_gpu.py on the device).  Everything is built with engine.SensorSetup directly, so that a
wrong index shows as a large error: absorption lengths a factor of ten apart, tree-ring tables of a few points, ring centres on
a pixel corner and far outside, private regions over the CCD corner and across a tile seam."""
import dataclasses
import functools
import os

import numpy as np

from imsim_amd import _abi, catalog, configs, sensor as sensormod, treerings
from imsim_amd.engine import SensorSetup, make_slots

SEED = (0x9E3779B9 << 32) | 398414
N_PHOT = (1, 255, 256, 257, 513, 4099)
OBJ_IDS = (0, 2 ** 31, 2 ** 32 + 5, 2 ** 40 + 7)
PHOT_FIRST = (0, 1000, 2 ** 32 - 100, 2 ** 33 + 3)
# absorption table: six points 20 nm apart inside the r band, neighbours a factor of ten apart; with 100 micron of silicon the
# last intervals convert most photons beyond the back (lost without a clip) and the first ones at the very surface
ABS_WL = np.array([580.0, 600.0, 620.0, 640.0, 660.0, 680.0])
ABS_LEN = np.array([0.4, 4.0, 40.0, 400.0, 4000.0, 400.0])
RAY_OPS = (_abi.IMS_OP_RUBIN_OPTICS, _abi.IMS_OP_RUBIN_DIFFRACTION_OPTICS)


@functools.lru_cache(maxsize=None)
def model(name, diffusion_factor=1.0):
    return sensormod.load_silicon_model(os.path.join(configs.DATA_DIR, "sensor_models", name), diffusion_factor=diffusion_factor)


def sed_tables():
    """inverse-CDF wavelength tables: one wider than the absorption table on both sides, one inside it"""
    u = np.linspace(0.0, 1.0, 257)
    return np.stack([545.0 + 160.0 * u ** 1.3, 603.7 + 52.1 * u])


class ConvertCase:
    def __init__(self, name, shape, model_name, chain, diff_step=None, diffusion_factor=1.0, sensor=True, n_obj=12):
        nx, ny = shape
        self.name = name
        sc = configs.scene_c3(nx=nx, ny=ny, seed=SEED, sensor=False)
        sc.sed_tables = sed_tables()
        ops = sc.ops
        sc.ops = {"default": ops, "no_trace": ops[:3], "none": []}[chain]
        self.has_angles = any(op[0] in RAY_OPS for op in sc.ops)
        self.default_chain = chain == "default"
        if sensor:
            m = model(model_name, diffusion_factor)
            if diff_step is not None:
                m = dataclasses.replace(m, diff_step=diff_step)
            tr = treerings.simple_treerings(amplitude=0.05, period=37.0, r_max=600.0, dr=3.0)
            sc.sensor = SensorSetup(model=m, abs_wl=ABS_WL, abs_len=ABS_LEN, tr_table=tr.f, tr_table2=tr.f2, tr_dr=tr.dr,
                                    tr_center=(-100.0, -100.0), slots=make_slots([(1, 1, nx, ny)]))
        self.scene = sc
        cat = catalog.synthetic_catalog(n_obj, nx=nx, ny=ny)
        phot = np.full(n_obj, 100)
        o, _ = configs.c3_objects(cat, phot, sc)
        i = np.arange(len(o))
        o["obj_id"] = [OBJ_IDS[k % 4] + 16 * (k // 4) for k in i]
        o["phot_first"] = [PHOT_FIRST[(k // 4 + k) % 4] for k in i]
        o["n_phot"] = [N_PHOT[k % 6] for k in i]
        o["sed_table"] = [(0, 1, -1)[k % 3] for k in i]
        o["sed_wave"] = [(571.3, 633.1, 691.9, 612.7)[k % 4] for k in i]          # below, inside, above the table, inside
        o["flags"], o["bf_state"] = 0, 0
        o["flags"][4] = _abi.IMS_OBJ_FAINT                                         # 513 photons that see neither ops nor sensor
        o["x0"], o["y0"] = 6.3 + (nx - 12) * ((i * 0.37) % 1.0), 6.8 + (ny - 12) * ((i * 0.61) % 1.0)
        o["stamp_xmin"], o["stamp_xmax"], o["stamp_ymin"], o["stamp_ymax"] = 1, nx, 1, ny
        self.objects = np.ascontiguousarray(o, dtype=_abi.OBJECT_DTYPE)

    def ref_sensor(self):
        import sensor_convert_ref as ref
        return None if self.scene.sensor is None else ref.Sensor(self.scene.sensor)


# name -> (CCD shape, sensor model, chain, keywords).  The cases are built on first use, not when the module is imported: loading
# the sensor models and tracing the WCS belongs to the tests that use them, not to the collection of the whole suite.
CONVERT = {"default_e2v4": ((33, 300), "lsst_e2v_50_4", "default", {}),
           "default_itl8_half_diffusion": ((148, 255), "lsst_itl_50_8", "default", dict(diffusion_factor=0.5)),
           "default_no_diffusion": ((33, 300), "lsst_e2v_50_4", "default", dict(diff_step=0.0)),
           "no_trace_itl8": ((33, 300), "lsst_itl_50_8", "no_trace", {}),
           "no_trace_no_diffusion": ((148, 255), "lsst_e2v_50_4", "no_trace", dict(diff_step=0.0)),
           "no_ops_e2v4": ((148, 255), "lsst_e2v_50_4", "none", {}),
           "no_sensor": ((33, 300), "lsst_e2v_50_4", "default", dict(sensor=False))}
CONVERT_NAMES = list(CONVERT)
DEFAULT_CHAIN_NAMES = [n for n, c in CONVERT.items() if c[2] == "default" and c[3].get("sensor", True)]


@functools.lru_cache(maxsize=None)
def convert_case(name):
    shape, model_name, chain, kw = CONVERT[name]
    return ConvertCase(name, shape, model_name, chain, **kw)


# ---------------- tree rings ----------------
# private regions (xmin, ymin, nx, ny): over the lower-left CCD corner, one pixel, nx + 1 = 17 owner cells (two 16-cell tiles,
# the second one cell wide), 40 x 12
REGIONS = [(-5, -3, 20, 14), (7, 9, 1, 1), (20, 30, 16, 9), (60, 100, 40, 12)]


class RingCase:
    def __init__(self, name, shape, model_name, table, table2, dr, center):
        nx, ny = shape
        self.name = name
        regions = [(1, 1, nx, ny)] + [(x, y, w, h) if x + w <= nx + 8 else (x - 40, y, w, h) for x, y, w, h in REGIONS]
        sc = configs.scene_c3(nx=nx, ny=ny, seed=SEED, sensor=False)
        sc.sensor = SensorSetup(model=model(model_name), abs_wl=ABS_WL, abs_len=ABS_LEN, tr_table=table, tr_table2=table2, tr_dr=dr,
                                tr_center=center, slots=make_slots(regions))
        self.scene = sc

    def ref_sensor(self):
        import sensor_convert_ref as ref
        return ref.Sensor(self.scene.sensor)


def _cos_table(amplitude, period, r_max, dr):
    t = treerings.simple_treerings(amplitude=amplitude, period=period, r_max=r_max, dr=dr)
    return t.f, t.f2, t.dr


def _short_table(values, dr):
    t = treerings.TreeRingTable(np.arange(len(values)) * dr, np.array(values))
    return t.f, t.f2, t.dr


RING_NAMES = ["spline_far_centre_4", "linear_far_centre_4", "table_ends_inside_corner_centre_4", "four_points_corner_centre_8",
              "three_points_linear_8", "spline_corner_centre_32"]


@functools.lru_cache(maxsize=None)
def _ring_tables():
    f, f2, dr = _cos_table(0.08, 41.0, 600.0, 3.0)
    # ends 119.6 px from the centre, inside the CCD; a step that no distance between pixel corners is a multiple of (with the
    # centre on a corner those distances are roots of integers, and r / dr on an integer is an ambiguous interval)
    g, g2, dg = _short_table(0.06 * np.cos(np.arange(45) * 2.7182818 / 29.0 * 2.0 * np.pi), 2.7182818)
    h, h2, dh = _short_table([0.07, -0.05, 0.06, -0.04], 47.3)       # four points: 141.9 px
    k, k2, dk = _short_table([0.05, -0.06, 0.03], 83.1)              # three points
    return {"spline_far_centre_4": ((148, 255), "lsst_e2v_50_4", f, f2, dr, (-100.0, -100.0)),
            "linear_far_centre_4": ((33, 300), "lsst_itl_50_4", f, None, dr, (-100.0, -100.0)),
            "table_ends_inside_corner_centre_4": ((148, 255), "lsst_e2v_50_4", g, g2, dg, (40.5, 100.5)),
            "four_points_corner_centre_8": ((148, 255), "lsst_itl_50_8", h, h2, dh, (17.5, 230.5)),
            "three_points_linear_8": ((33, 300), "lsst_e2v_50_8", k, None, dk, (20.5, 150.5)),
            "spline_corner_centre_32": ((33, 300), "lsst_e2v_50_32", g, g2, dg, (12.5, 77.5))}


@functools.lru_cache(maxsize=None)
def ring_case(name):
    return RingCase(name, *_ring_tables()[name])
