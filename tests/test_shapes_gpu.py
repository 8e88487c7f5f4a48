"""The sensor and image kernels on ragged, non-square CCDs.  Every other parity test renders square images whose sides are
multiples of 32, where the last 16 x 16 owner-cell tile is one cell wide, the 32 x 32 LDS charge tile lines up with the
image edge and a swapped row stride or tile count cannot show.  Here: shapes whose (n + 1) mod 16 tails and n mod 32
offsets differ, in both orientations, bright objects whose private regions and charge reach the last tile row and column
and all four corners, and the two real detector geometries (E2V 4096 x 4004, ITL 4072 x 4000).  Besides the oracle (bit
for bit), plain numpy references that share no code with it check the device (tests/shapes_ref.py)."""
import copy
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits_equal
import shapes_ref as ref

pytestmark = pytest.mark.gpu

NRECALC = 300
SENSOR = ("boundary", "bounds", "delta")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _arrays(r):
    return {name: r.bound.sensor_arrays[name].cpu().numpy().view(np.float64) for name in SENSOR}


def _assert_sensor(ga, orc, what, lo=0):
    for name in SENSOR:
        per = len(ga[name]) // len(ga["delta"])
        a, o = ga[name][lo * per:], orc.sensor_array(name)[lo * per:len(ga[name])]
        assert_bits_equal(a, o, f"{what}: sensor {name}")


def _batch(objects, i, nb):
    part = objects.copy()
    F = objects["n_phot"]
    lo, hi = (F * i) // nb, (F * (i + 1)) // nb
    part["phot_first"], part["n_phot"], part["bf_state"], part["flags"] = lo, hi - lo, 0, 0
    return part[part["n_phot"] > 0]


def _sensor_of(r):
    ss = r.scene.sensor
    return r.bound._slots_host[0], ss.model.num_vertices, ss.model.emptypoly


# ---------------------------------------------------------------------------------------------
# against the oracle, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native", ["1", "0"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_lsst_image_on_ragged_ccds_is_bit_exact(torch_cuda, monkeypatch, shape, native):
    """LSST_Image, full op chain, Silicon with tree rings, rounds of 300 photons: image, realized fluxes and the pixel-boundary
    state equal the oracle's, with the library's and the numpy planner"""
    from imsim_amd.engine import Renderer
    from oracle import orc_loader
    monkeypatch.setenv("IMS_NATIVE_PLAN", native)
    nx, ny = shape
    scene, objects = ref.ragged_c3_case(nx, ny)
    assert (objects["n_phot"] > 5 * NRECALC).sum() >= len(ref.edge_places(nx, ny))
    r = Renderer(scene)
    real = torch_cuda.zeros(len(objects), dtype=torch_cuda.float64, device="cuda")
    r.render_lsst_image(objects, nrecalc=NRECALC, realized=real)
    r.synchronize()
    orc = orc_loader.OracleScene(scene)
    real_o = np.zeros(len(objects))
    orc.render_lsst_image(objects, nrecalc=NRECALC, realized=real_o)
    img = orc.image
    assert img[0, 0] > 0 and img[0, -1] > 0 and img[-1, 0] > 0 and img[-1, -1] > 0
    assert_bits_equal(r.image_numpy(), img, "image")
    assert_bits_equal(real.cpu().numpy(), real_o, "realized flux")
    _assert_sensor(_arrays(r), orc, f"{shape}")


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_pooling_brighter_fatter_on_ragged_ccds_is_bit_exact(torch_cuda, shape):
    """photon pooling: slot 0 (the whole CCD) is the brighter-fatter region, recalculated between batches over the tiles
    in reach of the charge (tile tags) -- charge in the last tile row and column; pixel indices, image and sensor state equal
    the oracle's.  Then the same batches deposited into the delta image only (track_static_delta 2, folded into the image by
    the recalculations): the same image, and charge is conserved -- image plus the flux that left the CCD is the flux shot --
    and the image is the numpy histogram of the pixel indices"""
    from imsim_amd.engine import Renderer
    from oracle import orc_loader
    nx, ny = shape
    scene, objects = ref.ragged_c3_case(nx, ny, n_obj=80, flux_seed=4)
    scene.track_static_delta = 1
    r = Renderer(scene)
    orc = orc_loader.OracleScene(scene)
    nb = 3
    pixes = []
    for i in range(nb):
        part = _batch(objects, i, nb)
        if i:
            r.update_distortions(0, 1, bf_tag=i)
            orc.update_distortions(0, 1)
        pool = r.shoot_photons(part)
        r.apply_ops(pool)
        pix = r.accumulate(pool, want_pixel_index=True, bf_tag=i + 1)
        opool = orc.shoot_pool(part)
        orc.apply_ops(opool)
        opix = orc.accumulate(opool, want_pixel_index=True)
        r.synchronize()
        assert_bits_equal(pix.cpu().numpy(), opix, f"pixel indices, batch {i}")
        pixes.append((opix, opool.to_host()["flux"]))
        hit = opix[opix >= 0]
        assert (hit % nx == nx - 1).any() and (hit // nx == ny - 1).any(), "charge in the last column and row"
    assert_bits_equal(r.image_numpy(), orc.image, "pooled image")
    _assert_sensor(_arrays(r), orc, f"{shape}")
    # delta-only deposits
    sc2 = copy.copy(scene)
    sc2.track_static_delta = 2
    r2 = Renderer(sc2)
    shot = off = 0.0
    hist = np.zeros(nx * ny)
    for i in range(nb):
        part = _batch(objects, i, nb)
        if i:
            r2.update_distortions(0, 1, bf_tag=i, fold=True)
        pool = r2.shoot_photons(part)
        r2.apply_ops(pool)
        pix = r2.accumulate(pool, want_pixel_index=True, bf_tag=i + 1).cpu().numpy()
        f = pool.to_host()["flux"]
        assert_bits_equal(pix, pixes[i][0], f"delta only: pixel indices, batch {i}")
        shot += f.sum()
        off += f[pix < 0].sum()
        np.add.at(hist, pix[pix >= 0], f[pix >= 0])
    r2.fold_delta()
    r2.synchronize()
    img = r2.image64_numpy()
    assert float(r2.delta_tensor(0).abs().sum().item()) == 0.0
    assert off > 0 and img.sum() + off == shot
    assert_bits_equal(img.ravel(), hist, "delta only: image vs histogram of the pixel indices")
    assert_bits_equal(r2.image_numpy(), orc.image, "delta only: image vs oracle")


@pytest.mark.parametrize("shape", ref.SHAPES[:4], ids=ref.shape_id)
def test_lazy_static_state_on_ragged_ccds_gives_the_stored_state_image(torch_cuda, shape):
    """Renderer(lazy_static=True): slot 0 is never made, the photons near a pixel edge are finished from the tree-ring
    closed form (k_margin_photons) -- the image and realized fluxes of the stored-state render and of the oracle"""
    from imsim_amd.engine import Renderer
    from oracle import orc_loader
    nx, ny = shape
    scene, objects = ref.ragged_c3_case(nx, ny, flux_seed=3)
    out = []
    for lazy in (True, False):
        r = Renderer(scene, lazy_static=lazy)
        assert r.lazy_static == lazy
        if lazy:
            cells = (nx + 1) * (ny + 1)
            for name, per in (("boundary", 20), ("bounds", 8)):
                a = r.bound.sensor_arrays[name]
                a = a if a.dtype == torch_cuda.float64 else a.view(torch_cuda.float64)
                a[:cells * per].fill_(float("nan"))
        real = torch_cuda.zeros(len(objects), dtype=torch_cuda.float64, device="cuda")
        r.render_lsst_image(objects, nrecalc=NRECALC, realized=real)
        r.synchronize()
        out.append((r.image_numpy(), real.cpu().numpy()))
    assert_bits_equal(out[0][0], out[1][0], "image: lazy static state vs stored")
    assert_bits_equal(out[0][1], out[1][1], "realized fluxes")
    orc = orc_loader.OracleScene(scene)
    orc.render_lsst_image(objects, nrecalc=NRECALC)
    assert_bits_equal(out[0][0], orc.image, "image vs oracle")


FOCAL = {0: (200, 148), 1: (148, 200), 2: (255, 142), 3: (148, 255), 4: (200, 148)}


def _focal_build(det):
    from imsim_amd.config import ccd_seed
    nx, ny = FOCAL[det]
    scene, objects = ref.ragged_c3_case(nx, ny, n_obj=90, flux_seed=det + 2, seed=ccd_seed(398414, det),
                                    bright=(13000, 21000))          # 43 .. 70 rounds: the top chains that advance jointly
    return scene, objects


@pytest.mark.parametrize("search", ["1", "0"])
def test_focal_plane_of_ragged_ccds_joint_rounds_and_arena(torch_cuda, monkeypatch, search):
    """a focal plane of ragged CCDs of different sizes (a transposed pair among them, whose owner cells the sensor arena
    cannot tell apart): joint brighter-fatter rounds over lists of tiles (forced on at this size; appended to by the pixel
    search, or built from the charge marks) equal a chain per CCD, each CCD equals its stand-alone render, and one equals
    the oracle's.  The bright objects' private regions are wider than tall and taller than wide, at every edge"""
    from imsim_amd import focal_plane
    from imsim_amd.engine import Renderer
    from oracle import orc_loader
    dets = sorted(FOCAL)
    monkeypatch.setenv("IMS_FOCAL_JOINT", "0")
    monkeypatch.setenv("IMS_FOCAL_ARENA", "0")
    single = focal_plane.render_focal_plane(dets, _focal_build, concurrent=2, nrecalc=NRECALC)
    monkeypatch.setenv("IMS_FOCAL_ARENA", "1")
    monkeypatch.setenv("IMS_FOCAL_JOINT", "8")
    monkeypatch.setenv("IMS_JOINT_LIST_MIN", "0")
    monkeypatch.setenv("IMS_ACTIVE_FRACTION", "0.01")
    monkeypatch.setenv("IMS_JOINT_FINE_MARKS", "1")
    monkeypatch.setenv("IMS_JOINT_SEARCH_LISTS", search)
    joint = focal_plane.render_focal_plane(dets, _focal_build, concurrent=2, nrecalc=NRECALC)
    assert focal_plane.render_focal_plane.last_joint_plans == len(dets)
    assert focal_plane.render_focal_plane.last_arena_gib > 0.0
    assert min(int(_focal_build(d)[1]["n_phot"].max()) for d in dets) > 40 * NRECALC
    for det in dets:
        scene, objects = _focal_build(det)
        assert single[det].shape == (scene.ny, scene.nx)
        r = Renderer(scene)
        r.render_lsst_image(objects, nrecalc=NRECALC)
        r.synchronize()
        assert_bits_equal(single[det], r.image_numpy(), f"CCD {det} {FOCAL[det]}: chain per CCD vs stand-alone")
        assert_bits_equal(joint[det], single[det], f"CCD {det} {FOCAL[det]}: joint rounds vs a chain per CCD")
        del r
    scene, objects = _focal_build(1)
    orc = orc_loader.OracleScene(scene)
    orc.render_lsst_image(objects, nrecalc=NRECALC)
    assert_bits_equal(joint[1], orc.image, "CCD 1 vs oracle")
    from imsim_amd import engine
    engine._SENSOR_ARENAS.clear()


@pytest.mark.parametrize("shape", [(255, 142), (142, 200)], ids=ref.shape_id)
def test_sky_pixel_areas_and_flat_on_ragged_ccds(torch_cuda, shape):
    """the sky on the pixel areas of a Silicon sensor (areas and Poisson deviates equal the oracle's) and LSST_Flat (image and
    boundary state equal the oracle's) on non-square CCDs"""
    from imsim_amd import configs, flat, lsst_image, treerings
    from imsim_amd.engine import Renderer
    from oracle import orc_loader
    nx, ny = shape
    scene, _ = ref.ragged_c3_case(nx, ny, n_obj=10)
    r = Renderer(scene)
    b = lsst_image.LSST_ImageBuilder()
    areas = b.sky_pixel_areas(r)
    orc = orc_loader.OracleScene(scene)
    want = np.empty(nx * ny)
    acc = np.zeros(1, dtype=np.int64)
    orc.lib.orc_sensor_pixel_areas(orc.bound.sensor_dev_ptr, 0, want.ctypes.data, acc.ctypes.data)
    assert tuple(areas.shape) == (ny, nx)
    assert_bits_equal(areas.cpu().numpy().ravel(), want, "tree-ring pixel areas")
    b.add_noise(r, sky_level=20000.0, seed=5, pixel_areas=areas, sky_gradient=(0.9, 0.0007, -0.0003))
    r.synchronize()
    xx, yy = np.meshgrid(np.arange(float(nx)), np.arange(float(ny)))
    base = np.ascontiguousarray(want.reshape(ny, nx) * (0.9 + 0.0007 * xx - 0.0003 * yy))
    orc.lib.orc_flat_add(None, base.ctypes.data, 20000.0 * 0.2 * 0.2, 1.0, 5, lsst_image.NOISE_STREAM, nx, ny,
                         orc.image64.ctypes.data, None)
    assert_bits_equal(r.image.cpu().numpy(), orc.image64, "sky on tree-ring pixel areas")
    # LSST_Flat
    tr = treerings.simple_treerings(0.26, 87.0, dr=0.87)
    kw = dict(sensor=True, treering=tr, treering_center=(-100.0, -100.0), seed=77)
    fx, fy = nx - 10, ny - 10
    rf = Renderer(configs.scene_flat(fx, fy, **kw))
    fb = flat.LSST_FlatBuilder()
    fb.setup({"counts_per_pixel": 9000, "max_counts_per_iter": 3000, "xsize": fx, "ysize": fy})
    img = fb.build_image(rf, seed=77).cpu().numpy()
    of = orc_loader.OracleScene(configs.scene_flat(fx, fy, **kw))
    oimg = of.build_flat(9000.0, 3000.0, seed=77)
    assert img.shape == (fy, fx) and abs(img.mean() / 9000.0 - 1) < 0.01
    assert_bits_equal(img, oimg, "flat image")
    ga = _arrays(rf)
    for name in ("boundary", "bounds"):
        assert_bits_equal(ga[name], of.sensor_array(name), f"flat sensor {name}")


# ---------------------------------------------------------------------------------------------
# against plain numpy references
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_sensorless_image_is_the_histogram_of_the_pool(torch_cuda, shape):
    """no sensor, unit-flux photons: the fused kernel's image (LDS charge tiles that straddle the image edges) is np.add.at of
    the photon pool over the nominal pixels, clipped to the stamps and the image -- exactly"""
    from imsim_amd import configs, catalog
    from imsim_amd.engine import Renderer
    nx, ny = shape
    scene = configs.scene_c2(nx=nx, ny=ny)
    cat = catalog.synthetic_catalog(60, nx=nx, ny=ny)
    objects, _ = catalog.build_object_table(cat, catalog.realize_fluxes(cat["nominal_flux"], 2))
    for k, (x, y, w, h) in enumerate(ref.edge_places(nx, ny)):
        ref.place(objects, k, x, y, w, h, 3000 + 11 * k)
    r = Renderer(scene)
    g = r.shoot_ops_photons(objects).to_host()
    r.render(objects)
    r.synchronize()
    assert set(np.unique(g["flux"])) <= {0.0, 1.0}
    want = ref.histogram(g["x"], g["y"], g["flux"], ref.stamps_of(objects, g["obj_index"]), scene.xmin, scene.ymin, nx, ny)
    assert want[0, 0] > 0 and want[-1, -1] > 0 and want[0, -1] > 0 and want[-1, 0] > 0
    assert_bits_equal(r.image64_numpy(), want, "fused image vs histogram of the pool")


def _check_search(r, objects, pix, conv, obj_index, what):
    """the device's pixel of every photon (pix, from ims_accumulate) against the numpy pixel search over the device's own
    boundary array, the photons at their conversion depth taken from the converted pool (which stores no object index: the
    unconverted pool's obj_index is the same photon's)"""
    nx, ny = r.scene.nx, r.scene.ny
    slot, nV, empty = _sensor_of(r)
    bnd = r.bound.sensor_arrays["boundary"].cpu().numpy().view(np.float64)
    f = conv["flux"]
    live = np.flatnonzero(f != 0)
    zs = conv["dxdz"][live]
    ix, iy, lost, amb = ref.pixel_search(bnd, slot, nV, empty, conv["x"][live], conv["y"][live], np.abs(zs), np.signbit(zs),
                                         ref.stamps_of(objects, obj_index[live]))
    px, py = ix - r.scene.xmin, iy - r.scene.ymin
    on = ~lost & (px >= 0) & (px < nx) & (py >= 0) & (py < ny)
    want = np.where(on, py * nx + px, -1)
    got = pix[live]
    assert (pix[f == 0] == -1).all(), f"{what}: photons lost in the silicon were deposited"
    bad = (got != want) & ~amb
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {live.size} photons in another pixel than the polygons say, "
                           f"first {np.flatnonzero(bad)[:5]}: device {got[bad][:5]} numpy {want[bad][:5]}")
    assert amb.sum() <= max(3, 1e-4 * live.size), f"{what}: {int(amb.sum())} photons within 1e-12 px of an edge"
    searched = (want != np.floor(conv["y"][live] + 0.5 - r.scene.ymin).astype(np.int64) * nx
                + np.floor(conv["x"][live] + 0.5 - r.scene.xmin).astype(np.int64))
    assert searched[on].sum() > 0                                # some photons left their nominal pixel
    return int(amb.sum()), int((~on).sum())


@pytest.mark.parametrize("shape", ref.SHAPES[:4], ids=ref.shape_id)
def test_pixel_search_puts_every_photon_in_its_polygon(torch_cuda, shape):
    """every photon ims_accumulate deposits lies in the polygon of its pixel, rebuilt in numpy from the device's boundary
    array (polygon_vertex layout, shrunk by the photon's depth factor); a photon that no polygon of the search holds stays
    in its nominal pixel (coin set) or goes to the first neighbour searched; off the image on the device is off it in numpy.
    The converted pool (same Philox streams) supplies each photon's position at the conversion depth.  On the pristine
    tree-ring state, then after a brighter-fatter recalculation of slot 0 with charge in the tail tiles."""
    from imsim_amd.engine import Renderer
    nx, ny = shape
    scene, objects = ref.ragged_c3_case(nx, ny, n_obj=80, flux_seed=5)
    scene.track_static_delta = 1
    r = Renderer(scene)
    for i in range(2):
        part = _batch(objects, i, 2)
        if i:
            r.update_distortions(0, 1, bf_tag=i)
        conv = r.shoot_ops_photons(part, converted=True).to_host()
        pool = r.shoot_ops_photons(part)
        pix = r.accumulate(pool, want_pixel_index=True, bf_tag=i + 1)
        r.synchronize()
        _check_search(r, part, pix.cpu().numpy(), conv, pool.to_host()["obj_index"], f"{shape} batch {i}")
        if i == 0:
            hit = pix[pix >= 0].cpu().numpy()
            assert (hit % nx == nx - 1).any() and (hit // nx == ny - 1).any(), "charge in the last column and row"


def _device_areas(r):
    sc = r.scene
    area = r.torch.empty(sc.nx * sc.ny, dtype=r.torch.float64, device=r.device)
    acc = r.torch.zeros(1, dtype=r.torch.int64, device=r.device)
    from imsim_amd import _abi
    _abi.check(r.lib.ims_sensor_pixel_areas(r.bound.sensor_dev_ptr, C.byref(r.bound.sensor_host), 0, area.data_ptr(),
                                            acc.data_ptr(), r._stream()), "ims_sensor_pixel_areas")
    r.synchronize()
    return area.cpu().numpy().reshape(sc.ny, sc.nx)


@pytest.mark.parametrize("shape", [(255, 142), (148, 255), (33, 300)], ids=ref.shape_id)
def test_pixel_areas_are_the_shoelace_areas(torch_cuda, shape):
    """k_pixel_areas equals the shoelace area of every pixel's polygon of the device's boundary array to 1e-13, on the
    pristine tree-ring state and after a brighter-fatter recalculation"""
    from imsim_amd.engine import Renderer
    nx, ny = shape
    scene, objects = ref.ragged_c3_case(nx, ny, n_obj=40, flux_seed=6)
    scene.track_static_delta = 1
    r = Renderer(scene)
    slot, nV, empty = _sensor_of(r)
    prev = None
    for stage in ("pristine", "after brighter-fatter"):
        got = _device_areas(r)
        want = ref.slot_areas(r.bound.sensor_arrays["boundary"].cpu().numpy().view(np.float64), slot, nV, empty)
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0, err_msg=f"{shape} {stage}")
        if prev is None:
            prev = want
            pool = r.shoot_ops_photons(_batch(objects, 0, 1))
            r.accumulate(pool, bf_tag=1)
            r.update_distortions(0, 1, bf_tag=1)
    assert np.abs(want - prev).max() > 1e-4


def test_float_hand_over_is_astype_float32(torch_cuda):
    """ims_image_to_float rounds the f64 image exactly as numpy's astype(float32): non-integer values, ties, subnormals,
    overflow, signed zeros, at ragged lengths"""
    from imsim_amd import _abi
    lib = _abi.load()
    rng = np.random.default_rng(11)
    ulp = np.ldexp(1.0, -24)
    special = np.array([0.0, -0.0, 0.1, -0.1, 1.0 + ulp, 1.0 + 3 * ulp, 1.0 + ulp * 1.5, 2.0 ** 24 + 1.0, 2.0 ** 24 + 3.0,
                        3.4028235677973366e38, 3.5e38, -3.5e38, 1e-40, -1e-45, 7e-46, 1e-300, np.inf, -np.inf], dtype=np.float64)
    for n in (1, 17, 255, 257, 148 * 255, 4072 * 3 + 1):
        v = np.concatenate([special, rng.normal(0, 1e4, n) * rng.choice([1e-3, 1.0, 1e3], n)])[:n]
        src = torch_cuda.from_numpy(v).cuda()
        dst = torch_cuda.full((n + 64,), 12345.0, dtype=torch_cuda.float32, device="cuda")
        _abi.check(lib.ims_image_to_float(src.data_ptr(), dst.data_ptr(), n, None), "ims_image_to_float")
        torch_cuda.cuda.synchronize()
        out = dst.cpu().numpy()
        with np.errstate(over="ignore"):
            assert_bits_equal(out[:n], v.astype(np.float32), f"n = {n}")
        assert (out[n:] == 12345.0).all(), f"n = {n}: written past the end"


# ---------------------------------------------------------------------------------------------
# the real detector geometries
# ---------------------------------------------------------------------------------------------
REAL = [(4096, 4004, "lsst_e2v_50_4"), (4072, 4000, "lsst_itl_50_4")]


def _real_case(nx, ny, model):
    scene, objects = ref.ragged_c3_case(nx, ny, n_obj=1500, flux_seed=7, scratch=4_000_000, model_name=model,
                                        bright=(20000, 45000))
    return scene, objects


@pytest.mark.parametrize("nx,ny,model", REAL)
def test_real_ccd_lsst_image_is_bit_exact(torch_cuda, nx, ny, model):
    """LSST_Image on a whole E2V / ITL CCD, the static state not made (lazy_static): image, realized fluxes and the private
    regions' boundary state equal the oracle's; bright stars in the corners and the last tile row and column"""
    from imsim_amd.engine import Renderer
    from oracle import orc_loader
    scene, objects = _real_case(nx, ny, model)
    r = Renderer(scene, lazy_static=True)
    assert r.lazy_static
    real = torch_cuda.zeros(len(objects), dtype=torch_cuda.float64, device="cuda")
    r.render_lsst_image(objects, realized=real)
    r.synchronize()
    orc = orc_loader.OracleScene(scene)
    real_o = np.zeros(len(objects))
    orc.render_lsst_image(objects, realized=real_o)
    img = orc.image
    assert img[0, 0] > 0 and img[0, -1] > 0 and img[-1, 0] > 0 and img[-1, -1] > 0
    assert_bits_equal(r.image_numpy(), img, "image")
    assert_bits_equal(real.cpu().numpy(), real_o, "realized flux")
    _assert_sensor(_arrays(r), orc, f"{nx} x {ny} private regions", lo=r.bound.static_cells)


@pytest.mark.parametrize("nx,ny,model", REAL)
def test_real_ccd_pooling_is_bit_exact(torch_cuda, nx, ny, model):
    """photon pooling on a whole E2V / ITL CCD: two batches, one tile-tagged recalculation of slot 0 between them -- pixel
    indices, image and the state of the edge bands of slot 0 (the last rows and columns of owner cells) equal the oracle's"""
    from imsim_amd.engine import Renderer
    from oracle import orc_loader
    scene, objects = _real_case(nx, ny, model)
    scene.track_static_delta = 1
    r = Renderer(scene)
    orc = orc_loader.OracleScene(scene)
    for i in range(2):
        part = _batch(objects, i, 2)
        if i:
            r.update_distortions(0, 1, bf_tag=i)
            orc.update_distortions(0, 1)
        pool = r.shoot_photons(part)
        r.apply_ops(pool)
        pix = r.accumulate(pool, want_pixel_index=True, bf_tag=i + 1)
        opool = orc.shoot_pool(part)
        orc.apply_ops(opool)
        opix = orc.accumulate(opool, want_pixel_index=True)
        r.synchronize()
        assert_bits_equal(pix.cpu().numpy(), opix, f"pixel indices, batch {i}")
    assert_bits_equal(r.image_numpy(), orc.image, "pooled image")
    W, H = nx + 1, ny + 1
    band = np.zeros((H, W), bool)
    band[:40], band[-40:], band[:, :40], band[:, -40:] = True, True, True, True
    cells = np.flatnonzero(band.ravel())
    for name in SENSOR:
        per = {"boundary": 20, "bounds": 8, "delta": 1}[name]
        t = r.bound.sensor_arrays[name]
        t = t if t.dtype == torch_cuda.float64 else t.view(torch_cuda.float64)
        idx = torch_cuda.from_numpy((cells[:, None] * per + np.arange(per)).ravel()).cuda()
        got = t[idx].cpu().numpy()
        want = orc.sensor_array(name)[(cells[:, None] * per + np.arange(per)).ravel()]
        assert_bits_equal(got, want, f"{nx} x {ny}: sensor {name} in the edge bands")
