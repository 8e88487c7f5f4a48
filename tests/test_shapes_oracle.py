"""The CPU oracle on ragged, non-square CCDs, checked against plain numpy references that share no code with it
(tests/shapes_ref.py): pixel areas against the shoelace area of the polygons of its boundary array, its bounds lines against
the inner / outer rectangles of the same polygons, a sensorless image against the histogram of its photon pool, and charge
conservation of a pooled brighter-fatter render.  The same references check the GPU in tests/test_shapes_gpu.py."""
import numpy as np
import pytest

from helpers import assert_bits_equal
import shapes_ref as ref


def _sensor(orc):
    ss = orc.scene.sensor
    return orc.sensor_array("boundary"), orc.bound._slots_host[0], ss.model.num_vertices, ss.model.emptypoly


def _orc_areas(orc):
    sc = orc.scene
    area = np.empty(sc.nx * sc.ny)
    acc = np.zeros(1, dtype=np.int64)
    orc.lib.orc_sensor_pixel_areas(orc.bound.sensor_dev_ptr, 0, area.ctypes.data, acc.ctypes.data)
    return area.reshape(sc.ny, sc.nx)


def _pooled_batch(orc, objects, i, nb):
    part = objects.copy()
    F = objects["n_phot"]
    lo, hi = (F * i) // nb, (F * (i + 1)) // nb
    part["phot_first"], part["n_phot"], part["bf_state"], part["flags"] = lo, hi - lo, 0, 0
    return part[part["n_phot"] > 0]


@pytest.mark.parametrize("shape", ref.SHAPES[:3], ids=ref.shape_id)
def test_oracle_pixel_areas_and_bounds_are_the_polygons_of_its_boundary_array(shape):
    """orc_sensor_pixel_areas equals the shoelace area of every pixel's polygon (1e-13 relative) and the bounds lines are the
    inner / outer rectangles of those polygons -- on the pristine tree-ring state and after a brighter-fatter recalculation
    with charge in the last tile row and column"""
    from oracle import orc_loader
    nx, ny = shape
    scene, objects = ref.ragged_c3_case(nx, ny, n_obj=40)
    scene.track_static_delta = 1
    orc = orc_loader.OracleScene(scene)
    for stage in ("pristine", "after brighter-fatter"):
        bnd, slot, nV, empty = _sensor(orc)
        want = ref.slot_areas(bnd, slot, nV, empty)
        got = _orc_areas(orc)
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0, err_msg=stage)
        jj, ii = np.mgrid[0:ny, 0:nx]
        p = ref.polygons(bnd, slot, nV, empty, ii.ravel(), jj.ravel())
        x0, x1, y0, y1 = ref.inner_bounds(p, nV)
        b = orc.sensor_array("bounds")[:(nx + 1) * (ny + 1) * 8].reshape(ny + 1, nx + 1, 8)[:ny, :nx].reshape(-1, 8)
        for k, v in enumerate((x0, x1, y0, y1)):
            assert_bits_equal(b[:, k], v, f"{stage}: inner bound {k}")
        assert_bits_equal(b[:, 4], np.minimum(0.0, p[..., 0].min(axis=1)), f"{stage}: outer x min")
        assert_bits_equal(b[:, 5], np.maximum(1.0, p[..., 0].max(axis=1)), f"{stage}: outer x max")
        assert_bits_equal(b[:, 6], np.minimum(0.0, p[..., 1].min(axis=1)), f"{stage}: outer y min")
        assert_bits_equal(b[:, 7], np.maximum(1.0, p[..., 1].max(axis=1)), f"{stage}: outer y max")
        if stage == "pristine":
            assert 1e-6 < want.std() < 1e-2
            pool = orc.shoot_pool(_pooled_batch(orc, objects, 0, 1))
            orc.apply_ops(pool)
            pix = orc.accumulate(pool, want_pixel_index=True)
            hit = pix[pix >= 0]
            assert (hit % nx == nx - 1).any() and (hit // nx == ny - 1).any(), "charge in the last column and row"
            before = want
            orc.update_distortions(0, 1)
    assert np.abs(want - before).max() > 1e-4                # the charge moved the boundaries


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_oracle_sensorless_image_is_the_histogram_of_its_pool(shape):
    """no sensor, unit-flux photons: the oracle's image is np.add.at of its own pool over the nominal pixels, clipped to the
    stamps and to the image -- objects straddle every edge and corner"""
    from oracle import orc_loader
    from imsim_amd import configs, catalog
    nx, ny = shape
    scene = configs.scene_c2(nx=nx, ny=ny)
    cat = catalog.synthetic_catalog(60, nx=nx, ny=ny)
    objects, _ = catalog.build_object_table(cat, catalog.realize_fluxes(cat["nominal_flux"], 2))
    for k, (x, y, w, h) in enumerate(ref.edge_places(nx, ny)):
        ref.place(objects, k, x, y, w, h, 3000 + 11 * k)
    orc = orc_loader.OracleScene(scene)
    pool = orc.shoot_pool(objects)
    orc.accumulate(pool)
    g = pool.to_host()
    assert set(np.unique(g["flux"])) <= {0.0, 1.0}
    want = ref.histogram(g["x"], g["y"], g["flux"], ref.stamps_of(pool.objects, g["obj_index"]), scene.xmin, scene.ymin, nx, ny)
    assert want[0, 0] > 0 and want[-1, -1] > 0 and want[0, -1] > 0 and want[-1, 0] > 0
    assert_bits_equal(orc.image64, want, "image vs histogram of the pool")


@pytest.mark.parametrize("shape", ref.SHAPES[1:3], ids=ref.shape_id)
def test_oracle_pooled_charge_is_conserved(shape):
    """pooling mode with brighter-fatter recalculations between batches: the image plus the flux of the photons that left
    the CCD equals the flux shot, and the image is the histogram of the pixel indices"""
    from oracle import orc_loader
    nx, ny = shape
    scene, objects = ref.ragged_c3_case(nx, ny, n_obj=60)
    scene.track_static_delta = 1
    orc = orc_loader.OracleScene(scene)
    shot = off = 0.0
    hist = np.zeros(nx * ny)
    for i in range(3):
        if i:
            orc.update_distortions(0, 1)
        pool = orc.shoot_pool(_pooled_batch(orc, objects, i, 3))
        orc.apply_ops(pool)
        pix = orc.accumulate(pool, want_pixel_index=True)
        f = pool.to_host()["flux"]
        assert set(np.unique(f)) <= {0.0, 1.0}
        shot += f.sum()
        off += f[pix < 0].sum()
        np.add.at(hist, pix[pix >= 0], f[pix >= 0])
    assert off > 0
    assert orc.image64.sum() + off == shot
    assert_bits_equal(orc.image64.ravel(), hist, "image vs histogram of the pixel indices")
