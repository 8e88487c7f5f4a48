"""The binning rule of ims_psf_image restated in numpy, for the tests of psf_image: f64 products, sums and comparisons, each
rounded once, as include/imsim_hip.h states them.  Nothing here comes from the kernel."""
import numpy as np


def cells_reference(dx, dy, inv_scale, nx, ny):
    """(ix, iy, inside) of every offset: u = fl(fl(dx inv_scale) + nx / 2), v likewise; inside where 0 <= u < nx and 0 <= v < ny,
    then (ix, iy) = (floor u, floor v); elsewhere (beside the stamp, or not a number) ix = iy = -1"""
    dx, dy = np.asarray(dx, dtype=np.float64).reshape(-1), np.asarray(dy, dtype=np.float64).reshape(-1)
    s = np.float64(inv_scale)
    with np.errstate(invalid="ignore", over="ignore"):
        u = dx * s + np.float64(nx) / np.float64(2.0)
        v = dy * s + np.float64(ny) / np.float64(2.0)
        inside = (u >= 0.0) & (u < np.float64(nx)) & (v >= 0.0) & (v < np.float64(ny))
    ix = np.where(inside, np.floor(np.where(inside, u, 0.0)), -1.0).astype(np.int64)
    iy = np.where(inside, np.floor(np.where(inside, v, 0.0)), -1.0).astype(np.int64)
    return ix, iy, inside


def counts_reference(dx, dy, flux, inv_scale, nx, ny):
    """(counts int64 [ny][nx], outside, dropped) of one row's photons: those of flux 0 (and, in a converted pool, those the
    sensor lost, which it stores with flux 0) are dropped and in no cell"""
    flux = np.asarray(flux).reshape(-1)
    used = flux != 0
    ix, iy, inside = cells_reference(np.asarray(dx).reshape(-1)[used], np.asarray(dy).reshape(-1)[used], inv_scale, nx, ny)
    counts = np.zeros((ny, nx), dtype=np.int64)
    np.add.at(counts, (iy[inside], ix[inside]), 1)
    return counts, int((~inside).sum()), int((~used).sum())
