"""The binning rule of ims_psf_profile restated in numpy, for the tests of psf_profile: f64 products, sums and comparisons, each
rounded once, as include/imsim_hip.h states them.  Nothing here comes from the kernel."""
import numpy as np


def binning_reference(dx, dy, r2_edges, dirs):
    """(radial index, sector index) of every offset.  r2_edges: n_r + 1 ascending squared radii; dirs: [n_phi][2] = (c_b, s_b),
    counter-clockwise (n_phi 0: every sector index is 0).
    radial: the number of edges e <= fl(fl(dx dx) + fl(dy dy)); sector: the first b with t_b >= 0 and t_{b+1} < 0,
    t_b = fl(fl(c_b dy) - fl(s_b dx)), b + 1 wrapping to 0; n_phi where no b qualifies."""
    dx, dy = np.asarray(dx, dtype=np.float64).reshape(-1), np.asarray(dy, dtype=np.float64).reshape(-1)
    e = np.asarray(r2_edges, dtype=np.float64).reshape(-1)
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 2)
    r2 = dx * dx + dy * dy
    radial = (e[None, :] <= r2[:, None]).sum(axis=1).astype(np.int64)
    n_phi = len(d)
    if n_phi == 0:
        return radial, np.zeros(len(dx), dtype=np.int64)
    t = d[None, :, 0] * dy[:, None] - d[None, :, 1] * dx[:, None]
    q = (t >= 0.0) & (np.roll(t, -1, axis=1) < 0.0)
    sector = np.where(q.any(axis=1), q.argmax(axis=1), n_phi).astype(np.int64)
    return radial, sector


def counts_reference(dx, dy, flux, r2_edges, dirs):
    """(counts int64 [n_r + 2][n_phi + 1], dropped) of one row's photons: those of flux 0 are dropped and in no bin"""
    flux = np.asarray(flux).reshape(-1)
    used = flux != 0
    radial, sector = binning_reference(np.asarray(dx)[used], np.asarray(dy)[used], r2_edges, dirs)
    counts = np.zeros((len(np.asarray(r2_edges).reshape(-1)) + 1, len(np.asarray(dirs).reshape(-1, 2)) + 1), dtype=np.int64)
    np.add.at(counts, (radial, sector), 1)
    return counts, int((~used).sum())
