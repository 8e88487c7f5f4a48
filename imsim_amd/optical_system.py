"""The optical state of a visit: host-side mirror of imsim/optical_system.py (mock_deviations, OpticalZernikes) and of the
`OptWF` phase screen of imsim/atmPSF.py:37-76, in numpy only.

The residual aberrations the active-optics loop leaves are 19 annular-Zernike coefficients (Z4 .. Z22, in waves at 500 nm) that
vary over the field: 50 optical degrees of freedom are drawn once per visit from the error budget of `aos_sim_results.txt`, the
`sensitivity_matrix.txt` turns them into coefficients at 35 field points, `annular_nominal_coeff.txt` adds the design's own
residuals, and each coefficient is fitted over the field by the first 15 circular Zernikes of the field position in degrees.

For the kernels (include/imsim_hip.h, ims_optical_screen_t) the 19 fits become one 19 x 15 matrix of monomial coefficients in
(thx, thy) and the 19 annular Zernikes one 19 x 28 matrix of monomial coefficients in the normalised pupil position.

The three tables are not packaged: they are read from `<data_dir>/optics_data/` of an imSim data directory (as they are there,
or gzipped with `.gz` appended to the name).
"""
import functools
import math
import os

import numpy as np

from . import _abi, opd

AOS_FILE, MATRIX_FILE, NOMINAL_FILE = "aos_sim_results.txt", "sensitivity_matrix.txt", "annular_nominal_coeff.txt"
N_ZERNIKE = _abi.IMS_OPT_NZ                 # Z4 .. Z22
FIRST_J = 4
N_FIT = 15                                  # circular Zernikes Z1 .. Z15 of the field position
FIELD_DEG, PUPIL_DEG = 4, 6
DEVIATIONS_FUDGE = 3.0                      # atmPSF.py:45
THETA_REMAP = 1.708 / 2.04                  # atmPSF.py:67: no extrapolation beyond the outermost sampling point
R_OUTER, OBSCURATION, LAM0 = 4.18, 0.61, 500.0     # galsim.OpticalScreen(diam=8.36, obscuration=0.61), lam_0 default
OPTICAL_SEED_OFFSET = 314159                # the visit's optical state is seeded by default_rng(seed + 314159)


class OpticsDataError(OSError):
    """a table of optics_data is missing; config.Process turns it into a GalSimConfigError"""


def optics_data_path(data_dir, name):
    if data_dir is None:
        data_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
    path = os.path.join(data_dir, "optics_data", name)
    if not os.path.isfile(path) and os.path.isfile(path + ".gz"):
        return path + ".gz"                    # the same table gzipped (numpy reads it by its suffix)
    if not os.path.isfile(path):
        raise OpticsDataError(f"optics_data file {path} not found (atm_psf.doOpt needs aos_sim_results.txt, sensitivity_matrix.txt "
                              f"and annular_nominal_coeff.txt of an imSim data directory under <data_dir>/optics_data/)")
    return path


@functools.lru_cache(maxsize=8)
def _read_table(path, mtime, skip_header):
    a = np.genfromtxt(path, skip_header=skip_header)
    a.setflags(write=False)
    return a


def read_table(data_dir, name, skip_header=0):
    """one of the three tables, parsed once per file (a focal plane builds the visit's state for every CCD); read-only"""
    path = optics_data_path(data_dir, name)
    return _read_table(path, os.path.getmtime(path), skip_header)


def row(deg, q):
    """IMS_OPT_ROW(deg, q): index of x^0 y^q among the monomials x^p y^q, p + q <= deg, stored row by row in q"""
    return q * (deg + 1) - q * (q - 1) // 2


def n_monomials(deg):
    return (deg + 1) * (deg + 2) // 2


def cartesian_coords():
    """The 35 field sampling points [deg] of the sensitivity matrix: the centre, six spokes of five radii, four raft corners."""
    x, y = [0.0], [0.0]
    for radius in (0.379, 0.841, 1.237, 1.535, 1.708):
        for angle in np.deg2rad([0, 60, 120, 180, 240, 300]):
            x.append(radius * np.cos(angle))
            y.append(radius * np.sin(angle))
    x.extend([1.185, -1.185, -1.185, 1.185])
    y.extend([1.185, 1.185, -1.185, -1.185])
    return np.array(x), np.array(y)


def polar_coords():
    """The same 35 points as (r [deg], theta [rad])"""
    r, th = [0.0], [0.0]
    for radius in (0.379, 0.841, 1.237, 1.535, 1.708):
        for angle in (0, 60, 120, 180, 240, 300):
            r.append(radius)
            th.append(np.deg2rad(angle))
    for x, y in zip((1.185, -1.185, -1.185, 1.185), (1.185, 1.185, -1.185, -1.185)):
        th.append(np.arctan2(y, x))
        r.append(np.sqrt(x * x + y * y))
    return np.array(r), np.array(th)


def aos_std(data_dir=None):
    """per-degree-of-freedom standard deviation over the simulated iterations of aos_sim_results.txt (50 rows, one header line)"""
    aos = read_table(data_dir, AOS_FILE, skip_header=1)
    if aos.shape[0] != 50:
        raise ValueError(f"{AOS_FILE}: 50 rows expected, {aos.shape[0]} found")
    return np.std(aos, axis=1)


def mock_deviations(seed=None, data_dir=None):
    """50 random optical deviations, normal with mean 0 and the standard deviations of aos_std().  For an integer seed the
    values are those of the reference's `np.random.seed(seed); np.random.normal(0, std)` (the same MT19937 stream)."""
    return np.random.RandomState(seed).normal(0.0, aos_std(data_dir))


# ---------------- Zernikes as Cartesian monomials ----------------
def _poly_mul(a, b):
    out = {}
    for (pa, qa), ca in a.items():
        for (pb, qb), cb in b.items():
            k = (pa + pb, qa + qb)
            out[k] = out.get(k, 0) + ca * cb
    return out


def zernike_monomials(js, eps, deg):
    """[len(js), n_monomials(deg)]: Noll terms js of the Zernikes orthonormal over the annulus eps <= rho <= 1 (eps = 0: the
    circular ones, GalSim's normalisation) as coefficients of x^p y^q at row(deg, q) + p.  rho^k cos(m t) is
    (x^2 + y^2)^((k - m) / 2) Re (x + i y)^m and the sine term its imaginary part, multiplied out in integers; the radial
    coefficients are those of opd.zernike_table (exact rational Gram-Schmidt)."""
    nm = [opd.noll_to_nm(j) for j in js]
    radial = opd._radial_table(max(n for n, _ in nm), float(eps))
    r2 = {(2, 0): 1, (0, 2): 1}
    out = np.zeros((len(js), n_monomials(deg)))
    for i, (n, m) in enumerate(nm):
        if n > deg:
            raise ValueError(f"Zernike of order {n} does not fit monomials of degree {deg}")
        am = abs(m)
        re, im = {(0, 0): 1}, {}
        for _ in range(am):                               # (re + i im) (x + i y)
            re, im = ({k: v for k, v in _sum(_poly_mul(re, {(1, 0): 1}), _poly_mul(im, {(0, 1): -1})).items()},
                      {k: v for k, v in _sum(_poly_mul(re, {(0, 1): 1}), _poly_mul(im, {(1, 0): 1})).items()})
        ang = re if m >= 0 else im
        coef = radial[(n, am)] * (math.sqrt(2.0) if m != 0 else 1.0)
        rp = {(0, 0): 1}                                  # (x^2 + y^2)^((k - m) / 2), k = am, am + 2, ...
        for k in range(am, n + 1, 2):
            for (p, q), v in _poly_mul(rp, ang).items():
                out[i, row(deg, q) + p] += coef[k] * v
            rp = _poly_mul(rp, r2)
    return out


def _sum(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0) + v
    return out


def monomial_values(deg, x, y):
    """[n_monomials(deg), *x.shape]: x^p y^q in the order of row()"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = np.empty((n_monomials(deg),) + x.shape)
    for q in range(deg + 1):
        for p in range(deg - q + 1):
            out[row(deg, q) + p] = x ** p * y ** q
    return out


def pupil_matrix(eps=OBSCURATION):
    """19 x 28: annular Z4 .. Z22 as monomials of the normalised pupil position"""
    return zernike_monomials(range(FIRST_J, FIRST_J + N_ZERNIKE), eps, PUPIL_DEG)


class OpticalZernikes:
    """One state of the optics (imsim/optical_system.py OpticalZernikes): sampling_coeff [19, 35] at the field sampling points
    and its least-squares fit by the circular Zernikes Z1 .. Z15 of the field position in degrees (unscaled, as
    galsim.zernike.zernikeBasis(15, x, y) evaluates them)."""

    def __init__(self, deviations=None, data_dir=None, nominal=True):
        self.sensitivity = read_table(data_dir, MATRIX_FILE).reshape((35, N_ZERNIKE, 50))
        self.nominal_coeff = read_table(data_dir, NOMINAL_FILE)
        if self.nominal_coeff.shape != (N_ZERNIKE, 35):
            raise ValueError(f"{NOMINAL_FILE}: shape (19, 35) expected, {self.nominal_coeff.shape} found")
        if not nominal:
            self.nominal_coeff = np.zeros_like(self.nominal_coeff)
        self.cartesian_coords = cartesian_coords()
        self.deviations = mock_deviations(data_dir=data_dir) if deviations is None else np.asarray(deviations, dtype=np.float64)
        if self.deviations.shape != (50,):
            raise ValueError(f"50 optical deviations expected, shape {self.deviations.shape} given")
        self.deviation_coeff = np.dot(self.sensitivity, self.deviations).transpose()
        self.sampling_coeff = np.add(self.deviation_coeff, self.nominal_coeff)
        x, y = self.cartesian_coords
        self.fit_monomials = zernike_monomials(range(1, N_FIT + 1), 0.0, FIELD_DEG)         # [15 Zernikes, 15 monomials]
        basis = self.fit_monomials @ monomial_values(FIELD_DEG, x, y)                        # [15, 35]
        self.fit_coeff = np.stack([np.linalg.lstsq(basis.T, c, rcond=None)[0] for c in self.sampling_coeff])   # [19, 15]
        self.field_matrix = self.fit_coeff @ self.fit_monomials                             # [19, 15 monomials of (thx, thy)]

    @property
    def polar_coords(self):
        return polar_coords()

    def cartesian_coeff(self, fp_x, fp_y):
        """the 19 coefficients of Z4 .. Z22 at field position (fp_x, fp_y) [deg] (scalars or arrays)"""
        return np.tensordot(self.field_matrix, monomial_values(FIELD_DEG, fp_x, fp_y), axes=1)

    def polar_coeff(self, fp_r, fp_t):
        return self.cartesian_coeff(fp_r * np.cos(fp_t), fp_r * np.sin(fp_t))

    def screen_struct(self):
        """the device block: _abi.OpticalScreen"""
        S = _abi.OpticalScreen()
        fm, pm = np.ascontiguousarray(self.field_matrix), pupil_matrix()
        for j in range(N_ZERNIKE):
            for t in range(_abi.IMS_OPT_NFIELD):
                S.field[j][t] = float(fm[j, t])
            for t in range(_abi.IMS_OPT_NPUPIL):
                S.pupil[j][t] = float(pm[j, t])
        S.r_outer, S.remap, S.lam0 = R_OUTER, THETA_REMAP, LAM0
        S.inv_r = 1.0 / R_OUTER
        S.grad_scale = LAM0 * S.inv_r
        return S


def visit_optical_state(seed, data_dir=None, deviations=None, nominal=True):
    """The OpticalZernikes of a visit (OptWF, atmPSF.py:37-47).  The reference takes the seed of mock_deviations from the
    GalSim stream of the atm_psf input, which cannot be reproduced; here it comes from a generator of its own,
    default_rng(seed + OPTICAL_SEED_OFFSET) -- NOT from the stream AtmosphericPSF draws the atmosphere from (seed + 271828),
    so the atmosphere of a visit is the same with and without doOpt.  Explicit `deviations` are used as given (no fudge)."""
    if deviations is None:
        mock_seed = int(np.random.default_rng(int(seed) + OPTICAL_SEED_OFFSET).random() * 2 ** 31)
        deviations = DEVIATIONS_FUDGE * mock_deviations(mock_seed, data_dir)
    return OpticalZernikes(deviations, data_dir=data_dir, nominal=nominal)
