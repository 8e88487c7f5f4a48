"""ims_psf_adaptive / psf_map.adaptive on the GPU: one pass against the photon pool of the same rows reduced in np.longdouble,
the converged result against the numpy restatement iterated on that pool, closed forms, determinism, edge rows, the other
kernel variants, unequal weights, and `moments: adaptive` through the config driver.

The rows, scenes and the pool are those of tests/test_psf_map_gpu.py; the restatement is tests/adaptive_moments_ref.py.

The bound of the one-pass tests
-------------------------------
Reference: T = sum_i tau_i over the photons of the pool that arrived, tau_i = g_i m_i the exact term with g = w exp(-q / 2),
q = rho2 and m one of 1, u, v, u u, u v, v v, q q, formed and added in np.longdouble from the pool's f64 values and the f64
state.  Kernel: the f64 records of the row's segments (the device's sums over 256 photons), added here in longdouble.  U = 2^-53.

* the offsets.  dx = fl(x - x0_row) and u = fl(dx - x0) are one rounding each (the first is exact in stage psf, whose rows have
  x0_row = 0), so |u^ - u| <= eps_u = U (|dx| + |u|): an absolute error -- u is a difference and may cancel.  Likewise eps_v.
* the argument.  N = Myy u u - 2 Mxy u v + Mxx v v is three products of three factors (the exact doubling aside) and two
  additions: at most 5 roundings on any path, |N^ - N| <= gamma_5 Nabs, Nabs the sum of the absolute products.  det = Mxx Myy -
  Mxy Mxy: gamma_2 detabs.  One division.  With the offsets' errors carried through dq/du = 2 (Myy u - Mxy v) / det and
  dq/dv = 2 (Mxx v - Mxy u) / det:
      dq = (gamma_6 Nabs + gamma_3 |N| detabs / det) / det + |dq/du| eps_u + |dq/dv| eps_v .
  -q / 2 is exact.  exp turns an absolute error d of its argument into the relative error e^d - 1 of its value.  (Where the error
  is relative to q, d = q delta / 2, this is the familiar q / 2 e^(-q / 2) delta <= delta / e of the weight; the bound uses each
  photon's own q instead of the maximum 1 / e, which is never larger, and so also covers the part of dq that the offsets bring.)
* exp itself.  ims::dexp is good to 2 U relative for arguments above -693.49 (tests/test_math_spec.py::test_exp_is_good_to_two_u,
  on the points of tests/math_spec_cases.py); below -1000.5 ln 2 = -693.4938 it returns exactly 0.  For a photon whose argument
  is below -693.49 the error is therefore at most tau_i itself: |tau_i| is counted once more for it, and e^-693.49 w |m| on top
  (a term below 1e-290 of any sum here).
* the term.  w exp rounds once; g u and (g u) u round once each (g q q likewise): with exp's 2 U, gamma_5 |tau|.  The factor m
  carries the offsets' errors: dm = eps_u for u, 2 |u| eps_u for u u, |u| eps_v + |v| eps_u for u v, 2 q dq for q q.
      |t_i - tau_i| <= |tau_i| (expm1(dq / 2) + gamma_5) + g_i dm_i          (first order; the products of these errors are
  below 2^-45 of it and are covered by gamma_6, gamma_3 for the gamma_5, gamma_2 counted above and gamma_5 + U here).
* the sum.  The device adds a segment's terms through 6 butterfly levels and 3 additions; test_psf_map_gpu.bound(n, sum |tau_i|)
  allows gamma_{18 + ceil(n_seg / 256) + 4} and the reference's own (n + 4) 2^-64 -- more additions than happen here, so it holds.

  |S - T| <= bound(n, sum |tau_i|) + sum_i [ |tau_i| (expm1(dq_i / 2) + gamma_6) + g_i dm_i ]   with no fitted constant.

The counts are integers and must be equal."""
import dataclasses
import math
import os

import numpy as np
import pytest

import adaptive_moments_ref as ref
import photon_ops_cases as ops_cases
import test_psf_map_gpu as PM
import test_psf_profile_gpu as PP
from test_psf_map_gpu import renderers, torch_cuda                      # noqa: F401  (fixtures)
from imsim_amd import _abi, config, configs, fits_io, psf_map

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
U = 2.0 ** -53
N_ROWS = 40
_CACHE = {}


def gamma(k):
    return k * U / (1.0 - k * U)


def rows_and_pool(renderers, stage):
    """(scene, renderer, the 40 rows, (dx, dy, flux, offsets) of their pool), computed once per stage and left unchanged"""
    if stage not in _CACHE:
        sc, r, rows = PP.rows_of(renderers, stage, N_ROWS)
        assert set(rows["n_phot"]) == set(PM.COUNTS) and (rows["phot_first"] > 2 ** 32).sum() == 10
        _CACHE[stage] = (sc, r, rows, raw_pool(r, rows))
    return _CACHE[stage]


def raw_pool(r, rows):
    """(x, y, flux, offsets per row) of the rows' photons from the unconverted pool; the offsets dx = x - x0 are formed by the user"""
    pool = r.shoot_ops_photons(rows, converted=False)
    r.synchronize()
    pool = pool.to_host()
    return pool["x"], pool["y"], pool["flux"], np.concatenate([[0], np.cumsum(rows["n_phot"])])


def row_photons(rows, pool, i):
    """(dx, dy in longdouble as the reference takes them, dx, dy as the device's f64 subtraction leaves them, flux) of row i"""
    x, y, w, offs = pool
    sl = slice(offs[i], offs[i + 1])
    return (x[sl].astype(LD) - LD(rows["x0"][i]), y[sl].astype(LD) - LD(rows["y0"][i]), x[sl] - rows["x0"][i], y[sl] - rows["y0"][i],
            w[sl])


def given_states(rows, pool):
    """A state for every row that is not its fixed point: the centre a third of a sigma off the row's unweighted centroid, the
    matrix that of the long row 6 (its unweighted half-trace m) made elliptical and tilted: m (1.2, 0.2, 0.9)"""
    dx, dy, _, _, w = row_photons(rows, pool, 6)
    m = float(ref.unweighted_start(dx, dy, w)[2])
    state = np.zeros((len(rows), 5))
    for i in range(len(rows)):
        dx, dy, _, _, w = row_photons(rows, pool, i)
        start = ref.unweighted_start(dx, dy, w)
        cx, cy = (0.0, 0.0) if start is None else (float(start[0]), float(start[1]))
        state[i] = (cx + 0.3 * math.sqrt(m), cy - 0.2 * math.sqrt(m), 1.2 * m, 0.2 * m, 0.9 * m)
    return state


def one_pass_bound(dxl, dyl, dx64, dy64, w, state, n_phot):
    """(T [7], bound [7]) of the module docstring for one row"""
    ok = w != 0
    dxl, dyl, dx64, dy64, wl = dxl[ok], dyl[ok], np.abs(dx64[ok]).astype(LD), np.abs(dy64[ok]).astype(LD), w[ok].astype(LD)
    x0, y0, mxx, mxy, myy = (LD(t) for t in state)
    u, v = dxl - x0, dyl - y0
    eps_u, eps_v = U * (dx64 + np.abs(u)), U * (dy64 + np.abs(v))
    det, detabs = mxx * myy - mxy * mxy, abs(mxx * myy) + mxy * mxy
    n_abs = abs(myy) * u * u + 2 * abs(mxy) * np.abs(u * v) + abs(mxx) * v * v
    q = (myy * u * u - 2 * mxy * u * v + mxx * v * v) / det
    dq = (gamma(6) * n_abs + gamma(3) * np.abs(q) * detabs) / det + 2 * np.abs(myy * u - mxy * v) / det * eps_u \
        + 2 * np.abs(mxx * v - mxy * u) / det * eps_v
    g = wl * np.exp(-q / 2)
    g_abs = np.abs(g)
    flushed = -q / 2 < LD(-693.49)
    floor = np.where(flushed, np.abs(wl) * np.exp(LD(-693.49)), 0)
    au, av = np.abs(u), np.abs(v)
    ms = (np.ones_like(u), u, v, u * u, u * v, v * v, q * q)
    dms = (np.zeros_like(u), eps_u, eps_v, 2 * au * eps_u, au * eps_v + av * eps_u, 2 * av * eps_v, 2 * np.abs(q) * dq)
    T, B = [], []
    for m, dm in zip(ms, dms):
        tau = g * m
        a = np.abs(tau)
        per = a * (np.expm1(dq / 2) + gamma(6)) + g_abs * dm + np.where(flushed, a + floor * np.abs(m), 0)
        T.append(tau.sum())
        B.append(LD(PM.bound(n_phot, a.sum())) + per.sum())
    return T, B


def device_row_sums(run, rows, i, prefix):
    """the row's ten totals from the per-segment records the pass left in the scratch, added in longdouble"""
    part = run.partial.cpu().numpy()[:10 * run.n_segments].reshape(-1, 10)
    return part[prefix[i]:prefix[i + 1]].astype(LD).sum(axis=0)


def check_one_pass(r, rows, pool, stage, what):
    """one round from given_states: the seven sums within the bound, sum w and the counts exact, the update as the reference's"""
    state = given_states(rows, pool)
    run = psf_map.PreparedAdaptive(r, rows, stage, state, np.ones(len(rows), dtype=np.int32), tol=1e-6, max_iter=1)
    run.rounds(1)
    new_state, status, aux = run.raw()
    prefix = np.concatenate([[0], np.cumsum(-(-rows["n_phot"] // 256))])
    worst = 0.0
    for i in range(len(rows)):
        dxl, dyl, dx64, dy64, w = row_photons(rows, pool, i)
        S = device_row_sums(run, rows, i, prefix)
        T, B = one_pass_bound(dxl, dyl, dx64, dy64, w, state[i], rows["n_phot"][i])
        used, dropped = int((w != 0).sum()), int((w == 0).sum())
        assert (S[8], S[9]) == (used, dropped) == (aux[i, 2], aux[i, 3]), (what, i)
        wb = PM.bound(rows["n_phot"][i], np.abs(w).sum())
        assert abs(S[7] - w.astype(LD).sum()) <= wb and abs(LD(aux[i, 1]) - w.astype(LD).sum()) <= wb, (what, i)
        if used == 0:
            assert status[i].tolist() == [3, 0] and np.all(np.isnan(new_state[i])), (what, i)
            continue
        for k in range(7):
            err = abs(S[k] - T[k])
            worst = max(worst, float(err / B[k]))
            assert err <= B[k], (what, i, ref.NAMES[k], float(err), float(B[k]))
        step = ref.update(state[i], T)
        if step is None:                                  # the update fails: the state stays
            assert status[i].tolist() == [2, 0] and new_state[i].tobytes() == state[i].tobytes(), (what, i)
            continue
        assert status[i, 1] == 1 and status[i, 0] == (0 if step[1] < 1e-6 else 1), (what, i)
        b2 = float(min(np.linalg.eigvalsh([[state[i, 2], state[i, 3]], [state[i, 3], state[i, 4]]])))
        want = np.array([float(t) for t in step[0]])
        scale = np.array([math.sqrt(b2), math.sqrt(b2), b2, b2, b2])
        # (the update divides by A: the sums' bounds relative to A, amplified by at most 4 / b2 (u u) scale, stay far below 1e-9)
        assert np.all(np.abs(new_state[i] - want) <= 1e-9 * scale), (what, i)
        assert abs(aux[i, 0] - float(step[2])) <= 1e-9 * float(step[2]), (what, i)
    print(f"{what}: worst error / bound {worst:.3g} over {len(rows)} rows")
    return worst


@pytest.mark.parametrize("stage", ["psf", "ops"])
def test_one_pass_against_the_pool(renderers, stage):
    """40 rows with every photon count of the table (1, 63, 64, 65, 257, 1000, 2^16 + 1), every fourth based above 2^32: after
    ims_psf_adaptive with n_rounds = 1 from a given state, the seven sums agree with the longdouble reduction of the same
    photons within the bound of the module docstring; sum w within test_psf_map_gpu's bound; the counts are equal."""
    sc, r, rows, pool = rows_and_pool(renderers, stage)
    check_one_pass(r, rows, pool, stage, f"one pass, stage {stage}")


def compare_converged(got, rows, pool, tol, what, start=None):
    """rows of adaptive() against the reference iterated on the pool's photons: 1e-8 relative to b2 (lengths to sqrt(b2))"""
    n_conv = 0
    for i in range(len(rows)):
        dxl, dyl, _, _, w = row_photons(rows, pool, i)
        want = ref.iterate(dxl, dyl, w, start=None if start is None else start[i], tol=tol, max_iter=100)
        g = got[i]
        assert (g["status"], g["n_used"], g["n_dropped"]) == (want["status"], want["n_used"], want["n_dropped"]), (what, i)
        if want["status"] in (ref.EMPTY, ref.FAILED):
            continue
        n_conv += want["status"] == ref.CONVERGED
        mxx, mxy, myy = float(want["Mxx"]), float(want["Mxy"]), float(want["Myy"])
        b2 = 0.5 * (mxx + myy - math.sqrt((mxx - myy) ** 2 + 4.0 * mxy * mxy))
        for f, scale in (("xbar", math.sqrt(b2)), ("ybar", math.sqrt(b2)), ("sigma", math.sqrt(b2)), ("Mxx", b2), ("Mxy", b2), ("Myy", b2),
                         ("e1", 1.0), ("e2", 1.0), ("rho4", 1.0)):
            assert abs(g[f] - float(want[f])) <= 1e-8 * scale, (what, i, f, g[f], float(want[f]))
        assert g["fwhm"] == 2.3548200450309493 * g["sigma"]
    return n_conv


@pytest.mark.parametrize("stage", ["psf", "ops"])
def test_converged_result_against_the_reference(renderers, stage):
    """the same rows through psf_map.adaptive with tol = 1e-10: state, sigma, e1, e2 and rho4 agree with the reference iterated
    on the pool's photons to 1e-8 relative to b2 -- both locate the same fixed point to their threshold -- and status, n_used
    and n_dropped are equal"""
    sc, r, rows, pool = rows_and_pool(renderers, stage)
    got = psf_map.adaptive(sc, rows, stage=stage, tol=1e-10, renderer=r)
    n_conv = compare_converged(got, rows, pool, 1e-10, f"converged, stage {stage}")
    print(f"stage {stage}: {n_conv} of {len(rows)} rows converged, iterations {sorted(set(got['iter'].tolist()))}")
    assert n_conv >= 30 and np.all(got["status"][rows["n_phot"] == 1] == 2)
    unweighted = psf_map.compute(sc, rows, stage=stage, renderer=r)
    assert np.array_equal(got["n_used"], unweighted["n_used"]) and np.array_equal(got["flux"], unweighted["flux"])


@pytest.mark.parametrize("name", ["gaussian", "double_gaussian"])
def test_closed_forms(torch_cuda, name):
    """A Gaussian, and the DoubleGaussian component, in stage psf with 2^18 photons.  Row 0 holds them all; rows 1 .. 16 are its
    16 disjoint groups of 2^14 (the same random stream, phot_first advanced), whose scatter divided by 4 is the standard error.
    Gaussian: Mxx, Myy within 5 standard errors of sigma^2, Mxy of 0, rho4 of 2.  DoubleGaussian: Mxx, Myy within 5 standard
    errors of the mixture's root, and the adaptive sigma is below the unweighted one."""
    n, g = 1 << 18, 1 << 14
    if name == "gaussian":
        s = 0.7 / 2.3548200450309493
        psf, m = [(_abi.IMS_PSF_GAUSSIAN, 0, s, 0.0, 1.0)], s * s
    else:
        comp, _, _ = config.double_gaussian_psf(0.8)
        s1, s2, f1 = comp[2], comp[5], comp[6]
        psf, m = [comp], float(ref.mixture_root([s1 * s1, s2 * s2], [f1, 1.0 - f1]))
    scene = psf_map._as_scene(psf)
    rows = psf_map.point_rows(scene, np.zeros((17, 2)), [n] + [g] * 16, "psf", wavelength=620.0)
    rows["obj_id"] = 0
    rows["phot_first"] = [0] + [g * k for k in range(16)]
    r = psf_map.renderer_for(scene, seed=398414)
    a = psf_map.adaptive(scene, rows, stage="psf", renderer=r)
    assert np.all(a["status"] == 0) and a["n_used"].tolist() == [n] + [g] * 16 and np.all(a["n_dropped"] == 0)
    se = {f: float(np.std(a[f][1:], ddof=1)) / 4.0 for f in ("Mxx", "Myy", "Mxy", "rho4", "sigma")}
    full = a[0]
    print(name, {f: (float(full[f]), se[f]) for f in se}, "expected M", m, "iterations", int(full["iter"]))
    assert abs(full["Mxx"] - m) <= 5.0 * se["Mxx"] and abs(full["Myy"] - m) <= 5.0 * se["Myy"] and abs(full["Mxy"]) <= 5.0 * se["Mxy"]
    if name == "gaussian":
        assert abs(full["rho4"] - 2.0) <= 5.0 * se["rho4"]
    else:
        unweighted = psf_map.compute(scene, rows[:1], stage="psf", renderer=r)[0]
        print("unweighted sigma", float(unweighted["sigma"]), "adaptive sigma", float(full["sigma"]))
        assert full["sigma"] + 5.0 * se["sigma"] < unweighted["sigma"] and full["rho4"] > 2.0 + 5.0 * se["rho4"]


@pytest.mark.parametrize("stage", ["psf", "ops"])
def test_determinism(renderers, stage):
    """bit-identical: the rows permuted; a row alone (a long one and a short one); 16 rounds delivered at once or as 4 x 4"""
    sc, r, rows, pool = rows_and_pool(renderers, stage)
    a = psf_map.adaptive(sc, rows, stage=stage, renderer=r)
    b = psf_map.adaptive(sc, rows, stage=stage, renderer=r)
    assert a.tobytes() == b.tobytes() and (a["status"] == 0).sum() >= 30
    perm = np.random.default_rng(5).permutation(len(rows))
    c = psf_map.adaptive(sc, rows[perm].copy(), stage=stage, renderer=r)
    assert c.tobytes() == a[perm].tobytes()
    for i in (6, 3):
        alone = psf_map.adaptive(sc, rows[i:i + 1].copy(), stage=stage, renderer=r)
        assert alone.tobytes() == a[i:i + 1].tobytes(), i
    state = given_states(rows, pool)
    runs = []
    for batches in ((16,), (4, 4, 4, 4)):
        run = psf_map.PreparedAdaptive(r, rows, stage, state, np.ones(len(rows), dtype=np.int32), tol=1e-12, max_iter=16)
        for k in batches:
            run.rounds(k)
        runs.append(run.raw())
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()
    assert runs[0][1][:, 1].max() > 4                       # rows that were still being iterated across the batch boundaries


def test_edge_rows_in_one_call(renderers):
    """n_phot = 0 and a row whose photons are all vignetted (test_psf_map_gpu.test_all_photons_lost's point): status 3, NaN.  One
    photon: status 2.  Their neighbours are what they are without them.  A row frozen at entry -- whatever its status -- is not
    changed by further rounds, nor is a converged one."""
    sc, r = renderers["ops"]
    singles = psf_map.point_rows(sc, np.tile([[25.0, 31.0]], (8, 1)), 1, "ops")
    singles["obj_id"], singles["phot_first"] = 0, np.arange(8)
    arrived = np.flatnonzero(psf_map.compute(sc, singles, stage="ops", renderer=r)["n_used"] == 1)
    xy = np.array([[20.5, 30.25], [6.0e4, 32.0], [40.0, 12.5], [25.0, 31.0], [11.0, 50.0]])
    rows = psf_map.point_rows(sc, xy, [1000, 1000, 0, 1, 700], "ops")
    rows["obj_id"][3], rows["phot_first"][3] = 0, arrived[0]
    a = psf_map.adaptive(sc, rows, stage="ops", renderer=r)
    r.synchronize()                                   # (raises on a device-side error)
    assert a["status"].tolist() == [0, 3, 3, 2, 0] and a["iter"][[1, 2, 3]].tolist() == [0, 0, 0]
    assert (a["n_used"][1], a["n_dropped"][1], a["flux"][1]) == (0, 1000, 0.0) and (a["n_used"][2], a["n_dropped"][2]) == (0, 0)
    assert (a["n_used"][3], a["n_dropped"][3]) == (1, 0)
    for f in ("xbar", "ybar", "Mxx", "Myy", "Mxy", "sigma", "e1", "e2", "rho4", "fwhm"):
        assert np.isnan(a[f][1]) and np.isnan(a[f][2]), f
    others = psf_map.adaptive(sc, rows[[0, 4]].copy(), stage="ops", renderer=r)
    assert a[[0, 4]].tobytes() == others.tobytes() and np.all(a["sigma"][[0, 4]] > 0.1)
    with_guess = psf_map.adaptive(sc, rows, stage="ops", guess_sigma=float(a["sigma"][0]), max_iter=5, renderer=r)
    assert with_guess["status"].tolist()[1:4] == [3, 3, 1] and with_guess["iter"][3] == 5     # one photon: the weight shrinks for ever
    # the device finds an empty row by itself when the host did not mark it
    state = np.tile([0.0, 0.0, 2.0, 0.0, 2.0], (5, 1))
    state[[0, 4], 0], state[[0, 4], 1] = a["xbar"][[0, 4]] + 0.3, a["ybar"][[0, 4]] - 0.2
    run = psf_map.PreparedAdaptive(r, rows, "ops", state, np.ones(5, dtype=np.int32), tol=1e-6, max_iter=40)
    run()
    st, status, aux = run.raw()
    assert status[[0, 1, 2, 4], 0].tolist() == [0, 3, 3, 0] and status[3, 0] in (1, 2) and np.all(np.isnan(st[[1, 2]])) and aux[1].tolist()[1:] == [0.0, 0.0, 1000.0]
    run.rounds(3)
    again = run.raw()
    assert again[0][[0, 1, 2, 4]].tobytes() == st[[0, 1, 2, 4]].tobytes() and again[1][[0, 1, 2, 4]].tobytes() == status[[0, 1, 2, 4]].tobytes()
    assert again[2][[0, 1, 2, 4]].tobytes() == aux[[0, 1, 2, 4]].tobytes()
    # frozen at entry, with a state that no update would leave alone
    odd = np.tile([0.5, -0.5, 3.0, 0.5, 1.0], (5, 1))
    for frozen in (0, 2, 3):
        entry = np.array([frozen, 1, frozen, frozen, 1], dtype=np.int32)
        run = psf_map.PreparedAdaptive(r, rows, "ops", odd, entry, tol=1e-6, max_iter=8)
        run.rounds(8)
        st, status, aux = run.raw()
        assert st[[0, 2, 3]].tobytes() == odd[[0, 2, 3]].tobytes() and status[[0, 2, 3]].tolist() == [[frozen, 0]] * 3
        assert np.all(np.isnan(aux[[0, 2, 3], 0])) and np.all(aux[[0, 2, 3], 1:] == 0.0)
        assert status[1].tolist() == [3, 0] and status[4, 1] > 0 and st[4].tobytes() != odd[4].tobytes()


@pytest.mark.parametrize("which", ["perturbed", "doOpt", "bandpass_ratio"])
def test_other_kernel_variants_against_their_own_pools(torch_cuda, which):
    """A perturbed telescope (stage ops, the loops over surfaces in their frames), the optical phase screen (stage psf, the
    component's LDS set up per row) and a chain with a BandpassRatio behind it, whose photons carry unequal weights: one pass
    within the bound and the converged result as the reference's, each against the pool of its own scene."""
    if which == "perturbed":
        sc, stage = PP.perturbed_scene(), "ops"
        rows = psf_map.point_rows(sc, np.array([[30.0, 20.0], [12.0, 44.0]]), [5000, 300], stage)
    elif which == "doOpt":
        sc, stage = PP.doopt_scene(), "psf"
        rows = psf_map.point_rows(sc, np.array([[10.0, 20.0], [50.0, 40.0]]), [5000, 300], stage, wavelength=620.0)
        rows["atm_tan_x"], rows["atm_tan_y"] = np.radians([1.0, -0.5]), 0.0
        rows["x0"], rows["y0"] = 0.0, 0.0
    else:
        t, wl_min, wl_step = ops_cases.ratio_tables()
        sc = configs.scene_c3(nx=64, ny=64, sensor=False)
        sc = dataclasses.replace(sc, ops=list(sc.ops) + [(_abi.IMS_OP_BANDPASS_RATIO, 1, [])], ratio_tables=t, ratio_wl_min=wl_min,
                                 ratio_wl_step=wl_step)
        stage = "ops"
        rows = psf_map.point_rows(sc, np.array([[30.0, 20.0], [12.0, 44.0]]), [5000, 300], stage)
    r = psf_map.renderer_for(sc)
    pool = raw_pool(r, rows)
    if which == "bandpass_ratio":
        w = pool[2][pool[2] != 0]
        assert len(np.unique(w)) > 100 and w.max() - w.min() > 0.1                  # the weights are unequal
    state = given_states_small(rows, pool)
    check_pass_small(r, rows, pool, stage, state, which)
    got = psf_map.adaptive(sc, rows, stage=stage, tol=1e-10, renderer=r)
    n_conv = compare_converged(got, rows, pool, 1e-10, which)
    # (the doOpt scene's PSF is the image of the pupil annulus under astigmatism and defocus, a ring: no Gaussian weight matches it
    # and neither side converges -- they walk the same 100 rounds, and their status 1 and states are compared all the same)
    assert n_conv == (0 if which == "doOpt" else 2) and np.all(got["n_used"] > 250)
    if which == "bandpass_ratio":
        assert abs(got["flux"][0] - pool[2][:5000].astype(LD).sum()) < 1e-9 and got["flux"][0] != got["n_used"][0]


def given_states_small(rows, pool):
    """given_states for a table without the long row 6: every row's own half-trace"""
    state = np.zeros((len(rows), 5))
    for i in range(len(rows)):
        dxl, dyl, _, _, w = row_photons(rows, pool, i)
        cx, cy, m = (float(t) for t in ref.unweighted_start(dxl, dyl, w)[:3])
        state[i] = (cx + 0.3 * math.sqrt(m), cy - 0.2 * math.sqrt(m), 1.2 * m, 0.2 * m, 0.9 * m)
    return state


def check_pass_small(r, rows, pool, stage, state, what):
    run = psf_map.PreparedAdaptive(r, rows, stage, state, np.ones(len(rows), dtype=np.int32), tol=1e-6, max_iter=1)
    run.rounds(1)
    _, status, aux = run.raw()
    prefix = np.concatenate([[0], np.cumsum(-(-rows["n_phot"] // 256))])
    worst = 0.0
    for i in range(len(rows)):
        dxl, dyl, dx64, dy64, w = row_photons(rows, pool, i)
        S = device_row_sums(run, rows, i, prefix)
        T, B = one_pass_bound(dxl, dyl, dx64, dy64, w, state[i], rows["n_phot"][i])
        assert (S[8], S[9]) == (int((w != 0).sum()), int((w == 0).sum())) == (aux[i, 2], aux[i, 3]), (what, i)
        assert abs(S[7] - w.astype(LD).sum()) <= PM.bound(rows["n_phot"][i], np.abs(w).sum()), (what, i)
        for k in range(7):
            err = abs(S[k] - T[k])
            worst = max(worst, float(err / B[k]))
            assert err <= B[k], (what, i, ref.NAMES[k], float(err), float(B[k]))
        assert status[i, 1] == 1
    print(f"{what}: worst error / bound {worst:.3g}")


def test_config_end_to_end(torch_cuda, tmp_path):
    """A one-CCD visit with output.psf_map (nx 2, 2000 photons, stage ops), once with `moments: adaptive` and once without: 24
    planes against 12, the first 12 bit-identical, the header naming PLANE13 .. PLANE24 and carrying TOL and MAXITER, every point
    converged to a sigma below its unweighted one."""
    files = {}
    for key, extra in (("plain", {}), ("adaptive", {"moments": "adaptive", "tolerance": 1e-7, "max_iter": 60})):
        out = tmp_path / key
        o = {"input.instance_catalog.file_name": os.path.join(HERE, "golden", "example_instcat_subset.txt"),
             "image.nobjects": 3, "stamp.draw_method": "phot", "output.dir": str(out),
             "output.psf_map": dict({"file_name": "psf_map.fits", "nx": 2, "n_photons": 2000, "stage": "ops"}, **extra)}
        res = config.Process(os.path.join(HERE, "data", "test-config-instcat.yaml"), template_dirs=[os.path.join(HERE, "data")], overrides=o)
        fn = str(out / "psf_map.fits")
        assert fn in res.files
        files[key] = fits_io.read_fits(fn)
    (h0, d0), = files["plain"]
    (h1, d1), = files["adaptive"]
    assert d0.shape == (12, 2, 2) and d1.shape == (24, 2, 2) and d1[:12].tobytes() == d0.tobytes()
    assert "PLANE13" not in h0 and "TOL" not in h0 and "MAXITER" not in h0
    assert all(h1[k] == h0[k] for k in [f"PLANE{k}" for k in range(1, 13)] + ["STAGE", "NPHOT", "DET_NAME", "UNITS", "WAVELEN", "X_STEP"])
    assert [h1[f"PLANE{13 + k}"] for k in range(12)] == [name for name, _ in psf_map.ADAPTIVE_PLANES]
    assert (h1["TOL"], h1["MAXITER"]) == (1e-7, 60)
    names = [name for name, _ in psf_map.ADAPTIVE_PLANES]
    status, sigma, a_iter = d1[12 + names.index("a_status")], d1[12 + names.index("a_sigma")], d1[12 + names.index("a_iter")]
    assert np.all(status == 0) and np.all(a_iter >= 1) and np.all(a_iter < 60)
    assert np.all(sigma > 0.2) and np.all(sigma < d1[8])                 # below the unweighted sigma of the same photons
    assert np.all(d1[12 + names.index("a_fwhm")] == 2.3548200450309493 * sigma)
