"""tests/spike_ref.py -- the np.longdouble statement of the FFT branch's spike step -- against the reference's golden vectors,
and the oracle (oracle/orc_fft.c, which the GPU test holds the kernels to bit for bit) against it on every planted case of
tests/spike_cases.py.  The conditions the reference's bounds rest on (the near-decision cap, the planted boxes) and its teeth
are checked here on the reference alone."""
import math
import os

import numpy as np
import pytest

import spike_cases as sc
import spike_ref as sr
from imsim_amd import _abi, diffraction_fft as dfft
from oracle import orc_loader

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diffraction_fft_golden.npz")
LD = np.longdouble
_REF = {}


def reference(shape, geom):
    """the reference on a case, computed once"""
    if (shape, geom) not in _REF:
        c = sc.case(shape, geom)
        _REF[shape, geom] = sr.apply(c.S, c.rows, c.rbuf)
    return _REF[shape, geom]


def oracle(S, rbuf_raw=0):
    from imsim_amd.engine import Scene
    orc = orc_loader.OracleFft(Scene(nx=64, ny=64, seed=1), [], add_noise=False)
    orc.P.spikes = S
    orc.P.rbuf_raw = rbuf_raw
    return orc


def _spikes(w, lam, alpha, d_alpha, norm=1.0):
    return _abi.Spikes(1, int(w), 1e5, math.cos(alpha - d_alpha / 2), math.sin(alpha - d_alpha / 2), alpha - d_alpha, d_alpha,
                       dfft.SPIKE_WAVELENGTH / lam, dfft.SPIKE_R0, norm)


def test_reference_stencil_matches_the_golden_stencils():
    """prepare_psf_field_rotation's output for three (wavelength, alpha, d_alpha): the reference stencil over its own long-double
    sum, to the 2e-15 tests/test_fft_cpu.py holds the host's and the oracle's stencils to"""
    g = np.load(GOLD)
    for k in range(3):
        w, lam, alpha, d_alpha = g[f"psf{k}_args"]
        st = sr.stencil(sr.Geometry(_spikes(w, lam, alpha, d_alpha)))
        got = (st.S / np.sum(st.S)).astype(np.float64)
        np.testing.assert_allclose(got, g[f"psf{k}"], rtol=0, atol=2e-15)


def test_reference_image_matches_the_golden_image():
    """apply_diffraction_psf on the 40 x 44 golden image: box, zeroed core, dense sum (the tolerance of the oracle's golden test)"""
    g = np.load(GOLD)
    lam, rot, exptime, lat, az, alt, thr, cutoff = g["apply_args"]
    d_alpha = dfft.field_rotation_angle(lat, az, alt, exptime)
    S = _spikes(cutoff, lam, math.pi / 4 - rot, d_alpha)
    S.threshold = thr
    S.norm = float(sr.stencil_sum(sr.Geometry(S))[0])
    img = g["apply_in"]
    ny, nx = img.shape
    n = 64
    rows = np.zeros(1, dtype=_abi.FFT_OBJECT_DTYPE)
    rows["nfft"], rows["x0"], rows["y0"] = n, 1, 1
    rows["stamp_xmin"], rows["stamp_xmax"], rows["stamp_ymin"], rows["stamp_ymax"] = 1, nx, 1, ny
    grid = np.zeros((n, n))
    grid[:ny, :nx] = img
    out, _, boxes = sr.apply(S, rows, grid.ravel())
    np.testing.assert_allclose(out.astype(np.float64).reshape(n, n)[:ny, :nx], g["apply_out"], rtol=1e-12, atol=1e-9)
    sat = g["saturated_region"]
    assert tuple(boxes[0]) == (sat[0, 0], sat[0, 1] - 1, sat[1, 0], sat[1, 1] - 1)


@pytest.mark.parametrize("geom", list(sc.GEOMETRIES))
@pytest.mark.parametrize("cutoff", [20, 200])
def test_host_stencil_norm_is_the_long_double_sum(geom, cutoff):
    """diffraction_fft.stencil_norm against the long-double sum of S over the grid.  The host's values carry the stencil bound
    (relative to norm: the reference's bound times norm, the wedge decisions of flagged offsets included; numpy's arctangents
    are well inside what datan is allowed); a sum of n non-negative terms, in whatever order, rounds n - 1 times by at most u of
    the sum: n u of it."""
    S = sc.spikes(geom, cutoff)
    st = sr.stencil(sr.Geometry(S))
    total, n = sr.stencil_sum(sr.Geometry(S))
    bound = np.sum(st.bound) * LD(S.norm) + n * sr.U * total
    err = abs(LD(S.norm) - total)
    print(f"{geom}, cutoff {cutoff}: |norm - sum| / bound = {float(err / bound):.3f} ({n} terms)")
    assert err <= bound


@pytest.mark.parametrize("geom", list(sc.GEOMETRIES))
def test_near_decision_cap(geom):
    """at most FLAG_CAP of a geometry's non-zero offsets are near a decision -- at both cutoffs of the table test and at every
    cutoff a case uses; on the reference alone"""
    for cutoff in sorted({20, 200} | {sc.CUTOFF[s] for s, gs in sc.SHAPES.items() if geom in gs}):
        st = sr.stencil(sr.Geometry(sc.spikes(geom, cutoff)))
        flagged, nonzero = int(np.count_nonzero(st.near)), int(np.count_nonzero(st.S))
        print(f"{geom}, cutoff {cutoff}: {flagged} of {nonzero} non-zero offsets near a decision")
        assert nonzero >= 4 * cutoff + 1 and flagged <= sr.FLAG_CAP * nonzero
    if geom == "axis_exact":
        S = sc.spikes(geom, 20)
        assert S.sin0 == 0.0 and np.count_nonzero(sr.stencil(sr.Geometry(S)).S[20]) == 41      # row a = 0 holds 2 cutoff + 1 entries
    if geom == "axis_dyadic":
        st = sr.stencil(sr.Geometry(sc.spikes(geom, 20)))
        assert st.S[20, 30] > st.alt[20, 30] > 0 and not st.near[20, 30]       # on an axis the wedge decides, exactly, and it matters


def test_near_decision_flags_fire_where_the_docstring_says():
    """the geometries the cases avoid: at rot = pi/4 exactly with d_alpha = 0.04 the three half-axes whose dth is not provably exact
    are flagged (3 cutoff offsets; the +a half-axis is decided exactly), at rot = 0 exactly the diagonals are; a flagged offset's
    bound is widened by the difference of its candidates"""
    c = 20
    st = sr.stencil(sr.Geometry(_spikes(c, 622.2, 0.0, 0.04)))
    assert np.count_nonzero(st.near) == 3 * c and not st.near[c + 1:, c].any() and st.near[:c, c].all()
    assert np.count_nonzero(st.near) > sr.FLAG_CAP * np.count_nonzero(st.S)
    k = (c - 5, c)
    assert st.bound[k] >= abs(st.S[k] - st.alt[k]) / LD(1.0) > 1e-3 * st.S[k]
    st = sr.stencil(sr.Geometry(_spikes(c, 622.2, math.pi / 4, 2.2e-3)))
    assert st.near[np.arange(2 * c + 1), np.arange(2 * c + 1)].sum() >= c and np.count_nonzero(st.near) > sr.FLAG_CAP * np.count_nonzero(st.S)


@pytest.mark.parametrize("shape,geom", sc.CASES, ids=[f"{s}/{g}" for s, g in sc.CASES])
def test_oracle_is_within_the_reference_bounds(shape, geom):
    """orc_fft_spikes on every case: every pixel within the reference's bound, pixels outside the stamp (bound 0) exactly the
    clipped input; the case's box is the planted one.  (The oracle's first visit to sin0 == 0.0 and exptime-free constants.)"""
    c = sc.case(shape, geom)
    want, bound, boxes = reference(shape, geom)
    assert np.array_equal(boxes, c.boxes), (boxes, c.boxes)
    got = oracle(c.S).spikes(c.rows, c.rbuf)
    ratio = sr.worst_ratio(got, want, bound)
    print(f"{c.name}: oracle worst error / bound {ratio:.3g}; largest bound {float(bound.max()):.3g}")
    assert ratio <= 1.0
    assert np.abs(got - np.clip(c.rbuf, 0, None)).max() > 1.0 or not (c.boxes[:, 1] >= c.boxes[:, 0]).any()


def test_oracle_under_rbuf_raw_semantics():
    """the reference fed the raw buffer (rbuf_raw = 1) is the reference fed fl64(raw fl64(1 / n^2)) exactly, and the oracle on
    that image is within its bounds"""
    c = sc.case("batch", "generic")
    raw, image = sc.raw_buffer(c)
    want, bound, boxes = sr.apply(c.S, c.rows, raw, raw=True)
    same = sr.apply(c.S, c.rows, image)
    assert np.array_equal(want, same[0]) and np.array_equal(bound, same[1]) and np.array_equal(boxes, c.boxes)
    assert sr.worst_ratio(oracle(c.S).spikes(c.rows, image), want, bound) <= 1.0


@pytest.mark.parametrize("mutation", list(sr.MUTATIONS))
def test_teeth(mutation):
    """every restated mistake leaves the bounds of the case named in spike_ref.MUTATIONS"""
    shape, geom = sr.MUTATIONS[mutation]
    c = sc.case(shape, geom)
    if mutation == "no_inv_n2":
        raw, _ = sc.raw_buffer(c)
        want, bound, _ = sr.apply(c.S, c.rows, raw, raw=True)
        bad, _, bad_boxes = sr.apply(c.S, c.rows, raw, raw=True, mutate=mutation)
    else:
        want, bound, _ = reference(shape, geom)
        bad, _, bad_boxes = sr.apply(c.S, c.rows, c.rbuf, mutate=mutation)
    ratio = sr.worst_ratio(bad, want, bound)
    print(f"{mutation} on {c.name}: worst error / bound {ratio:.3g}")
    assert ratio > 1.0
    assert np.array_equal(bad_boxes, c.boxes) == (mutation != "box_over_grid")
