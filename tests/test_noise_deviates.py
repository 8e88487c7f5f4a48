"""The Poisson deviate, its log Gamma and the read-noise Gaussian on the CPU: the oracle against tests/noise_deviate_ref.py
(plain numpy, np.longdouble, mpmath's log Gamma) draw for draw, against the exact Poisson law, and the proof that these
tests fail when a constant of the algorithm is wrong.  The GPU half is tests/test_noise_deviates_gpu.py."""
import numpy as np
import pytest
from scipy import stats

import noise_deviate_cases as K
import noise_deviate_ref as R
from oracle import orc_loader

EQUAL_CASES = [(m, obj) for m in K.LAW_MEANS + ("ramp",) for obj in (K.OBJ_LOW, K.OBJ_HIGH)]
_cache = {}


def _means(m, n):
    return K.ramp(n) if isinstance(m, str) else np.full(n, m)


def _ref(m, obj):
    """the reference's draws of a case, computed once"""
    if (m, obj) not in _cache:
        _cache[(m, obj)] = R.poisson_ref(_means(m, K.N_EQUAL), K.SEED, obj, np.arange(K.N_EQUAL))
    return _cache[(m, obj)]


def _law_draws(m):
    if ("law", m) not in _cache:
        _cache[("law", m)] = orc_loader.poisson_probe(np.full(K.N_LAW, m), K.SEED, K.OBJ_HIGH)
    return _cache[("law", m)]


@pytest.mark.parametrize("mean,obj", EQUAL_CASES, ids=lambda v: f"{v:g}" if isinstance(v, float) else str(v))
def test_oracle_equals_the_restatement(mean, obj):
    got = orc_loader.poisson_probe(_means(mean, K.N_EQUAL), K.SEED, obj)
    assert np.all(got >= 0) and np.all(got == np.floor(got))
    share = R.assert_equal_apart_from_ties(got, None, K.SEED, obj, None, f"mean {mean}, object {obj:#x}", ref=_ref(mean, obj))
    print(f"near-tie share, mean {mean}, object {obj:#x}: {share:.3g}")


def test_edge_means():
    """means that are not above zero give 0, NaN included; so do the smallest ones (exp(-mean) rounds to 1 and no product of
    uniforms in (0, 1] exceeds it); 700, 746 and 36.7 are PTRS draws -- no exp(-mean), but log and lgamma at k near the mean"""
    for mean, want in K.EDGE_MEANS:
        for obj in (K.OBJ_LOW, K.OBJ_HIGH):
            got = orc_loader.poisson_probe(np.full(4096, mean), K.SEED, obj)
            ref = R.poisson_ref(np.full(4096, mean), K.SEED, obj, np.arange(4096))
            R.assert_equal_apart_from_ties(got, None, K.SEED, obj, None, f"edge mean {mean}", ref=ref)
            if want is not None:
                assert np.all(got == want) and not ref[1].any()
            else:
                assert abs(got.mean() - mean) < 6 * np.sqrt(mean / 4096)
    assert np.all(orc_loader.poisson_probe(np.zeros(10)) == 0)


@pytest.mark.parametrize("mean", K.LAW_MEANS, ids=lambda v: f"{v:g}")
def test_oracle_follows_the_poisson_law(mean):
    k = _law_draws(mean)
    p = R.law_pvalue(k, mean)
    print(f"law p-value at mean {mean}: {p:.3g}")
    assert p >= R.P_PASS
    sigma, n = np.sqrt(mean), len(k)
    up = np.ceil(mean + 4 * sigma)
    lo, hi = R.tail_interval(float(stats.poisson.sf(up - 1, mean)), n)
    assert lo <= int((k >= up).sum()) <= hi
    down = np.floor(mean - 4 * sigma)
    lo, hi = R.tail_interval(float(stats.poisson.cdf(down, mean)) if down >= 0 else 0.0, n)
    assert lo <= int((k <= down).sum()) <= hi


@pytest.mark.parametrize("mean", (3.0, 47.0, 1e9))
def test_neighbouring_pixels_and_streams_are_uncorrelated(mean):
    n = K.N_LAW
    a = _law_draws(mean)
    lim = 5.0 / np.sqrt(n)
    assert abs(np.corrcoef(a[:-1], a[1:])[0, 1]) < lim
    b = orc_loader.poisson_probe(np.full(n, mean), K.SEED, K.OBJ_HIGH + 1)
    assert abs(np.corrcoef(a, b)[0, 1]) < lim


@pytest.mark.parametrize("name", list(K.WRONG_CONSTANTS))
def test_a_wrong_constant_is_caught(name):
    """The restatement with ONE constant changed, against the oracle: caught = the equality breaks on 2^17 draws of a law
    mean of the PTRS branch ("equality"), or the changed sampler's own 2^17 draws miss the law's pass mark at one ("law").
    Which of the two catches a constant is asserted per constant (noise_deviate_cases.WRONG_CONSTANTS).  `V from u01` escapes
    both, as it must; that is asserted too, so that nobody takes it for covered."""
    changed, caught = K.WRONG_CONSTANTS[name]
    broken, worst_p = 0, 1.0
    for mean in (10.0, 12.0, 47.0, 1e3):
        want, tie = R.poisson_ref(np.full(K.N_EQUAL, mean), K.SEED, K.OBJ_HIGH, np.arange(K.N_EQUAL), constants=changed)
        got = orc_loader.poisson_probe(np.full(K.N_EQUAL, mean), K.SEED, K.OBJ_HIGH)
        assert tie.mean() <= R.EDGE_SHARE_CAP
        broken += int(((got != want) & ~tie).sum())
        worst_p = min(worst_p, R.law_pvalue(want, mean))
    print(f"{name}: {broken} draws of 4 x 2^17 differ, smallest law p-value of the changed sampler on 2^17 draws {worst_p:.3g}")
    assert {m for m, hit in (("equality", broken > 0), ("law", worst_p < R.P_PASS)) if hit} == caught


def _lgamma_points():
    eight = [np.nextafter(8.0, 0.0), 8.0, np.nextafter(8.0, 9.0), np.nextafter(7.0, 0.0), 7.0, np.nextafter(7.0, 8.0)]
    return np.concatenate([10 ** np.linspace(0.0, 10.0, 100000), np.arange(1.0, 65.0), eight])


def lgamma_worst_ratio(values):
    """worst |values - log Gamma| / lgamma_bound over the points of the probe test"""
    x = _lgamma_points()
    if "lgamma" not in _cache:
        exact = R.lgamma_exact(x)
        _cache["lgamma"] = (exact, R.lgamma_bound(x, exact))
    exact, bound = _cache["lgamma"]
    return float((np.abs(np.asarray(values).astype(R.LD) - exact) / bound).max())


def test_lgamma_probe_against_mpmath():
    ratio = lgamma_worst_ratio(orc_loader.math_probe(13, _lgamma_points()))
    print(f"lgamma: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_read_noise_gaussian_follows_the_normal_law():
    g = orc_loader.gauss_probe(seed=K.SEED, obj=K.READOUT_ID_BASE + 3, n=K.N_LAW // 2, slot=0)
    p = R.normal_pvalue(g)
    print(f"read noise: p-value of 2^20 deviates over 64 equiprobable bins {p:.3g}")
    assert p >= R.P_PASS


def test_stream_id_spaces_are_disjoint():
    """A Poisson / Gaussian stream is addressed by (seed, object id, pixel).  The invariants: flat iteration i,
    sky noise NOISE_STREAM + stream_id and the dark current DARK_STREAM are iteration ids added to FLAT_ID_BASE: flat
    iterations stay below NOISE_STREAM, add_noise takes every stream_id >= 0 but the ONE that lands on DARK_STREAM (ids above
    it included: only equality collides); the read noise lives at READOUT_ID_BASE + amplifier, below FLAT_ID_BASE; catalog
    object ids must stay below READOUT_ID_BASE; realised fluxes are drawn at a pixel no image has."""
    from imsim_amd import _abi, lsst_image, readout
    import readout_ref
    assert readout_ref.READOUT_ID_BASE == K.READOUT_ID_BASE
    noise, dark = lsst_image.NOISE_STREAM, readout.DARK_STREAM
    # a flat that reached NOISE_STREAM iterations would need 2^20 launches per CCD; sky ids start there
    assert noise == 1 << 20 and dark > noise
    collide = [sid for sid in range(0, 4096) if noise + sid == dark]
    assert collide == [7]                                         # the id test_add_noise_refuses_the_dark_current_stream covers
    # iteration ids of 31 bits added to the flat base never carry into the key's high word of another space, and the sixteen
    # amplifiers fit under the flat base
    assert dark < 2 ** 31 and (K.FLAT_ID_BASE & 0xFFFFFFFF) == 0 and (K.READOUT_ID_BASE & 0xFFFFFFFF) == 0
    assert K.READOUT_ID_BASE + _abi.IMS_MAX_AMPS <= K.FLAT_ID_BASE
    assert K.FLAT_ID_BASE + 2 ** 32 < 2 ** 63
    # the catalog ids these tests use above 2^32 respect the rule they document
    assert 2 ** 32 < K.CATALOG_ID_HIGH < K.READOUT_ID_BASE
    assert _abi.IMS_FLUX_PIXEL < 0                                # no image has a negative pixel index


def test_add_noise_refuses_the_dark_current_stream():
    from imsim_amd import lsst_image, readout
    assert lsst_image.NOISE_STREAM + 7 == readout.DARK_STREAM
    with pytest.raises(ValueError, match="dark-current"):
        lsst_image.LSST_ImageBuilderBase().add_noise(None, 100.0, stream_id=7)
