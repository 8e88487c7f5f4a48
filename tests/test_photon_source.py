"""The photon source against an independent reference, on the CPU: tests/photon_source_ref.py (plain numpy, np.longdouble)
against the oracle's photon pool on every case of tests/photon_source_cases.py, with the assertion the GPU file uses
(tests/test_photon_source_gpu.py).  This proves the reference and its derived bounds without a GPU, and pins the oracle -- which
shares its structure with the kernels -- to something that shares none of it."""
import numpy as np
import pytest

import photon_source_cases as cases
import photon_source_ref as ref

LD = np.longdouble
CASES = cases.all_cases()
# one oracle run per scene: the renderer's switches (quads, pre-pass) do not exist on the CPU
CPU_CASES = list({(c.name.split("_q")[0] + ("_c1" if "_c1" in c.name else "") + c.name[c.name.find("_fits"):] * ("_fits" in c.name)
                   + c.name[c.name.find("_over"):] * ("_over" in c.name)): c for c in CASES}.values())


def test_philox_known_answers():
    # Random123 kat_vectors, philox4x32 with 10 rounds (the three that tests/test_oracle_math.py holds the oracle to)
    def run(ctr, key):
        return [int(v[0]) for v in ref.philox4x32_10(ctr, key)]
    assert run([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert run([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert run([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_words_address_the_counter_and_key_the_spec_names():
    """counter = (photon lo, photon hi, slot, obj_id lo), key = (seed lo, seed hi ^ obj_id hi), also above 2^32"""
    seed, obj, k, slot = (0xABCDEF01 << 32) | 0x2345, 2 ** 40 + 7, 2 ** 33 + 3, 21
    got = [int(v[0]) for v in ref.words(seed, obj, [k], slot)]
    want = [int(v[0]) for v in ref.philox4x32_10([3, 2, 21, 7], [0x2345, 0xABCDEF01 ^ 0x100])]
    assert got == want
    assert float(ref.w01(np.array([0], dtype=np.uint64))[0]) == 2.0 ** -33


@pytest.mark.parametrize("case", CPU_CASES, ids=[c.name for c in CPU_CASES])
def test_oracle_pool_matches_the_reference(case):
    from oracle import orc_loader
    shot = ref.shoot(case.source(), case.objects)
    pool = orc_loader.OracleScene(case.scene).shoot_photons(case.objects).to_host()
    assert len(pool["x"]) == case.objects["n_phot"].sum() > 0
    assert np.array_equal(pool["obj_index"], np.repeat(np.arange(len(case.objects)), case.objects["n_phot"]))
    ref.assert_matches(shot, pool, case.name)
    if shot.kick is not None:
        # the wraps the case is there for: coordinates several hundred metres either side of zero
        assert case.source().atm.max_fx == 0.0 and shot.kick_bound > 0
        assert np.abs(shot.kick).max() > 0


def test_a_list_of_five_components_is_refused():
    """a launch holds IMS_MAX_PSF = 4 components (components 0 .. 3: two blocks of words); a fifth Gaussian cannot be shot and
    must not be dropped silently"""
    from imsim_amd import _abi
    from imsim_amd.engine import BoundScene, HostMem
    assert _abi.IMS_MAX_PSF == 4
    scene = cases._scene(cases.GAUSS[:5], sed=cases.sed_tables(3))
    with pytest.raises(ValueError, match="too many PSF components"):
        BoundScene(scene, HostMem(), None)


# ---- the table samplers on the toy tables, against a brute-force search and a longdouble interpolation ----
def _u(n=20000, seed=3):
    w = np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64)
    w[:4] = [0, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1]
    return ref.w01(w)


def _brute_bin(cdf, u):
    """largest i <= n - 2 with cdf[i] <= u, one comparison per knot"""
    return np.array([max(i for i in range(len(cdf) - 1) if cdf[i] <= uu) for uu in u.astype(np.float64)])


@pytest.mark.parametrize("n_bins", [1, 2, 7, 4096])
def test_radial_sampler_on_the_toy_tables(n_bins):
    r2s, cdfs = cases.toy_radial(n_bins)
    u = _u(2000 if n_bins == 4096 else 20000)
    if n_bins == 4096:
        u = np.concatenate([u, _u(2000, 5) * 2.0 ** -12])            # deep inside the first guide cell
    for r2, cdf in zip(r2s, cdfs):
        knots = cdf[(cdf > 0) & (cdf < 1)]
        u = np.concatenate([u, np.array(knots, dtype=LD)]) if n_bins <= 7 else u         # the knots themselves
        i = _brute_bin(cdf, u)
        assert np.array_equal(i, ref.table_bin(cdf, u))
        assert np.array_equal(i, np.searchsorted(cdf, u.astype(np.float64), side="right").clip(1, n_bins) - 1)
        wd = (cdf[i + 1] - cdf[i]).astype(LD)
        f = np.where(wd > 0, (u - cdf[i]) / np.where(wd > 0, wd, 1), 0)
        want = r2[i] + f * (r2[i + 1].astype(LD) - r2[i])
        got = ref.radial_r2(r2, cdf, u)
        assert np.all(np.abs(got - want) <= 4 * ref.EPS * np.abs(want))
        assert np.all((got >= r2[i]) & (got <= r2[i + 1]))
        if n_bins == 7:
            # a bin of no width is never drawn from (the search ends past it), and r2 jumps across it
            assert np.any(np.diff(cdf) == 0) and np.all(wd > 0)
            empty = np.flatnonzero(np.diff(cdf) == 0)
            assert not np.isin(i, empty).any() and np.isin(empty[empty + 1 < n_bins] + 1, i).all()


def test_guide_table_brackets_every_deviate_on_the_toy_tables():
    """the invariant the kernel's narrowed bisection rests on (ims_radial_tables_t.guide), on the tables that stress it: fewer
    bins than guide cells, thousands of bins in one guide cell, bins of no width.  With lo = guide[g] and
    hi = min(guide[g + 1] + 1, n_bins), g = floor(512 u): cdf[lo] <= u, and u < cdf[hi] or hi = n_bins; so the brute-force bin
    lies in [lo, hi)."""
    import ctypes as C
    from imsim_amd.engine import BoundScene, HostMem

    class NoDerive:
        def fill_derived_op(self, op):
            pass
    for n_bins in (1, 2, 7, 4096):
        case = cases.toy_case(n_bins)
        bound = BoundScene(case.scene, HostMem(), NoDerive())                  # (owns the tables behind the pointers)
        P = bound.base_params
        nt, ng = P.radial.n_tables, P.radial.n_guide
        assert ng == 512 and P.radial.n_bins == n_bins
        guide = np.ctypeslib.as_array(C.cast(P.radial.guide, C.POINTER(C.c_int32)), (nt, ng + 1))
        u = _u(4000)
        g = np.floor(u * ng).astype(np.int64)
        for t, cdf in enumerate(np.atleast_2d(case.scene.radial_cdf)):
            lo, hi = guide[t][g], np.minimum(guide[t][g + 1] + 1, n_bins)
            i = ref.table_bin(cdf, u)
            assert np.all((lo <= i) & (i < hi))
            assert np.all(cdf[lo] <= u) and np.all((u < cdf[hi]) | (hi == n_bins))
            if n_bins == 4096:
                # and the "+ 1" is needed: without it the bracket loses the bin of some deviates of this table
                assert np.any(i >= np.minimum(guide[t][g + 1], n_bins))


def test_oracle_table_samplers_at_the_knots_and_between():
    """the oracle's own radial and linear samplers, called directly: a deviate of the stream never equals a knot (it is an odd
    multiple of 2^-33), so what happens AT a knot -- cdf[i] <= u, not < -- shows in no photon pool"""
    import ctypes as C
    from imsim_amd import _abi
    from oracle import orc_loader
    lib = orc_loader.load()
    lib.orc_radial_r2.restype = C.c_double
    lib.orc_radial_r2.argtypes = [C.POINTER(_abi.RadialTables), C.c_int, C.c_double]
    lib.orc_lin_lookup.restype = C.c_double
    lib.orc_lin_lookup.argtypes = [C.POINTER(_abi.LinTables), C.c_int, C.c_double]
    for n_bins in (1, 2, 7, 4096):
        r2s, cdfs = (np.ascontiguousarray(a) for a in cases.toy_radial(n_bins))
        T = _abi.RadialTables()
        T.n_tables, T.n_bins, T.r2, T.cdf = len(r2s), n_bins, r2s.ctypes.data, cdfs.ctypes.data
        for t, (r2, cdf) in enumerate(zip(r2s, cdfs)):
            knots = cdf[(cdf > 0) & (cdf < 1)]
            u = np.concatenate([_u(1500), np.array(knots[:: max(1, len(knots) // 600)], dtype=LD)])
            got = np.array([lib.orc_radial_r2(C.byref(T), t, float(v)) for v in u])
            want = ref.radial_r2(r2, cdf, u)
            assert np.all(np.abs(got - want) <= 4 * ref.EPS * np.abs(want))
    for n_pts in (2, 3, 2049):
        v = np.ascontiguousarray(cases.sed_tables(n_pts))
        L = _abi.LinTables()
        L.n_tables, L.n_pts, L.arg_min, L.arg_step, L.val = 2, n_pts, 0.0, 1.0 / (n_pts - 1), v.ctypes.data
        u = np.concatenate([_u(1500), np.linspace(0, 1, n_pts)[1:-1][:600].astype(LD)])
        for t in range(2):
            got = np.array([lib.orc_lin_lookup(C.byref(L), t, float(x)) for x in u])
            want, bound = ref.lin_lookup(v[t], u)
            assert np.all(np.abs(got - want) <= bound)


@pytest.mark.parametrize("n_pts", [2, 3, 2049])
def test_wavelength_table_lookup(n_pts):
    u = _u()
    for v in cases.sed_tables(n_pts):
        got, bound = ref.lin_lookup(v, u)
        x = np.linspace(0.0, 1.0, n_pts)
        i = np.clip(np.searchsorted(x, u.astype(np.float64), side="right") - 1, 0, n_pts - 2)
        f = (u - x[i].astype(LD)) * (n_pts - 1)
        want = v[i] + f * (v[i + 1].astype(LD) - v[i])
        assert np.all(np.abs(got - want) <= bound) and np.all(bound <= 8 * 2.0 ** -52 * 700)
    flat = cases.sed_tables(2049)[1]
    assert np.all(ref.lin_lookup(flat, u[u < 0.18])[0] == 540.0)


@pytest.mark.parametrize("interpolant", ["nearest", "quintic"])
def test_image_samplers(interpolant):
    case = cases.profiles_case(interpolant)
    src = case.source()
    u, u2 = _u(5000, 7), _u(5000, 8)
    for (w, h), cdf, img in zip(src.image_sizes, src.image_cdfs, case.scene.image_profiles):
        gx, gy, pix, f = ref.image_nearest(cdf, w, h, u, u2)
        assert np.array_equal(pix, _brute_bin(cdf, u))
        assert np.all(np.asarray(img).reshape(-1)[pix] > 0)                   # an empty pixel is never drawn
        assert np.all((f >= 0) & (f <= 1))
        assert np.all(np.abs(gx - ((pix % w) + f - LD(w) / 2)) == 0) and np.all(np.abs(gy - ((pix // w) + u2 - LD(h) / 2)) == 0)
    if interpolant == "quintic":
        kx, kcdf, norm, neg = src.interp
        d, negative, slope = ref.interp_offset(kx, kcdf, neg, u)
        i = _brute_bin(kcdf, u)
        assert np.all((d >= kx[i]) & (d <= kx[i + 1])) and np.all(np.abs(d) <= 3)
        # the sign rule of the negative lobes: K < 0 on 1 < |x| < 2 and (25 + sqrt 31) / 11 < |x| < 3
        from imsim_amd.engine import quintic_kernel
        inside = np.abs(np.abs(d)[:, None] - np.array([1.0, 2.0, neg[2], 3.0])[None, :]).min(axis=1) > 1e-6
        assert np.array_equal(negative[inside], quintic_kernel(d.astype(np.float64))[inside] < 0)
        assert negative.any() and (~negative).any()
