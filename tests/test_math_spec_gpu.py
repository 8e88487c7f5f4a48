"""The device's elementary functions and Philox block (csrc/ims_math.h, through ims_test_math) against the oracle, bit for bit,
on the inputs of tests/math_spec_cases.py: bulk, every branch point with its neighbours, and the out-of-domain points.  The
oracle in turn is held to derived error bounds by tests/test_math_spec.py (CPU)."""
import numpy as np
import pytest

import math_spec_cases as mc
from helpers import assert_bits_equal
from test_parity_gpu import _dev_math

pytestmark = pytest.mark.gpu

# probe number of ims_test_math, in-domain and out-of-domain inputs
FUNCTIONS = {
    "exp": (1, mc.exp_in, mc.exp_out),
    "sincos2pi": (2, mc.sincos2pi_in, mc.sincos2pi_out),
    "atan": (3, mc.atan_in, mc.atan_out),
    "sincos": (4, mc.sincos_in, mc.sincos_out),
    "tanh": (5, mc.tanh_in, mc.tanh_out),
    "atan2": (14, mc.atan2_in, mc.atan2_out),
    "pow": (15, mc.pow_in, mc.pow_out),
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def both(torch_cuda):
    """name -> (inputs, device result, oracle result): one launch per function, shared by the tests below"""
    from oracle import orc_loader
    out = {}
    for name, (which, inside, outside) in FUNCTIONS.items():
        x = np.concatenate([inside(), outside()])
        out[name] = (x, _dev_math(torch_cuda, which, x), orc_loader.math_probe(which, x))
    return out


@pytest.mark.parametrize("name", list(FUNCTIONS))
def test_device_equals_oracle_on_the_spec_cases(both, name):
    """Every result that is a number has the same bits on both sides -- in domain and out of it: signed zeros, the flush and
    the cap of exp, saturated quadrants, infinities -- and a NaN on one side is a NaN on the other."""
    x, dev, orc = both[name]
    assert dev.shape == orc.shape
    nan = np.isnan(orc)
    assert np.array_equal(np.isnan(dev), nan), f"{name}: a NaN on one side only"
    assert_bits_equal(dev[~nan], orc[~nan], name)
    assert nan.sum() <= 10                                  # the handful of out-of-domain points, never the bulk


def test_nan_results_carry_the_same_bits(both):
    """The sign and payload of a NaN result, the last part of `device == oracle on every input` (inputs: +-inf, NaN with either
    sign).  exp, pow, sincos2pi and sincos hand a NaN on the same way on gfx950 and x86.  atan and tanh divide by a function of
    their argument with the lean ddiv, whose residual steps negate the denominator (fma(-b, y, 1)): a NaN leaves them with its
    sign bit inverted (first seen here: atan(NaN) 0xfff8.., tanh(-inf) 0x7ff8.. from exp(+inf) = 0xfff8.., atan2(NaN, 1) 0xfff8..
    against the opposite sign from a plain division).  orc_atan and orc_tanh_pos state that (orc_nan_through_ddiv); atan2 follows
    from atan of the quotient, which is a full IEEE division on both sides."""
    bad = []
    for name, (x, dev, orc) in both.items():
        nan = np.isnan(orc) & np.isnan(dev)
        diff = np.flatnonzero(nan & (dev.view(np.uint64) != orc.view(np.uint64)))
        print(f"{name}: {int(nan.sum())} NaN results, {diff.size} with other bits")
        bad += [(name, int(i), hex(int(dev.view(np.uint64)[i])), hex(int(orc.view(np.uint64)[i]))) for i in diff]
    assert not bad, bad


def test_division_and_roots_at_the_ends_of_their_range(torch_cuda):
    """ddiv, dsqrt_n and dsqrt0 are correctly rounded at the ends of their stated 2^+-500 operand range (the bulk is in
    test_parity_gpu.py::test_lean_div_sqrt)"""
    x = mc.sqrt_ends()
    assert_bits_equal(_dev_math(torch_cuda, 7, x), np.sqrt(x), "dsqrt_n")
    assert_bits_equal(_dev_math(torch_cuda, 9, x), np.sqrt(x), "dsqrt0")
    p = mc.div_ends()
    assert_bits_equal(_dev_math(torch_cuda, 8, p), p[:, 0] / p[:, 1], "ddiv")


def _words(torch, quads, seed, obj):
    return _dev_math(torch, 16, np.asarray(quads, dtype=np.float64), seed=seed, obj=obj).astype(np.uint64)


def test_device_philox_known_answers(torch_cuda):
    """The device's rng_block against the Random123 known-answer vectors of philox4x32 with 10 rounds, through the documented
    mapping counter = (photon lo, photon hi, slot, object lo), key = (seed lo, seed hi ^ object hi)."""
    t = torch_cuda
    assert list(_words(t, [0, 0, 0, 0], 0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ff = 0xffffffff
    assert list(_words(t, [ff, ff, ff, ff], 0xffffffffffffffff, 0)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    # the same key from an object id with high bits: seed hi ^ object hi = 0xffffffff
    assert list(_words(t, [ff, ff, ff, ff], 0x0f0f0f0fffffffff, -0x0f0f0f1000000000)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    # digits of pi: photon 0x85a308d3243f6a88, slot 0x13198a2e, object 0x03707344, seed 0x299f31d0a4093822
    assert list(_words(t, [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], 0x299f31d0a4093822, 0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_device_philox_equals_oracle_on_random_counters(torch_cuda):
    """1e4 random (counter, key) pairs, photon indices above 2^32 and object ids with high bits among them: the device block equals
    the oracle's through the same probe, and the oracle's raw orc_test_philox fed with the counter and key the mapping implies."""
    import ctypes as C
    from oracle import orc_loader
    lib = orc_loader.load()
    rng = np.random.default_rng(16)
    n = 2500
    k = 0
    for seed, obj in ((0x0123456789abcdef, 0x7d00000000), (0xfedcba9876543210, -(1 << 40)), (1, 0), (0xffffffff00000000, 0x12345678 << 32)):
        q = rng.integers(0, 2 ** 32, (n, 4)).astype(np.float64)
        q[: n // 2, 1] = rng.integers(0, 4, n // 2)                      # photon indices of realistic size, just above 2^32
        q[: n // 4, 1] = 0
        q[:, 2] = np.where(rng.integers(0, 2, n) == 1, q[:, 2], rng.integers(0, 40, n))
        dev = _words(torch_cuda, q, seed, obj).reshape(n, 4)
        orc = orc_loader.math_probe(16, q, seed=seed, obj=obj).astype(np.uint64).reshape(n, 4)
        assert np.array_equal(dev, orc)
        k0, k1 = seed & 0xffffffff, (seed >> 32) ^ ((obj >> 32) & 0xffffffff)
        for i in range(0, n, 25):                                        # the mapping itself, against the bare generator
            c = (C.c_uint32 * 4)(*[int(v) for v in q[i]])
            lib.orc_test_philox(c, C.c_uint32(k0), C.c_uint32(k1))
            assert [int(v) for v in c] == [int(v) for v in dev[i]]
            k += 1
    assert k == 400
