"""The means and the mean maps of the Poisson deviate's tests, once, for the CPU and the GPU files."""
import numpy as np

SEED = 11
OBJ_LOW, OBJ_HIGH = 3, 0x7F00000003            # object ids on both sides of 2^32 (the high word goes into the Philox key)
FLAT_ID_BASE = 0x7F00000000                    # object id space of the flat builder's streams (+ iteration)
READOUT_ID_BASE = 0x7E00000000                 # ... of the read-noise streams (+ amplifier)
CATALOG_ID_HIGH = 5 << 32                      # added to catalog object ids in the GPU tests: above 2^32, below the id bases
N_EQUAL, N_LAW = 2 ** 17, 2 ** 20

BELOW_10, ABOVE_10 = float(np.nextafter(10.0, 0.0)), float(np.nextafter(10.0, 20.0))
LAW_MEANS = (1e-3, 0.3, 3.0, 9.5, BELOW_10, 10.0, ABOVE_10, 10.5, 12.0, 47.0, 1e3, 2e6, 1e9)

# edge means; `None` = the value is the reference's draw, a number = the value the spec gives whatever the uniforms are
# (exp(-5e-324) and exp(-1e-300) round to 1, and no product of uniforms in (0, 1] exceeds 1)
EDGE_MEANS = ((0.0, 0.0), (-1.0, 0.0), (float("nan"), 0.0), (5e-324, 0.0), (1e-300, 0.0), (700.0, None), (746.0, None),
              (36.7, None))

# the PTRS constants changed one at a time: name -> (changed entries of noise_deviate_ref.PTRS, what catches it).
# "equality": draws differ from the oracle's beyond the near ties; "law": the changed sampler's own draws miss the pass mark.
# The test asserts each set exactly, so that losing a mechanism shows; why each is what it is:
# * the shift moves k itself and invalpha / Stirling's coefficient move the acceptance: draws differ, but the full test still
#   accepts by the (nearly) right ratio, so the law holds to far below what 2^17 draws resolve;
# * 0.07 -> 0.05 accepts without the full test where the squeeze is no longer inside the density: wrong, but by 1e-3 of the draws;
# * vr -> 0.95 accepts every V up to 0.95 unexamined: the tails are over-filled by per cent, which the law sees;
# * `V from u01` is beyond the reach of any test on draws: u01 and u01_open differ by 2^-53, which moves log V by 2^-53 / V
#   and flips a comparison of a draw with probability about 2^-53 ln 2^53 = 4e-15.
WRONG_CONSTANTS = {
    "0.43 -> 0.5": (dict(shift=0.5), {"equality"}),
    "vr -> 0.95": (dict(vr=0.95), {"equality", "law"}),
    "0.07 -> 0.05": (dict(squeeze=0.05), {"equality"}),
    "invalpha * 1.02": (dict(invalpha_scale=1.02), {"equality"}),
    "Stirling 1/12 -> 1/13": (dict(stirling_c1=1.0 / 13.0), {"equality"}),
    "V from u01": (dict(v_open=False), set()),
}


def ramp(n=N_EQUAL):
    """n means log-spaced from 1e-6 to 1e9"""
    return 10.0 ** np.linspace(-6.0, 9.0, n)


# ---- the mean map of the flat-field test: `base` of a 1000 x 1049 image (1 049 000 pixels = 4097 workgroups of 256 + 168)
FLAT_NX, FLAT_NY, BAND = 1000, 1049, 64
FLAT_LEVEL = 0.9                               # mean = level * base[p], one f64 product, which the reference forms too


def base_for(mean, level=FLAT_LEVEL):
    """a double b with level * b == mean in f64 where one exists among the neighbours of mean / level, else mean / level"""
    b = mean / level
    if not np.isfinite(b) or b == 0.0:
        return b
    cands = [b]
    for _ in range(2):
        cands = [float(np.nextafter(cands[0], -np.inf))] + cands + [float(np.nextafter(cands[-1], np.inf))]
    for c in cands:
        if level * c == mean:
            return c
    return b


def flat_base():
    """[ny][nx] map: a band of 64 rows per law mean, a band with the log ramp, a row with the edge means (cycled), the rest
    the ramp again, reversed.  Returns (base, bands) with bands = {law mean: row slice}; level * base is exactly the mean
    for the three means at the branch point."""
    base = np.empty((FLAT_NY, FLAT_NX))
    bands = {}
    for i, m in enumerate(LAW_MEANS):
        bands[m] = slice(i * BAND, (i + 1) * BAND)
        base[bands[m]] = base_for(m)
    for m in (BELOW_10, 10.0, ABOVE_10):
        assert FLAT_LEVEL * base[bands[m]][0, 0] == m
    r0 = len(LAW_MEANS) * BAND
    base[r0:r0 + BAND] = ramp(BAND * FLAT_NX).reshape(BAND, FLAT_NX) / FLAT_LEVEL
    edge = np.array([base_for(m) for m, _ in EDGE_MEANS])
    base[r0 + BAND] = edge[np.arange(FLAT_NX) % len(edge)]
    rest = FLAT_NY - (r0 + BAND + 1)
    base[r0 + BAND + 1:] = ramp(rest * FLAT_NX)[::-1].reshape(rest, FLAT_NX) / FLAT_LEVEL
    return base, bands
