"""Generate golden vectors for the CCD readout chain from the reference, in THIS container.  Run once; the .npz
is committed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_readout_golden.py

* bleed trails: imsim/bleed_trails.py is numpy-only and is imported as it is.  Inputs are float64 arrays of
  integer electron counts (all sums exact), including the reference's own regression channel
  tests/data/neg_pixel_bleed.pickle (tests/test_bleed_trails.py:66-75).
  The shape cases (section 5: odd ny, channels under eight rows, more than 256 channels, nothing / everything saturated,
  exact full well, negative pixels) come from a generator of their own; the vectors that were there before keep their
  bytes, which the script checks against the committed file before it writes.
* cte_matrix: imsim/readout.py imports galsim / astropy / lsst at module level and cannot be imported; the one
  numpy + scipy function is compiled from its own source text (located with `ast`, nothing is written to the repo).
"""
import ast
import importlib.util
import os
import pickle
import sys
import types

import numpy as np
import scipy.special

REF = "/root/reference"
pkg = types.ModuleType("imsim")
pkg.__path__ = [os.path.join(REF, "imsim")]
sys.modules["imsim"] = pkg
spec = importlib.util.spec_from_file_location("imsim.bleed_trails", os.path.join(REF, "imsim", "bleed_trails.py"))
bleed = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bleed)

src = open(os.path.join(REF, "imsim", "readout.py")).read()
node = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "cte_matrix")
ns = {"np": np, "scipy": scipy}
exec(compile(ast.Module(body=[node], type_ignores=[]), "readout.py:cte_matrix", "exec"), ns)
cte_matrix = ns["cte_matrix"]

out = {}
rng = np.random.default_rng(20261002)
full_well = 100000.0

# 1. one channel with a saturated star in the middle (tests/test_bleed_trails.py:41-64)
ch = np.full(2000, 800.0)
ch[980:1020] = 2 * full_well
out["chan_in"], out["chan_out"] = ch, bleed.bleed_channel(ch, full_well)

# 2. an image with several kinds of runs: near the bottom edge (charge leaves), near the top edge (closed),
#    two runs close enough to merge, a run across the midline, isolated hot pixels
img = rng.poisson(800.0, size=(96, 40)).astype(np.float64)
img[2:6, 3] += 5 * full_well            # bleeds off the bottom
img[90:95, 7] += 3 * full_well          # reaches the closed top
img[30:34, 11] += 4 * full_well         # two runs that meet
img[40:43, 11] += 6 * full_well
img[44:52, 15] += 2.5 * full_well       # straddles the midline (48)
img[60, 20] += 1.2 * full_well          # single hot pixel
img[10:80, 25] += 1.5 * full_well       # long run: more charge than the column can hold below the top
img[0:96, 30] += 2 * full_well          # a fully saturated column
img[47:49, 33] += 30 * full_well
out["img_in"] = img
out["img_midline"] = bleed.bleed_eimage(img.copy(), full_well, midline_stop=True)
out["img_nomidline"] = bleed.bleed_eimage(img.copy(), full_well, midline_stop=False)
out["full_well"] = np.array(full_well)

# 3. the reference's regression channel (a data file of its test suite)
with open(os.path.join(REF, "tests", "data", "neg_pixel_bleed.pickle"), "rb") as fobj:
    channel_data, fw = pickle.load(fobj)
cd = np.asarray(channel_data, dtype=np.float64)
out["neg_in"], out["neg_fw"] = cd, np.array(float(fw))
out["neg_out"] = bleed.bleed_channel(cd, float(fw))
out["neg_out_native"] = np.asarray(bleed.bleed_channel(np.asarray(channel_data), fw), dtype=np.float64)

# 4. CTE matrices
out["cte_64_1e-6"] = cte_matrix(64, 1.0e-6)
out["cte_64_1e-3"] = cte_matrix(64, 1.0e-3)
out["cte_40_1e-2_nt5"] = cte_matrix(40, 1.0e-2, ntransfers=5)

# 5. bleed trails at the shapes and values where an implementation can go wrong (a generator of their own: the vectors above
#    keep their values).  Every case `<name>_in` is bled with and without the midline stop.
rng2 = np.random.default_rng(20261017)
fw = full_well
cases = {}

# odd ny: ymid = 48, the halves have 48 and 49 rows
img = rng2.poisson(800.0, size=(97, 40)).astype(np.float64)
img[44:48, 2] += 3 * fw                 # ends at row 47, the last row of the lower half
img[48:52, 5] += 3 * fw                 # starts at row 48, the first row of the upper half
img[46:51, 8] += 4 * fw                 # straddles the midline
img[0, 11] += 2.5 * fw                  # first row
img[96, 14] += 2.5 * fw                 # last row
img[0, 17] += 2 * fw                    # first and last row of one column
img[96, 17] += 2 * fw
img[47, 20] += 6 * fw                   # one pixel on either side of the midline, different columns and the same column
img[48, 23] += 6 * fw
img[47:49, 26] += 40 * fw               # more charge than the upper half can hold
img[90:96, 29] += 9 * fw                # reaches the closed top, spills downwards
cases["odd"] = img

# channels shorter than eight rows
img = rng2.poisson(800.0, size=(5, 9)).astype(np.float64)
img[0, 0] += 2 * fw
img[4, 1] += 2 * fw
img[1:3, 2] += 1.5 * fw                 # across ymid = 2
img[2, 4] += 3.5 * fw
img[0:5, 6] += 1.25 * fw
img[1, 8] += 0.5 * fw                   # bright, not saturated
img[3, 8] += 7 * fw
cases["short"] = img

# wide and flat: with the midline stop column x of half h is channel h nx + x, and a boundary between two groups of 256
# channels falls inside the image
for ny, nx in ((7, 257), (6, 513)):
    img = np.full((ny, nx), 1000.0)
    ymid = ny // 2
    for k, x in enumerate((0, 255, 256, nx - 1)):
        img[ymid - 1 - (k % 2), x] += (2 + k) * fw           # lower half
        img[ymid + (k % 3), x] += (1.5 + k) * fw             # upper half
    img[ymid - 1:ymid + 1, 128] += 3 * fw                    # across the midline, away from the boundaries
    cases[f"wide{nx}"] = img

cases["unsat"] = np.minimum(rng2.poisson(50000.0, size=(11, 6)).astype(np.float64), fw)
cases["unsat"][5, 3] = fw               # exactly full well is not saturated
cases["allsat"] = fw + 1.0 + rng2.poisson(3000.0, size=(9, 6)).astype(np.float64)

# a pixel exactly at full well next to one just above it; a negative pixel beside a run
img = rng2.poisson(800.0, size=(12, 6)).astype(np.float64)
img[5, 0], img[6, 0] = fw, fw + 1.0
img[3, 1], img[4, 1] = fw + 1.0, fw
img[4, 2] = -50.0
img[5:7, 2] += 3 * fw
img[8, 3] = -7.0
img[9, 3] += 1.5 * fw
img[2:4, 4] = fw                        # a run of pixels exactly at full well: nothing happens
img[7, 5] = fw + 1.0                    # one electron to give away
cases["edge"] = img

for name, img in cases.items():
    assert (img == np.round(img)).all(), name
    out[f"{name}_in"] = img
    out[f"{name}_midline"] = bleed.bleed_eimage(img.copy(), fw, midline_stop=True)
    out[f"{name}_nomidline"] = bleed.bleed_eimage(img.copy(), fw, midline_stop=False)

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "readout_golden.npz")
if os.path.exists(path):
    # the vectors already committed stay what they are, bit for bit
    with np.load(path) as old:
        for key in old.files:
            a, b = np.ascontiguousarray(old[key]), np.ascontiguousarray(out[key])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
        print("unchanged:", sorted(old.files))
np.savez_compressed(path, **out)
print("wrote", path, {k: v.shape for k, v in out.items()})
print("neg channel dtype", np.asarray(channel_data).dtype, "fw", fw, "native == float64 path:",
      np.array_equal(out["neg_out"], out["neg_out_native"]))
