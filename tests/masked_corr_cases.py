"""Seeded cases of the masked correlation tests: a smoothed random field with noise, cut twice at a known offset so that
``moving(x + offset) ~ fixed(x)``, with diagonal wedges of invalid voxels in both crops and a bright block in the invalid part of
the moving crop.  How a voxel is made invalid differs per case: NaN wedges (but for the block, which a uint8 mask takes out), explicit uint8 masks
over finite data, or a dark background under ``valid_above``."""
import numpy as np
from scipy import ndimage

PAD = 16
BRIGHT = 5000.0
DARK_THRESHOLD = 50.0

# name: shape, planted offset, max_shift, how voxels are invalid, wedge steepness / cut of the fixed crop
CASES = {
    "nan_13x20": dict(shape=(13, 20), offset=(3, -5), max_shift=None, kind="nan"),
    "nan_6x9x11": dict(shape=(6, 9, 11), offset=(-1, 2, -3), max_shift=None, kind="nan"),
    "above_24x40_shift_5_7": dict(shape=(24, 40), offset=(-4, 6), max_shift=(5, 7), kind="above"),
    "nan_1x17": dict(shape=(1, 17), offset=(0, -4), max_shift=None, kind="nan", min_overlap=4),      # (4 ** ndim = 16 of 17 voxels)
    "mask_8x16x16": dict(shape=(8, 16, 16), offset=(2, -3, 4), max_shift=None, kind="mask"),
    # the planted shift lies on the edge of the window along x; the wedge leaves two voxels of the first row of the fixed crop, so
    # that this window too holds overlaps of two voxels (seed 2: with seed 1 those two are nearly equal and their variance falls
    # under the tolerance, r = 0)
    "nan_5x31_edge": dict(shape=(5, 31), offset=(1, -9), max_shift=(4, 9), kind="nan", fixed_cut=0.93, fixed_slope=4.0, seed=2),
}
# max |r(float32 restatement) - r(float64 brute force)| over the eligible shifts, per case, as measured with numpy 2.2 (pocketfft in
# single precision; tests/test_masked_corr_host.py measures it again and allows another pocketfft build a factor of 2).
MEASURED_R_ERROR = {
    "nan_13x20": 1.22e-06,
    "nan_6x9x11": 2.10e-06,
    "above_24x40_shift_5_7": 3.80e-07,
    "nan_1x17": 6.05e-07,
    "mask_8x16x16": 2.17e-06,
    "nan_5x31_edge": 1.51e-06,
}
R_ERROR = 2.2e-06                      # the largest of them, rounded up
# What the GPU's r may differ by from the brute force on eligible shifts: 8 x the restatement's error, because the GPU transform sums
# in another order than pocketfft (Stockham passes per axis, other twiddle tables).
GPU_R_TOLERANCE = 8 * R_ERROR          # 1.76e-05
WEDGE_CASES = [k for k, c in CASES.items() if c["kind"] in ("nan", "mask")]


def wedges(shape, fixed_cut=0.35, fixed_slope=1.0, moving_cut=0.6):
    """Validity of the two crops: a corner of the last two axes cut off diagonally in each (another corner in each)."""
    ii = np.indices(shape).astype(np.float64)
    u, v = ii[-1] / shape[-1], ii[-2] / shape[-2]
    return (u + fixed_slope * v) > fixed_cut, (u - v) < moving_cut


def make_case(name):
    """Returns a dict: ``F``, ``M`` (float32), ``kwargs`` (fixed_mask, moving_mask, valid_above as the oracle and the public function
    take them), ``max_shift``, ``offset``, ``vF``, ``vM`` (the validity the case intends)."""
    c = CASES[name]
    shape, offset = c["shape"], c["offset"]
    rng = np.random.default_rng(c.get("seed", 1))
    G = ndimage.gaussian_filter(rng.random([s + 2 * PAD for s in shape]), 1.5) * 1000.0 + 100.0
    F = G[tuple(slice(PAD, PAD + s) for s in shape)].astype(np.float32)
    M = G[tuple(slice(PAD - k, PAD - k + s) for s, k in zip(shape, offset))].astype(np.float32)      # M(x) = G(x - offset)
    F = F + rng.normal(0, 20, shape).astype(np.float32)
    M = M + rng.normal(0, 20, shape).astype(np.float32)
    vF, vM = wedges(shape, c.get("fixed_cut", 0.35), c.get("fixed_slope", 1.0))
    kwargs = {"min_overlap": c["min_overlap"]} if "min_overlap" in c else {}
    ii = np.indices(shape).astype(np.float64)
    u, v = ii[-1] / shape[-1], ii[-2] / shape[-2]
    block = ~vM & (u > 0.8)          # the bright block: finite voxels in the moving crop's wedge
    if c["kind"] == "nan":
        # NaN wedges in both crops, but for the block, which a mask takes out
        F[~vF] = np.nan
        M[~vM] = np.nan
        M[block] = BRIGHT
        kwargs["moving_mask"] = (~block).astype(np.uint8)
    elif c["kind"] == "mask":
        F[~vF] = 0.0
        M[~vM] = BRIGHT
        kwargs["fixed_mask"] = vF.astype(np.uint8)
        kwargs["moving_mask"] = vM.astype(np.uint8)
    else:
        # a dark, structured background where the sample is not (another corner of each crop), the NaN wedges and the block besides
        dark_f, dark_m = (u + v) > 1.55, (v - u) > 0.6
        F[dark_f] = (10.0 + 20.0 * u[dark_f]).astype(np.float32)
        M[dark_m] = (10.0 + 20.0 * v[dark_m]).astype(np.float32)
        F[~vF] = np.nan
        M[~vM] = np.nan
        M[block] = BRIGHT
        kwargs["moving_mask"] = (~block).astype(np.uint8)
        vF, vM = vF & ~dark_f, vM & ~dark_m
        kwargs["valid_above"] = (DARK_THRESHOLD, DARK_THRESHOLD)
    return {"name": name, "F": np.ascontiguousarray(F), "M": np.ascontiguousarray(M), "kwargs": kwargs, "max_shift": c["max_shift"],
            "offset": list(offset), "vF": vF, "vM": vM}


_cache = {}


def case_with_oracle(name):
    """The case, the brute-force result and the float32 restatement, computed once and shared (treat them as read-only)."""
    if name not in _cache:
        from tests.masked_corr_oracle import brute_force, float32_chain

        case = make_case(name)
        kw = dict(case["kwargs"])
        kw.setdefault("valid_above", (None, None))
        _cache[name] = (case, brute_force(case["F"], case["M"], max_shift=case["max_shift"], **kw),
                        float32_chain(case["F"], case["M"], max_shift=case["max_shift"], **kw))
    return _cache[name]
