"""Seeded cases of the masked correlation tests: a smoothed random field with noise, cut twice at a known offset so that
``moving(x + offset) ~ fixed(x)``, with diagonal wedges of invalid voxels in both crops and a bright block in the invalid part of
the moving crop.  How a voxel is made invalid differs per case: NaN wedges (but for the block, which a uint8 mask takes out), explicit uint8 masks
over finite data, or a dark background under ``valid_above``."""
import numpy as np
from scipy import ndimage

PAD = 16                               # margin of the field around the fixed crop: at least this, and at least max |offset| of the case
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

# The smallest shapes at which the chain leaves the paths of the cases above (every kernel is a grid-stride launch of 256 threads and
# at most 1024 workgroups: 262144 items per trip of its loop; a fold of more than 256 partials takes a second trip too).
#   nan_520x520_shift_300: 270400 voxels and a window of 601 x 601 = 361201 entries (a second trip of the statistics and of both
#     window kernels, 1024 partials in every fold), padded 1024 x 1024 = 2^20 (four trips of pack and combine, the LDS Stockham
#     transform on both axes), the peak at window index 450 * 601 + 289 = 270739: a thread finds it in its second trip.
#   nan_20x130x130_shift_3_40_40: 3D, 338000 voxels, padded 32 x 256 x 256 = 2^21 (eight trips), a 256-point axis next to a 32-point one.
#   nan_3x4100_shift_1_10: padded 4 x 8192: the four-step transform, at 2^15 padded voxels.
# The brute force cannot run these windows: their oracle is masked_corr_oracle.fft_float64.
LARGE_CASES = {
    "nan_520x520_shift_300": dict(shape=(520, 520), offset=(150, -11), max_shift=(300, 300), kind="nan"),
    "nan_20x130x130_shift_3_40_40": dict(shape=(20, 130, 130), offset=(2, -5, 9), max_shift=(3, 40, 40), kind="nan"),
    "nan_3x4100_shift_1_10": dict(shape=(3, 4100), offset=(1, -7), max_shift=(1, 10), kind="nan"),
}
ITEMS_PER_TRIP = 1024 * 256            # of a grid-stride loop at the grid cap (mvs_masked_corr_plan.h: kMaxBlocks x kThreads)
# max |r(float32 restatement) - r(fft_float64)| over the eligible shifts, per large case, measured with numpy 2.2 as above
# (tests/test_masked_corr_host.py measures it again and allows a factor of 2).  The GPU is allowed 8 x the figure of its case, for
# the reason given with GPU_R_TOLERANCE.
MEASURED_R_ERROR_LARGE = {
    "nan_520x520_shift_300": 6.73e-06,
    "nan_20x130x130_shift_3_40_40": 2.88e-06,
    "nan_3x4100_shift_1_10": 1.22e-06,
}
GPU_R_TOLERANCE_LARGE = {k: 8 * v for k, v in MEASURED_R_ERROR_LARGE.items()}


def wedges(shape, fixed_cut=0.35, fixed_slope=1.0, moving_cut=0.6):
    """Validity of the two crops: a corner of the last two axes cut off diagonally in each (another corner in each)."""
    ii = np.indices(shape).astype(np.float64)
    u, v = ii[-1] / shape[-1], ii[-2] / shape[-2]
    return (u + fixed_slope * v) > fixed_cut, (u - v) < moving_cut


def make_case(name):
    """Returns a dict: ``F``, ``M`` (float32), ``kwargs`` (fixed_mask, moving_mask, valid_above as the oracle and the public function
    take them), ``max_shift``, ``offset``, ``vF``, ``vM`` (the validity the case intends)."""
    c = CASES[name] if name in CASES else LARGE_CASES[name]
    shape, offset = c["shape"], c["offset"]
    pad = max(PAD, max(abs(k) for k in offset))
    rng = np.random.default_rng(c.get("seed", 1))
    G = ndimage.gaussian_filter(rng.random([s + 2 * pad for s in shape]), 1.5) * 1000.0 + 100.0
    F = G[tuple(slice(pad, pad + s) for s in shape)].astype(np.float32)
    M = G[tuple(slice(pad - k, pad - k + s) for s, k in zip(shape, offset))].astype(np.float32)      # M(x) = G(x - offset)
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


# ---- value edges: small crops, compared with the brute force ----------------------------------------------------------------------
def _variant(case, name, **changed):
    out = dict(case, name=name)
    out.update(changed)
    return out


def infinity_case():
    """nan_13x20 with six seeded valid voxels of each crop set to +inf or -inf: they are not valid (and ``vF``, ``vM`` say so)."""
    case = make_case("nan_13x20")
    rng = np.random.default_rng(7)
    changed = {}
    for im, v in (("F", "vF"), ("M", "vM")):
        pick = rng.choice(np.flatnonzero(case[v]), 6, replace=False)
        data, valid = case[im].copy(), case[v].copy()
        data.ravel()[pick] = np.array([np.inf, -np.inf, np.inf, np.inf, -np.inf, -np.inf], np.float32)
        valid.ravel()[pick] = False
        changed[im], changed[v] = data, valid
    return _variant(case, "nan_13x20_inf", **changed)


CAMERA_OFFSET = 30000.0
# max |r(float32 restatement) - r(float64 brute force)| over the eligible shifts of camera_offset_case(), measured as MEASURED_R_ERROR
# (the GPU is allowed 8 x this), and the same of the restatement that does not centre: the data is there to tell the two apart.
MEASURED_R_ERROR_CAMERA = 1.96e-06
MEASURED_R_ERROR_CAMERA_UNCENTRED = 0.89


def camera_offset_case():
    """The field of nan_13x20 as a 16-bit camera gives it: whole numbers of an amplitude of about 50 around CAMERA_OFFSET (float32
    holds them exactly), the bright block saturated.  Returns the case and the same crops without the offset (``plain_F``,
    ``plain_M`` in the dict), whose r in float64 is the same."""
    case = make_case("nan_13x20")
    block = np.isfinite(case["M"]) & ~case["vM"]
    plain_F, plain_M = np.rint((case["F"] - 600.0) * 0.4), np.rint((case["M"] - 600.0) * 0.4)      # (NaN stays NaN)
    F, M = (plain_F + CAMERA_OFFSET).astype(np.float32), (plain_M + CAMERA_OFFSET).astype(np.float32)
    M[block] = 65535.0
    plain_M[block] = 65535.0 - CAMERA_OFFSET
    return _variant(case, "nan_13x20_camera_offset", F=F, M=M, plain_F=plain_F.astype(np.float32), plain_M=plain_M.astype(np.float32))


THRESHOLD_VALUE = np.float32(0.1)      # (double)float32(0.1) = 0.100000001490116 > 0.1


def threshold_case():
    """(12, 18) crops of a smooth field in about 0.2 .. 1.2 cut at the offset (2, -3), all finite, no masks; a seeded quarter of the
    voxels of each crop holds float32(0.1) exactly and a tenth 0.05.  With ``valid_above=0.1`` the former are valid, with
    ``valid_above=float(np.float32(0.1))`` they are not; the latter never are."""
    shape, offset = (12, 18), (2, -3)
    rng = np.random.default_rng(3)
    G = ndimage.gaussian_filter(rng.random([s + 2 * PAD for s in shape]), 1.5) * 5.0 - 1.8
    F = G[tuple(slice(PAD, PAD + s) for s in shape)].astype(np.float32)
    M = G[tuple(slice(PAD - k, PAD - k + s) for s, k in zip(shape, offset))].astype(np.float32)
    for im in (F, M):
        im += rng.normal(0, 0.02, shape).astype(np.float32)
        kind = rng.random(shape)
        im[kind < 0.25] = THRESHOLD_VALUE
        im[kind > 0.9] = np.float32(0.05)
    return {"name": "threshold_12x18", "F": np.ascontiguousarray(F), "M": np.ascontiguousarray(M), "kwargs": {}, "max_shift": None, "offset": list(offset)}


def eligibility_case():
    """All-valid (8, 16) crops with the planted offset (4, 0) and ``min_overlap=1``: N(s) = (8 - |s_z|)(16 - |s_x|), max N = 128, and
    N = 64 at the planted shift: exactly at the bound of ``overlap_ratio=0.5`` (eligible), below that of 0.51."""
    shape, offset = (8, 16), (4, 0)
    rng = np.random.default_rng(5)
    G = ndimage.gaussian_filter(rng.random([s + 2 * PAD for s in shape]), 1.5) * 1000.0 + 100.0
    F = G[tuple(slice(PAD, PAD + s) for s in shape)].astype(np.float32) + rng.normal(0, 5, shape).astype(np.float32)
    M = G[tuple(slice(PAD - k, PAD - k + s) for s, k in zip(shape, offset))].astype(np.float32) + rng.normal(0, 5, shape).astype(np.float32)
    return {"name": "all_valid_8x16", "F": np.ascontiguousarray(F), "M": np.ascontiguousarray(M), "kwargs": {"min_overlap": 1}, "max_shift": None,
            "offset": list(offset), "vF": np.ones(shape, bool), "vM": np.ones(shape, bool)}


_cache = {}


def value_case(name, **kwargs):
    """One of the value-edge cases with its brute force and float32 restatement under the case's keyword arguments updated by
    ``kwargs``, computed once per (name, kwargs) and shared."""
    from tests.masked_corr_oracle import brute_force, float32_chain

    key = (name, tuple(sorted(kwargs.items())))
    if key not in _cache:
        case = {"inf": infinity_case, "camera": camera_offset_case, "threshold": threshold_case, "eligibility": eligibility_case}[name]()
        kw = dict(case["kwargs"])
        kw.update(kwargs)
        case = dict(case, kwargs=kw)
        kw = dict(kw)
        kw.setdefault("valid_above", (None, None))
        _cache[key] = (case, brute_force(case["F"], case["M"], max_shift=case["max_shift"], **kw),
                       float32_chain(case["F"], case["M"], max_shift=case["max_shift"], **kw))
    return _cache[key]


def case_with_oracle(name):
    """The case, the float64 result (the brute force; of a large case ``fft_float64`` in its place) and the float32 restatement,
    computed once and shared (treat them as read-only)."""
    if name not in _cache:
        from tests.masked_corr_oracle import brute_force, fft_float64, float32_chain

        case = make_case(name)
        kw = dict(case["kwargs"])
        kw.setdefault("valid_above", (None, None))
        exact = fft_float64 if name in LARGE_CASES else brute_force
        _cache[name] = (case, exact(case["F"], case["M"], max_shift=case["max_shift"], **kw),
                        float32_chain(case["F"], case["M"], max_shift=case["max_shift"], **kw))
    return _cache[name]
