"""Case table of the thin-overlap tests (tests/test_thin_overlap_host.py, tests/test_thin_overlap_gpu.py): crops whose SSIM region
has a shortest axis below 9, where candidate scoring leaves the 7-wide window -- 5 for a shortest axis of 5 or 6, 3 for 3 or 4,
no SSIM (value -1) below 3 -- and the lower edge of the 7-wide fast path (shortest axis 7 or 8).  Plain data plus the `_pair` call:
the host test checks with the oracle that every case is what it says it is, the GPU test runs the library on it."""
from collections import namedtuple

import numpy as np

from tests.helpers import _pair

# shape, true shift: the crops of _pair(shape, shift) (default seed and sigma)
# nan_band: None or (axis, start, width) -- the MOVING crop is valid only inside [start, start + width) along `axis`
# region_mode: "union" / "intersection"
# window: the SSIM window every code-0 candidate must get (0 = none: SSIM is -1), or one entry per candidate where the candidates of
#         one case differ (None for a candidate that fails the 10 % mask test)
# group: "a" finite 3D, "b" finite 2D, "c" NaN bands, "d" lower edge of the 7-wide fast path
ScoreCase = namedtuple("ScoreCase", "name group shape shift nan_band region_mode window")


def crops(case):
    """The pair of a case, NaN band applied."""
    a, b = _pair(case.shape, case.shift)
    if getattr(case, "nan_band", None) is not None:
        axis, start, width = case.nan_band
        keep = np.zeros(case.shape[axis], bool)
        keep[start:start + width] = True
        b = b.copy()
        b[tuple(~keep if d == axis else slice(None) for d in range(len(case.shape)))] = np.nan
    return a, b


def candidates(case):
    """Zero, the negated true shift, the negated true shift plus 1/2 on every axis, a shift in tenths of a pixel and one candidate
    that leaves less than 10 % of the moving crop (95 % of the longest axis)."""
    shape, nd = case.shape, len(case.shape)
    neg = [-float(s) for s in case.shift]
    tenth = [0.3, 0.0, -0.7][3 - nd:] if nd == 3 else [0.3, -0.7]
    far = [0.0] * nd
    far[int(np.argmax(shape))] = 0.95 * max(shape)
    return [[0.0] * nd, neg, [v + 0.5 for v in neg], tenth, far]


def _finite(group, shape, shift, window):
    return ScoreCase("x".join(map(str, shape)), group, shape, shift, None, "union", window)


def _band(shape, shift, band, window):
    """One "intersection" case on the window of the band and the same inputs under "union", which stay on the 7-wide window."""
    name = "x".join(map(str, shape)) + "_axis%d_%d:%d" % (band[0], band[1], band[1] + band[2])
    return [ScoreCase(name + "_intersection", "c", shape, shift, band, "intersection", window),
            ScoreCase(name + "_union", "c", shape, shift, band, "union", 7)]


SCORE_CASES = [
    # a. finite 3D crops, thin axis in each position
    _finite("a", (6, 48, 40), (1, -2, 3), 5), _finite("a", (5, 48, 40), (1, -2, 3), 5),
    _finite("a", (4, 48, 40), (1, -2, 3), 3), _finite("a", (3, 48, 40), (1, -2, 3), 3),
    _finite("a", (2, 48, 40), (0, -2, 3), 0), _finite("a", (1, 48, 40), (0, -2, 3), 0),
    _finite("a", (40, 5, 48), (2, 1, -3), 5), _finite("a", (40, 4, 48), (2, 1, -3), 3),
    _finite("a", (40, 48, 5), (2, -3, 1), 5), _finite("a", (40, 48, 4), (2, -3, 1), 3),
    # b. finite 2D crops
    _finite("b", (5, 64), (1, -4), 5), _finite("b", (6, 64), (1, -4), 5), _finite("b", (64, 4), (3, 1), 3),
    _finite("b", (3, 50), (1, 2), 3), _finite("b", (2, 50), (0, 2), 0), _finite("b", (6, 6), (1, -1), 5),
    # c. NaN bands inside full-size crops: a band of width w leaves a region of w - 1 (the zero-weight NaN tap of the order-1
    # interpolation takes the last sample), its origin not at 0
    *_band((24, 40, 36), (2, -3, 4), (0, 9, 7), 5),
    *_band((24, 40, 36), (2, -3, 4), (1, 17, 5), 3),
    *_band((24, 40, 36), (2, -3, 4), (2, 20, 7), 5),
    *_band((24, 40, 36), (2, -3, 4), (0, 3, 3), 0),
    *_band((24, 40, 36), (2, -3, 4), (2, 30, 2), 0),
    *_band((40, 90), (2, -3), (0, 11, 5), 3),
    # columns 0:7: the candidates that move the band to the left lose what leaves the crop -- 3 columns stay
    *_band((40, 90), (2, -3), (1, 0, 7), (5, 3, 3, 5, None)),
    *_band((40, 90), (2, -3), (1, 50, 3), 0),
    # d. the lower edge of the 7-wide fast path: a cropped interior 1 or 2 voxels thick, fewer walk items than residue classes
    _finite("d", (7, 48, 40), (1, -2, 3), 7), _finite("d", (8, 48, 40), (1, -2, 3), 7),
    _finite("d", (48, 7, 40), (2, 1, -3), 7), _finite("d", (48, 40, 8), (2, -3, 1), 7),
    _finite("d", (7, 7, 7), (1, 0, -1), 7), _finite("d", (8, 9, 7), (1, -1, 1), 7),
]

# End to end (phase correlation + candidate scoring): finite crops, region mode and upsample factor left to the default
E2eCase = namedtuple("E2eCase", "name shape shift all_minus_one")


def _e2e(shape, shift, all_minus_one=False):
    return E2eCase("x".join(map(str, shape)), shape, shift, all_minus_one)


E2E_CASES = [
    _e2e((6, 48, 40), (1, -2, 3)), _e2e((5, 48, 40), (1, -2, 3)), _e2e((4, 48, 40), (1, -2, 3)), _e2e((3, 48, 40), (1, -2, 3)),
    _e2e((2, 48, 40), (0, -2, 3), True), _e2e((1, 48, 40), (0, -2, 3), True),
    _e2e((40, 5, 48), (2, 1, -3)), _e2e((40, 48, 4), (2, -3, 1)),
    _e2e((7, 48, 40), (1, -2, 3)), _e2e((8, 48, 40), (1, -2, 3)), _e2e((7, 7, 7), (1, 0, -1)),
    _e2e((5, 64), (1, -4)), _e2e((64, 4), (3, 1)), _e2e((3, 50), (1, 2)), _e2e((2, 50), (0, 2), True), _e2e((6, 6), (1, -1)),
]
# the cases that run under the switches of the candidate search (ssim_prune off, materialize_shifts on, the defaults)
SWITCH_SHAPES = [(7, 48, 40), (8, 48, 40), (7, 7, 7), (5, 48, 40)]
# finite integer-valued crops, resident on the device: rank correlation through the key histograms.  The float sorts of the host
# run and the histograms rank the same values only where the winner is a whole-pixel shift (the moving values are copies of the
# taps): those cases carry the rel=1e-10 demand.  A half-pixel winner interpolates, and float32 rounding splits ties of the exact
# tap sums (5x48x40: 1537 distinct float32 values against 1172 distinct sums), which the histograms keep: these cases
# (INTEGER_HALF_SHAPES, shifts of E2E_CASES) are compared with the rank correlation of the exact sums instead.
INTEGER_SHAPES = [(5, 48, 40), (3, 48, 40)]
INTEGER_WHOLE_CASES = [E2eCase("5x48x40_whole", (5, 48, 40), (0, -2, 3), False), E2eCase("3x48x40_whole", (3, 48, 40), (0, -2, 3), False)]
INTEGER_HALF_SHAPES = [(5, 48, 40), (3, 48, 40)]


def integer_crops(case):
    """The pair of a case as integer-valued float32 crops (uint16 tiles on the fixed grid)."""
    a, b = crops(case)
    return np.round(a * 3000).astype(np.float32), np.round(b * 3000).astype(np.float32)


def exact_key_spearman(a, b, t):
    """Spearman coefficient of the fixed crop against the EXACT tap sums of the moving crop shifted by t (every component a multiple
    of 1/2, finite crops): scipy's ranks of integers, no float32 rounding of the interpolated value."""
    from scipy import stats

    sl_a, taps = [], [[]]
    for n, tk in zip(a.shape, t):
        f = int(np.floor(tk))
        h = 1 if tk != f else 0
        lo, hi = max(0, -f), min(n, n - f - h)
        sl_a.append(slice(lo, hi))
        taps = [p + [slice(lo + f + o, hi + f + o)] for p in taps for o in range(h + 1)]
    key = sum(b[tuple(p)].astype(np.float64) for p in taps)
    return float(stats.spearmanr(a[tuple(sl_a)].ravel(), key.ravel()).correlation)


def by_shape(cases, shape):
    (case,) = [c for c in cases if c.shape == tuple(shape) and getattr(c, "nan_band", None) is None]
    return case
