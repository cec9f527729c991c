"""Case table of the tests of the float32 SSIM walk and its float64 re-walk (tests/test_ssim_walk_cases_host.py,
tests/test_ssim_f32_walk_gpu.py).  The pruned arg-max search of the candidate scoring (csrc/mvs_prune_search.h) walks candidates with
running sums and box means in float32 and walks again, in float64, the complete candidates that end within kPruneMarginF32 (mean
SSIM) of the best.  It reproduces the reference's nanargmax only while the float32 mean of every candidate is within half that
margin of its float64 value: the error cases measure that on inputs where the float32 variance terms are worst (bright, flat), the
near-tie cases put two candidates inside the margin so that the re-walk has to decide.

Every case: finite 3D float32 crops rescaled to [0, 1], an explicit candidate list, region mode "union", data range 1, every
candidate with oracle code 0 and the 7-wide window.  The oracle values are computed once per case (`oracle`)."""
import functools
import os
import re
from collections import namedtuple

import numpy as np
from scipy import ndimage

from oracle import reg_oracle as ro
from tests.helpers import _pair, _sparse_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the constants of csrc/mvs_prune_search.h and csrc/mvs_score.hip, restated (tests/test_ssim_walk_cases_host.py holds them against
# the sources' text) ----
MARGIN = 1e-3            # kPruneMarginF32
SLACK = 1e-2             # score_batch: 1e-2 max(1, (value_bound / data_range)^2) for crops in [0, 1] with data range 1
PRUNE_ITEMS = 320        # prune_env: work items a candidate's walk is cut into (about)
SCORE_RTOL, SCORE_FLOOR = 2e-5, 1e-3      # the bar of the score tests: |ssim - oracle| <= 2e-5 max(|oracle|, 1e-3)


def header_margin():
    """kPruneMarginF32 as csrc/mvs_prune_search.h states it."""
    text = open(os.path.join(ROOT, "multiview-stitcher_amd", "csrc", "mvs_prune_search.h")).read()
    (value,) = re.findall(r"constexpr double kPruneMarginF32 = ([0-9.eE+-]+);", text)
    return float(value)


def walk_geometry(shape, budget=PRUNE_ITEMS):
    """WalkGeom<7> (csrc/mvs_prune_search.h) in Python: tiles of 16 x 56 over the interior cropped by 3 per side, z segments of at
    least 8 planes sized for about `budget` work items.  Returns (tiles per segment, segments, planes per segment)."""
    cz, cy, cx = (n - 6 for n in shape)
    tiles = -(-cy // 16) * -(-cx // 56)
    nzs = max(1, min(budget // max(tiles, 1), (cz + 7) // 8))
    zseg = -(-cz // nzs)
    return tiles, -(-cz // zseg), zseg


# name; kind ("error" / "tie"); builder and its arguments; candidates (z, y, x rows); planes per z segment of the walk
Case = namedtuple("Case", "name kind build args candidates zseg")

SMALL = (40, 96, 120)


def _field(shape, seed, sigma, pad=4):
    """A smooth zero-mean texture with max |value| = 1 on `shape` grown by `pad` per side (room for the shifted window)."""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.random(tuple(s + 2 * pad for s in shape)), sigma)
    f -= f.mean()
    return f / np.abs(f).max()


def _pin_range(im):
    """One voxel at 0 and one at 1 (in a corner, inside the border the SSIM crops): rescaling to [0, 1] keeps the level."""
    im[0, 0, 0], im[0, 0, 1] = 0.0, 1.0
    return im


def _bright_pair(shape, level, amp, shift, seed, sigma=2.0, noise=0.25):
    """Two windows of `level + amp * texture`, the moving one displaced by the whole-voxel `shift` (b[i] = a[i + shift]) and carrying
    white noise of `noise * amp`: a bright, nearly flat background, where the window variances (<= amp^2) are small against C2 = 9e-4
    and the float32 error of E[x^2] - E[x]^2 at level^2 counts most."""
    pad = 4
    big = level + amp * _field(shape, seed, sigma, pad)
    a = big[tuple(slice(pad, pad + s) for s in shape)].astype(np.float32)
    b = big[tuple(slice(pad + d, pad + d + s) for d, s in zip(shift, shape))]
    b = (b + noise * amp * np.random.default_rng(seed + 1).standard_normal(shape)).astype(np.float32)
    return _pin_range(np.ascontiguousarray(a)), _pin_range(np.ascontiguousarray(b))


def _mid_pair(shape, shift, noise):
    return _pair(shape, shift, noise=noise)


def _blob_pair(shape, shift):
    """(noise in the moving blob: the aligned candidate ends at 0.99 instead of 1, which keeps its neighbours in the search)"""
    return _sparse_pair(shape, shift, seed=5, invert=False, noise=0.2)


def _scene(shape, seed, level=None, amp=None, pin=None):
    """gaussian_filter(rng.random(shape), 1.5); with level / amp as a bright flat background (`_bright_pair`) that carries the two
    range voxels at `pin` and its x neighbour."""
    big = ndimage.gaussian_filter(np.random.default_rng(seed).random(shape), 1.5)
    if level is not None:
        big -= big.mean()
        big = level + amp * big / np.abs(big).max()
        big[pin], big[pin[:2] + (pin[2] + 1,)] = 0.0, 1.0
    return big


def _blend_pair(shape, eps, seed):
    """The moving crop is (0.5 + eps) s(x) + (0.5 - eps) s(x + 1) of the smooth scene s the fixed crop holds (x: the last axis): the
    candidates (0, 0, 0) and (0, 0, -1) see s mixed with its neighbour on either side and tie at a small eps (not at 0: the shifted
    candidate loses the plane that leaves the crop)."""
    big = _scene(tuple(shape[:2]) + (shape[2] + 1,), seed)
    a = big[:, :, :-1].astype(np.float32)
    b = ((0.5 + eps) * big[:, :, :-1] + (0.5 - eps) * big[:, :, 1:]).astype(np.float32)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def _two_copy_pair(shape, eps, seed, axis, d, level=None, amp=None):
    """The moving crop holds two copies of the scene, (0.5 + eps) s(. + d) + (0.5 - eps) s(. - d) along `axis`: the candidates -d and
    +d each align one copy with the fixed crop and lose the same number of planes at the border, so they tie near eps = 0 on any
    background -- on a bright flat one a candidate that loses one plane more is 0.009 behind -- and the phase correlation of the pair
    finds one of the two copies, so the reference's enumeration (+-estimate) holds both."""
    grown = tuple(n + 2 * d if k == axis else n for k, n in enumerate(shape))
    big = _scene(grown, seed, level, amp, tuple(d if k == axis else 0 for k in range(3)))
    cut = lambda lo: tuple(slice(lo, lo + n) if k == axis else slice(None) for k, n in enumerate(shape))      # noqa: E731
    a = big[cut(d)].astype(np.float32)
    b = ((0.5 + eps) * big[cut(2 * d)] + (0.5 - eps) * big[cut(0)]).astype(np.float32)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def _around(t, far):
    """The aligned candidate, half-voxel and whole-voxel neighbours of it, and one candidate far off."""
    z, y, x = (float(v) for v in t)
    return [(z, y, x), (z, y, x + 0.5), (z, y + 0.5, x), (z + 0.5, y, x), (z, y, x - 1.0), (z, y - 0.5, x - 0.5), tuple(float(v) for v in far)]


# eps of the near ties, tuned with the oracle to a top-two gap of about 5e-4 (tests/test_ssim_walk_cases_host.py holds the gaps)
EPS = {"tie_first_wins": -0.0218, "tie_second_wins": -0.0259, "tie_bright_flat": 0.0172,
       "pair_first_wins": 0.00136, "pair_second_wins": 0.000973, "pair_bright_flat": 0.00909}
TIE_CANDIDATES = [(0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 0.0, 0.5), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)]

CASES = [
    Case("bright_flat", "error", _bright_pair, (SMALL, 0.9, 0.02, (1, -2, 3), 21), _around((-1, 2, -3), (3, -5, 7)), 7),
    Case("near_saturated", "error", _bright_pair, (SMALL, 0.97, 0.005, (1, -2, 3), 22), _around((-1, 2, -3), (3, -5, 7)), 7),
    Case("mid_texture", "error", _mid_pair, (SMALL, (2, -3, 4), 0.02), _around((-2, 3, -4), (3, -5, 7)), 7),
    # (the blob is 10 planes thick: half a voxel along z costs more than the others)
    Case("sparse_blob", "error", _blob_pair, (SMALL, (2, -3, 4)),
         [(-2.0, 3.0, -4.0), (-2.0, 3.0, -3.5), (-2.0, 3.5, -4.0), (-2.0, 3.0, -4.5), (-2.0, 2.5, -4.0), (-1.5, 3.0, -4.0), (3.0, -5.0, 7.0)], 7),
    # 80 tiles, 4 z segments of 13 planes: the z-neighbour crops of the bench mosaic
    Case("workload_segment", "error", _bright_pair, ((57, 262, 286), 0.9, 0.02, (1, -2, 3), 23), _around((-1, 2, -3), (3, -5, 7))[:4], 13),
    # 161 tiles: one segment of 24 planes, the longest running sum a volume of this size gets
    Case("one_segment", "error", _bright_pair, ((30, 374, 398), 0.9, 0.02, (1, -2, 3), 24), _around((-1, 2, -3), (3, -5, 7))[:4], 24),
    Case("tie_first_wins", "tie", _blend_pair, (SMALL, EPS["tie_first_wins"], 4), TIE_CANDIDATES, 7),
    Case("tie_second_wins", "tie", _blend_pair, (SMALL, EPS["tie_second_wins"], 4), TIE_CANDIDATES, 7),
    # bright flat: the pair that ties is -1 / +1 along x (two copies), every other candidate loses one plane more
    Case("tie_bright_flat", "tie", _two_copy_pair, (SMALL, EPS["tie_bright_flat"], 4, 2, 1, 0.9, 0.02),
         [(0.0, 0.0, -1.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.5), (0.0, 0.0, 1.5), (1.0, 0.0, -1.0)], 7),
]
ERROR_CASES = [c for c in CASES if c.kind == "error"]
TIE_CASES = [c for c in CASES if c.kind == "tie"]


# The near ties as crop pairs of the whole registration (register_crops): two copies 5 voxels either side along y, so that the
# reference's enumeration holds the pair that ties, (0, -5, 0) and (0, 5, 0).  name -> arguments of _two_copy_pair
TIE_PAIRS = {
    "pair_first_wins": (SMALL, EPS["pair_first_wins"], 4, 1, 5),
    "pair_second_wins": (SMALL, EPS["pair_second_wins"], 4, 1, 5),
    "pair_bright_flat": (SMALL, EPS["pair_bright_flat"], 4, 1, 5, 0.9, 0.02),
}
PAIR_NEAR_TIE = [(0.0, -5.0, 0.0), (0.0, 5.0, 0.0)]


@functools.lru_cache(maxsize=None)
def tie_pair(name):
    """The (unrescaled) crops of a near-tie pair and the oracle's whole registration of them, with its debug record."""
    a, b = _two_copy_pair(*TIE_PAIRS[name])
    want = ro.phase_correlation_registration(a, b, return_debug=True)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, want


def by_name(name):
    (case,) = [c for c in CASES if c.name == name]
    return case


@functools.lru_cache(maxsize=None)
def crops(name):
    """The rescaled crops of a case (read-only: shared by the tests)."""
    case = by_name(name)
    a, b = case.build(*case.args)
    im0, im1 = ro.rescale_intensity_01(a), ro.rescale_intensity_01(b)
    im0.setflags(write=False)
    im1.setflags(write=False)
    return im0, im1


def scoring_args(im0, im1):
    """data_range, im1_min, value_bound as registration.phase_correlation_registration derives them from rescaled crops."""
    data_range = float(np.nanmax([im0, im1]) - np.nanmin([im0, im1]))
    return data_range, float(np.nanmin(im1)), float(max(np.abs(im0).max(), np.abs(im1).max()))


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Per candidate of the case: (codes, SSIM values, Spearman coefficients) of the oracle's candidate loop."""
    case = by_name(name)
    im0, im1 = crops(name)
    data_range, im1_min, _ = scoring_args(im0, im1)
    im0nm = np.isnan(im0)
    bb0 = ro.get_bb_from_nanmask(~im0nm)
    res = [ro.score_candidate(im0, im1, im0nm, t, im1.size, "union", data_range, im1_min, bb0) for t in case.candidates]
    codes = np.array([r[0] for r in res])
    ssim = np.array([np.nan if r[1] is None else r[1] for r in res], dtype=np.float64)
    spear = np.array([np.nan if r[2] is None else r[2] for r in res], dtype=np.float64)
    for v in (codes, ssim, spear):
        v.setflags(write=False)
    return codes, ssim, spear
