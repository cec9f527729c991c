"""GPU: the Spearman coefficient of mvs_score.hip by each of its three routes, on tied data and on device-resident crops.

  sort32   compaction, two float radix sorts, ranks_sorted_kernel<float> / rankcorr_kernel       (host crops, float crops)
  sort16   the same with the fixed crop's raw 16-bit integers as sort keys                        (device-resident integer crops;
           where only the size of the tables keeps a pair from the histograms, the moving crop's exact integer key sums too)
  hist     hist_rank_kernel<false>, hist_fold_kernel, rank_table_kernel, hist_rank_kernel<true>   (device-resident integer crops,
           both finite, every shift component a multiple of 1/2, nbx + nby <= 48 * 1024 bins)

Every case reads the counters "reg_rank_hist" / "reg_rank_sort16" / "reg_rank_sort32" and asserts the route it was built for.

Reference: scipy.stats.spearmanr in float64 over the jointly valid voxels on EXACT keys -- the raw integers of the fixed crop and
the moving crop's integers interpolated in float64 (shifts that are multiples of 1/2: sums of integers times 1/2^k, exact), or,
on the float route, the inputs themselves under whole-pixel shifts.  Every average rank is a multiple of 1/2 below 2^24, exact in
float32; the three sums run in float64 over at most 3e5 terms, so the coefficient is determined to about n * 2^-53 ~ 3e-11:
the bar is 1e-9 (derived, not measured).  End-to-end cases also keep the project's bars against the scipy-on-float32 oracle
(oracle/reg_oracle.py): translation equal, quality within 1e-6 -- that oracle interpolates rescaled float32 values, so its ties
may differ from the exact ones: the hist cases below differ from it by up to 7e-8, and so did the sort16 fallback of the bin-limit
case with a half-integer axis from the exact keys (2.3e-8: rescaled taps rounded to float32 before the interpolation, so equal
key sums a + b == c + d came out one ulp apart) until compact_kernel<true> ranked that case by the exact key sums as well.

Data: microscopy-like crops -- zero background and a saturated plateau (lowest 30 % of a smooth field clipped to 0, top 20 % to the
maximum) -- so that both sorts see runs of equal keys that enter, leave and span the 2048-key chunks of chunk_average_ranks, and,
for the sort32 route, chosen multisets of levels permuted in space.  Not covered here (they need more than 16.7 M voxels / 4.2 M
keys): the non-folded flush of hist_rank_kernel and the gridDim stride loop of the rank kernels; tests/test_rank_plan_host.py
checks the sizing arithmetic of the former."""
import functools
import warnings

import numpy as np
import pytest
from scipy import ndimage, stats

from oracle import reg_oracle as ro

pytestmark = pytest.mark.gpu

K_HIST_BINS_MAX = 48 * 1024          # kHistBinsMax of csrc/mvs_score.hip: x + y bins of a workgroup's private histogram
K_RANK_CHUNK = 2048                  # kRankChunk: sorted keys per turn of chunk_average_ranks
ROUTES = ("hist", "sort16", "sort32")
BAR = 1e-9


def _reset_routes():
    from multiview_stitcher_amd import _lib

    for r in ROUTES:
        _lib.get_counter("reg_rank_" + r, reset=True)


def _routes_taken():
    from multiview_stitcher_amd import _lib

    return {r: _lib.get_counter("reg_rank_" + r, reset=True) for r in ROUTES}


def _only(route, times=1):
    return {r: float(times if r == route else 0) for r in ROUTES}


def _same(got, want, bar):
    """Both NaN, or both finite and within ``bar``."""
    if np.isnan(want):
        return bool(np.isnan(got))
    return bool(np.isfinite(got)) and abs(got - want) <= bar


def _exact_spearman(a, b, t):
    """spearmanr in float64 over the jointly valid voxels of the fixed crop and the moving crop under the candidate ``t`` (the
    translation of the affine: im1t[o] = im1[o + t], i.e. the content moves by -t), on exact keys."""
    bt = ndimage.shift(b.astype(np.float64), -np.asarray(t, dtype=np.float64), order=1, mode="constant", cval=np.nan)
    mask = ~np.isnan(a) & ~np.isnan(bt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (a constant input: NaN, with a warning)
        return float(stats.spearmanr(a[mask].astype(np.float64), bt[mask]).correlation)


def _hist_bins(a, b, t):
    """nbx + nby as hist_ranks_apply computes them from the raw extrema of the crops (0 = the histogram route does not apply)."""
    t = np.asarray(t, dtype=np.float64)
    if np.isnan(a).any() or np.isnan(b).any() or np.any(t * 2 != np.floor(t * 2)):
        return 0
    nf = int(np.sum(t != np.floor(t)))
    nbx = int(a.max()) - int(a.min()) + 1
    nby = (int(b.max()) - int(b.min())) * 2**nf + 1
    return nbx + nby


def _is_u16(a):
    v = a[~np.isnan(a)]
    return bool(np.all((v >= 0) & (v <= 65535) & (v == np.floor(v))))


def _expected_route(a, b, t):
    """The route a DEVICE-RESIDENT pair takes for the winning candidate ``t`` (mvs_pair.hip:61-72, hist_ranks_apply)."""
    if _is_u16(a) and _is_u16(b) and 0 < _hist_bins(a, b, t) <= K_HIST_BINS_MAX:
        return "hist"
    return "sort16" if _is_u16(a) else "sort32"


# ---- a) sort32 through score_candidates: chosen multisets of levels ------------------------------------------------------------

SORT32_M = [2047, 2048, 2049, 4096, 4097, 6400, 2993, 5207]        # the last two: m % 8 == 1 and 7 (float4 store tail)
LAYOUTS = ["distinct", "two_levels", "run_spans_a_chunk", "run_ends_at_2048", "single_at_2047", "constant"]


def _sorted_levels(m, layout):
    """The fixed image's keys in sorted order (level ids; equal ids = one run)."""
    ids = np.arange(m)
    if layout == "distinct":
        return ids
    if layout == "two_levels":
        return (ids >= m // 2).astype(np.int64)
    if layout == "constant":
        return np.zeros(m, dtype=np.int64)
    if layout == "run_spans_a_chunk":
        # starts inside chunk 0; with more than two chunks it ends inside chunk 2 (chunk 1 lies wholly inside it), else at the end
        runs = [(min(1000, m // 4), m if m <= 2 * K_RANK_CHUNK + 1 else max(m - m // 4, 2 * K_RANK_CHUNK + 1))]
    elif layout == "run_ends_at_2048":
        end = min(K_RANK_CHUNK, m)
        runs = [(end - 700, end)]
    else:       # a run of length 1 at position 2047 (the last key of chunk 0) between two long runs
        p = min(K_RANK_CHUNK - 1, m - 1)
        runs = [(p - 1000, p), (p + 1, min(m, p + 1 + 1500))]
    for s, e in runs:
        ids[s:e] = s
    return ids


@functools.lru_cache(maxsize=None)
def _level_images(m, layout):
    shape = (100, 64) if m > 3009 else (59, 51)
    n = shape[0] * shape[1]
    rng = np.random.default_rng(m * 7 + LAYOUTS.index(layout))
    levels = _sorted_levels(m, layout).astype(np.float64)
    x = levels / max(levels.max(), 1.0)
    # a noisy monotone function of the fixed image, requantised to 12 levels: long runs in the second sort, 0 < |rho| < 1
    y = np.clip(np.floor((x + 0.25 * rng.standard_normal(m)) * 8.0), -2, 9)
    where = rng.permutation(n)[:m]
    im0 = np.full(n, np.nan, dtype=np.float32)
    im1 = np.clip(np.floor(rng.standard_normal(n) * 3.0), -2, 9).astype(np.float32)
    im0[where] = levels.astype(np.float32)
    im1[where] = y.astype(np.float32)
    im0, im1 = im0.reshape(shape), im1.reshape(shape)
    assert int(np.sum(~np.isnan(im0))) == m
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        im0, im1 = ro.rescale_intensity_01(im0), ro.rescale_intensity_01(im1)
    for im in (im0, im1):
        im.setflags(write=False)
    return im0, im1


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m", SORT32_M)
def test_sort32_ranks_of_tied_levels_match_scipy(hip_device, m, layout):
    """Host float crops: compaction, two float sorts, ranks_sorted_kernel<float>, rankcorr_kernel.  ``m`` jointly valid voxels (NaNs
    in the fixed image) at the chunk edges 2047 / 2048 / 2049 / 4096 / 4097, several chunks, and ragged float4 tails; runs of equal
    keys that start, end and lie across the chunks.  Whole-pixel candidates only: the ranked values are the inputs themselves, so
    the oracle's float32 keys are exact and the Spearman bar is 1e-9.  A constant fixed image gives what scipy gives (NaN)."""
    from multiview_stitcher_amd import _reg_ops

    im0, im1 = _level_images(m, layout)
    cands = [[0.0, 0.0], [2.0, -3.0]]
    im0nm = np.isnan(im0)
    data_range = float(np.nanmax([im0, im1]) - np.nanmin([im0, im1]))
    im1_min = float(np.nanmin(im1))
    valid1 = np.sum(~np.isnan(im1))
    im0_bb = ro.get_bb_from_nanmask(~im0nm)
    _reset_routes()
    ssim, spear, codes = _reg_ops.score_candidates(im0, im1, cands, "intersection", data_range, im1_min, quality_for_all=True)
    taken = _routes_taken()
    for i, t in enumerate(cands):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            code, s, q = ro.score_candidate(im0, im1, im0nm, t, valid1, "intersection", data_range, im1_min, im0_bb)
        print(f"sort32 m={m} {layout} t={t}: code {codes[i]} spearman {spear[i]!r} want {q!r} diff {abs(spear[i] - q) if code == 0 else 0.0:.3e}")
        assert code == 0 and codes[i] == 0, (i, t, codes[i], code)
        assert abs(ssim[i] - s) <= 2e-5 * max(abs(s), 1e-3), (i, t, ssim[i], s)
        assert _same(spear[i], q, BAR), (i, t, spear[i], q)
        if layout not in ("constant", "distinct"):
            assert 0.05 < abs(q) < 0.999 or i == 1
    assert taken == _only("sort32", len(cands)), taken


# ---- b), c) sort16 and hist through register_crops on device-resident integer crops ----------------------------------------------

def _plateau_fields(shape, seed, vmax, sigma=2.0, noise=0.03):
    """A smooth random field, its lowest 30 % clipped to 0 and its top 20 % to ``vmax``, rounded to integers -- once as it is (the
    fixed tile) and once with independent noise added before the clipping (the moving tile: the coefficient is not 1)."""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.random(shape), sigma)
    lo, hi = np.quantile(f, [0.3, 0.8])
    g = f + noise * (hi - lo) * rng.standard_normal(shape)
    return tuple(np.round(np.clip((v - lo) / (hi - lo), 0.0, 1.0) * vmax) for v in (f, g))


def _whole_pixel_pair(shape, shift, vmax, seed):
    """b[o] = a[o + shift]: the winning candidate is t = -shift."""
    pad = 8
    big0, big1 = _plateau_fields(tuple(s + 2 * pad for s in shape), seed, vmax)
    a = np.ascontiguousarray(big0[tuple(slice(pad, pad + s) for s in shape)]).astype(np.float32)
    b = np.ascontiguousarray(big1[tuple(slice(pad + d, pad + d + s) for d, s in zip(shift, shape))]).astype(np.float32)
    return a, b, -np.asarray(shift, dtype=np.float64)


def _binned_pair(shape, jit, vmax, seed, noise=0.03):
    """uint16 tiles binned by 2 (block mean cast back to uint16) from offsets that differ by ``jit`` unbinned pixels: an odd
    component is a half-integer shift on the binned grid.  The winning candidate is t = -jit / 2."""
    pad = 8
    ndim = len(shape)
    bigs = [v.astype(np.uint16) for v in _plateau_fields(tuple(2 * s + 2 * pad for s in shape), seed, vmax, sigma=3.0, noise=noise)]

    def binned(big, off):
        sl = tuple(slice(pad + o, pad + o + 2 * s) for o, s in zip(off, shape))
        v = big[sl].astype(np.float64).reshape([q for s in shape for q in (s, 2)]).mean(axis=tuple(range(1, 2 * ndim, 2)))
        return v.astype(np.uint16).astype(np.float32)

    return binned(bigs[0], (0,) * ndim), binned(bigs[1], jit), -np.asarray(jit, dtype=np.float64) / 2.0


def _planted(a, b, t, max0, max1):
    """The same pair with one voxel of each crop raised to ``max0`` / ``max1`` (the same spot of the structure, to the pixel): the
    raw extrema hist_ranks_apply sizes its tables from."""
    a, b = a.copy(), b.copy()
    p = tuple(s // 2 for s in a.shape)
    a[p] = max0
    b[tuple(int(pi + np.floor(ti)) for pi, ti in zip(p, t))] = max1
    assert a.min() == 0 and b.min() == 0 and a.max() == max0 and b.max() == max1
    return a, b


CROP_CASES = {
    # b) sort16: a value range too wide for the histograms (2 * 40001 bins), 3D and 2D; a small range with NaN columns
    "sort16_3d_wide": lambda: _whole_pixel_pair((24, 40, 36), (2, -3, 4), 40000, 11) + (2, "sort16"),
    "sort16_2d_wide": lambda: _whole_pixel_pair((96, 80), (5, -7), 40000, 12) + (10, "sort16"),
    "sort16_3d_nan_columns": lambda: _nan_columns(_whole_pixel_pair((24, 40, 36), (1, 2, -3), 3000, 13)) + (2, "sort16"),
    # c) hist: whole-pixel and half-integer shifts on 1, 2, 3 axes of either sign; one part (n < 8192), several parts, odd nx and n
    "hist_3d_whole": lambda: _binned_pair((24, 40, 36), (2, -4, 2), 4095, 21) + (2, "hist"),
    "hist_3d_half_1_axis_one_part": lambda: _binned_pair((12, 20, 30), (2, -3, 4), 4095, 22) + (2, "hist"),
    "hist_3d_half_2_axes_odd": lambda: _binned_pair((9, 31, 33), (2, 3, -5), 4000, 23) + (2, "hist"),
    "hist_3d_half_3_axes": lambda: _binned_pair((24, 40, 36), (-1, 3, -5), 3500, 24) + (2, "hist"),
    "hist_2d_half_1_axis": lambda: _binned_pair((96, 80), (3, -2), 4095, 25) + (2, "hist"),
    "hist_2d_half_2_axes_odd": lambda: _binned_pair((95, 81), (-3, 5), 1000, 26) + (2, "hist"),
    # a few thousand voxels and more noise: an error common to all ranks of a table (a constant c added to the centred ranks changes
    # the coefficient by about 12 c^2 (1 - rho) / n^2) stays above the bar only on crops this small
    "hist_2d_small_half_1_axis": lambda: _binned_pair((40, 36), (3, -2), 4095, 41, noise=0.1) + (2, "hist"),
    "hist_2d_small_half_2_axes_odd": lambda: _binned_pair((33, 45), (-3, 5), 4095, 42, noise=0.1) + (2, "hist"),
    "hist_3d_small_half_1_axis": lambda: _binned_pair((8, 20, 24), (2, -3, 4), 4095, 43, noise=0.1) + (2, "hist"),
    # the bin limit: nbx + nby == kHistBinsMax (96 KiB of LDS) is hist, one more is sort16
    "limit_whole_at": lambda: _limit_case((2, -4, 2), 24575, 24575) + (2, "hist"),
    "limit_whole_above": lambda: _limit_case((2, -4, 2), 24575, 24576) + (2, "sort16"),
    "limit_half_at": lambda: _limit_case((2, -3, 4), 16384, 16383) + (2, "hist"),
    "limit_half_above": lambda: _limit_case((2, -3, 4), 16385, 16383) + (2, "sort16"),
}
LIMIT_BINS = {"limit_whole_at": K_HIST_BINS_MAX, "limit_whole_above": K_HIST_BINS_MAX + 1, "limit_half_at": K_HIST_BINS_MAX,
              "limit_half_above": K_HIST_BINS_MAX + 1}


def _nan_columns(pair):
    a, b, t = pair
    a = a.copy()
    a[..., :3] = np.nan          # the fixed crop only: the moving crop's interpolated keys stay finite wherever they are inside
    return a, b, t


def _limit_case(jit, max0, max1):
    a, b, t = _binned_pair((24, 40, 36), jit, 4095, 31)
    return _planted(a, b, t, max0, max1) + (t,)


@functools.lru_cache(maxsize=None)
def _crop_case(name):
    """(fixed, moving, planted translation, upsample factor, route, oracle result, exact-key coefficient): computed once."""
    a, b, t, up, route = CROP_CASES[name]()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = ro.phase_correlation_registration(a, b, upsample_factor=up)
    for im in (a, b):
        im.setflags(write=False)
    return a, b, t, up, route, want, _exact_spearman(a, b, t)


@pytest.mark.parametrize("name", list(CROP_CASES))
def test_device_resident_integer_crops_rank_by_their_route(hip_device, name):
    """mvs_register_crops on DeviceArray crops of integer tiles with a zero background and a saturated plateau: the route the pair
    was built for ran (exactly one rank correlation: the winner's), the translation is the planted one and the oracle's, and the
    quality equals scipy's on the exact keys to 1e-9 and the oracle's to 1e-6."""
    from multiview_stitcher_amd import _reg_ops
    from multiview_stitcher_amd.device import DeviceArray

    a, b, t_true, up, route, want, exact = _crop_case(name)
    # on the CPU, before anything runs: the pair is what the case says it is
    assert _is_u16(a) and _is_u16(b)
    if name in LIMIT_BINS:
        assert _hist_bins(a, b, t_true) == LIMIT_BINS[name]
    elif route == "sort16" and not np.isnan(a).any():
        assert _hist_bins(a, b, t_true) > K_HIST_BINS_MAX
    elif route == "hist":
        assert max(a.max(), b.max()) <= 4095
    assert _expected_route(a, b, t_true) == route
    np.testing.assert_array_equal(want["affine_matrix"][:-1, -1], t_true)
    assert np.isfinite(exact) and 0.05 < exact < 0.9999
    # both plateaus hold a large share of the voxels: runs far longer than a chunk of 2048 keys (or one histogram part)
    assert np.mean(a == 0) > 0.15 and np.mean(a >= min(np.nanmax(a), 4095)) > 0.1

    _reset_routes()
    t, q, st, nc = _reg_ops.register_crops(DeviceArray.from_host(a), DeviceArray.from_host(b), up)
    taken = _routes_taken()
    print(f"{route} {name}: t {t} quality {q!r} exact {exact!r} diff {abs(q - exact):.3e} oracle diff {abs(q - want['quality']):.3e} routes {taken}")
    assert st == 0
    assert taken == _only(route), taken
    np.testing.assert_array_equal(t, t_true)
    assert np.isfinite(q)
    assert abs(q - want["quality"]) <= 1e-6
    assert abs(q - exact) <= BAR
