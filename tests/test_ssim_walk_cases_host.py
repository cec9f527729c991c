"""The preconditions of the float32-walk cases (tests/ssim_walk_cases.py), checked with the oracle alone: every candidate is scored
(code 0) on the 7-wide window of finite crops in [0, 1]; every near tie has its top two candidates inside the margin of the float32
walk and the third well outside; every case has the walk geometry it is listed for and would take the pruned search; and the
near-tie crop pairs of the whole registration still enumerate the pair that ties.  A case that fails here is retuned (seed, eps,
candidates); it is never skipped or dropped.  The constants the case table restates are held against the sources' text."""
import os
import re

import numpy as np
import pytest

from tests import ssim_walk_cases as sc

CSRC = os.path.join(sc.ROOT, "multiview-stitcher_amd", "csrc")


def test_restated_constants_equal_the_sources():
    assert sc.header_margin() == sc.MARGIN == 1e-3
    score = open(os.path.join(CSRC, "mvs_score.hip")).read()
    assert "const double slack = 1e-2 * std::max(1.0, (vb / sc.data_range) * (vb / sc.data_range));" in score and sc.SLACK == 1e-2
    assert "prune && n_in >= 2 && sc.data_range > 0.0 && std::isfinite(slack) && slack <= 0.05;" in score
    assert re.search(r"\(items && atoi\(items\) > 0\) \? atoi\(items\) : (\d+),", score).group(1) == str(sc.PRUNE_ITEMS)
    geom = open(os.path.join(CSRC, "mvs_prune_search.h")).read()
    assert "static constexpr int TY = 16, TX = 56, H = WIN / 2, PAD = (WIN - 1) / 2;" in geom and "static constexpr int kMinSeg = 8;" in geom
    from tests import helpers
    import inspect

    assert "2e-5 * max(abs(s), 1e-3)" in inspect.getsource(helpers._check_scores) and (sc.SCORE_RTOL, sc.SCORE_FLOOR) == (2e-5, 1e-3)


def test_the_table_holds_every_listed_case():
    assert [c.name for c in sc.ERROR_CASES] == ["bright_flat", "near_saturated", "mid_texture", "sparse_blob", "workload_segment", "one_segment"]
    assert [c.name for c in sc.TIE_CASES] == ["tie_first_wins", "tie_second_wins", "tie_bright_flat"]
    shapes = {c.name: sc.crops(c.name)[0].shape for c in sc.CASES}
    assert shapes["workload_segment"] == (57, 262, 286) and shapes["one_segment"] == (30, 374, 398)
    assert all(shapes[n] == (40, 96, 120) for n in shapes if n not in ("workload_segment", "one_segment"))
    for c in sc.ERROR_CASES:
        assert 4 <= len(c.candidates) <= (5 if np.prod(shapes[c.name]) > 1e6 else 8)
        whole = [all(float(v).is_integer() for v in t) for t in c.candidates]
        assert any(whole) and not all(whole), c.candidates          # integer and half-voxel shifts
    for name in ("tie_first_wins", "tie_second_wins"):
        assert sc.by_name(name).candidates == [(0, 0, 0), (0, 0, -1), (0, 0, 0.5), (0, 0, 1), (1, 0, 0)]
    assert sorted(sc.TIE_PAIRS) == ["pair_bright_flat", "pair_first_wins", "pair_second_wins"]


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_case_is_scored_on_the_seven_wide_window_by_the_pruned_search(case):
    im0, im1 = sc.crops(case.name)
    assert im0.dtype == im1.dtype == np.float32 and im0.ndim == 3 and im0.shape == im1.shape
    assert np.isfinite(im0).all() and np.isfinite(im1).all()
    assert im0.min() == im1.min() == 0.0 and im0.max() == im1.max() == 1.0
    codes, ssim, _ = sc.oracle(case.name)
    assert (codes == 0).all() and np.isfinite(ssim).all() and (ssim > -1).all(), (codes, ssim)
    # finite crops under "union": the region of every candidate is the whole volume, its window min(7, shortest axis made odd)
    assert min(im0.shape) >= 7
    assert len(set(case.candidates)) == len(case.candidates)
    # the pruned path: two or more candidates, slack = 1e-2 max(1, (value_bound / data_range)^2) <= 0.05
    data_range, im1_min, value_bound = sc.scoring_args(im0, im1)
    assert len(case.candidates) >= 2 and data_range == 1.0 and im1_min == 0.0
    assert sc.SLACK * max(1.0, (value_bound / data_range) ** 2) == sc.SLACK <= 0.05
    # float32 data and buffers of the walk: the volume in bytes stays below 2^31
    assert im0.size * 4 < 2 ** 31
    tiles, nzs, zseg = sc.walk_geometry(im0.shape)
    assert zseg == case.zseg, (tiles, nzs, zseg)


def test_walk_geometry_of_the_two_large_cases():
    assert sc.walk_geometry((57, 262, 286)) == (80, 4, 13)
    assert sc.walk_geometry((30, 374, 398)) == (161, 1, 24)
    assert sc.walk_geometry((40, 96, 120)) == (18, 5, 7)
    assert sc.walk_geometry((51, 256, 256)) == (16 * 5, 4, 12)


@pytest.mark.parametrize("case", sc.ERROR_CASES, ids=lambda c: c.name)
def test_error_case_keeps_candidates_close_to_the_best(case):
    """The float32 error can only be measured on candidates the search completes: a candidate with mean m against the best b is
    completed when its bound is predicted to hold for 3/4 of the volume -- (1 + slack - b) / (1 + slack - m) * 1.15 >= 3/4 if its
    mean is what it is everywhere.  Three or more candidates of every case are well inside that (>= 0.8 without the factor)."""
    _, ssim, _ = sc.oracle(case.name)
    keep = (1.0 + sc.SLACK - ssim.max()) / (1.0 + sc.SLACK - ssim)
    assert (keep >= 0.8).sum() >= 3, keep


@pytest.mark.parametrize("case", sc.TIE_CASES, ids=lambda c: c.name)
def test_near_tie_has_two_candidates_inside_the_margin_and_the_rest_outside(case):
    _, ssim, _ = sc.oracle(case.name)
    order = np.argsort(-ssim)
    gap = ssim[order[0]] - ssim[order[1]]
    # 10 times the 2e-5 bar of the score tests, and below the margin of the float32 walk
    assert 2e-4 <= gap <= 8e-4 < sc.MARGIN, gap
    assert ssim[order[0]] - ssim[order[2]] > 2e-3, ssim
    assert sorted(order[:2].tolist()) == [0, 1]


def test_the_winner_flips_between_the_first_two_near_ties():
    assert int(np.argmax(sc.oracle("tie_first_wins")[1])) == 0 and int(np.argmax(sc.oracle("tie_second_wins")[1])) == 1


@pytest.mark.parametrize("name", sorted(sc.TIE_PAIRS))
def test_near_tie_pair_is_enumerated_by_the_reference(name):
    """The whole registration of the pair: the phase correlation finds one of the two copies, the enumeration (+-estimate) holds both
    candidates of the near tie, they are the two best, inside the margin, and every other candidate fails the 10 % test."""
    a, b, want = sc.tie_pair(name)
    dbg = want["debug"]
    assert dbg["region_mode"] == "union" and np.isfinite(a).all() and np.isfinite(b).all()
    listed = [tuple(t) for t in dbg["t_candidates"].tolist()]
    assert 2 not in dbg["codes"]                    # the metric lists are aligned with the candidate list
    ssim = {t: s for t, s, c in zip(listed, dbg["ssim"], dbg["codes"]) if c == 0}
    assert sorted(ssim) == sorted(sc.PAIR_NEAR_TIE), ssim
    gap = abs(ssim[sc.PAIR_NEAR_TIE[0]] - ssim[sc.PAIR_NEAR_TIE[1]])
    assert 2e-4 <= gap <= 8e-4 < sc.MARGIN, gap
    assert tuple(want["affine_matrix"][:3, 3]) == max(ssim, key=ssim.get)
    first = ssim[sc.PAIR_NEAR_TIE[0]] > ssim[sc.PAIR_NEAR_TIE[1]]
    assert first == (name != "pair_second_wins")
