"""The preconditions of the thin-overlap cases (tests/thin_overlap_cases.py), checked with the oracle alone: every case reaches the
SSIM window it is built for -- no case drifts back onto the 7-wide path -- and every end-to-end case has a winner that float32
rounding cannot change.  A case that fails here gets another seed or shift; it is never skipped or dropped."""
import warnings

import numpy as np
import pytest
from scipy import ndimage

from oracle import reg_oracle as ro
from tests import thin_overlap_cases as tc


def _oracle_windows(case):
    """Per candidate: (oracle code, SSIM window of the region slice under the case's region mode -- 0 below 3 --, oracle SSIM)."""
    a, b = tc.crops(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        im0, im1 = ro.rescale_intensity_01(a), ro.rescale_intensity_01(b)
        im0nm = np.isnan(im0)
        data_range = np.nanmax([im0, im1]) - np.nanmin([im0, im1])
        im1_min = np.nanmin(im1)
        valid1 = np.sum(~np.isnan(im1))
        bb0 = ro.get_bb_from_nanmask(~im0nm)
        out = []
        for t in tc.candidates(case):
            code, ssim, _ = ro.score_candidate(im0, im1, im0nm, t, valid1, case.region_mode, data_range, im1_min, bb0)
            win = None
            if code == 0:
                im1t = ndimage.affine_transform(im1, ro.affine_from_translation(list(t)), order=1, mode="constant", cval=np.nan)
                bb1 = ro.get_bb_from_nanmask(~np.isnan(im1t))
                if case.region_mode == "union":
                    ext = [max(bb0[d][1], bb1[d][1]) + 1 - min(bb0[d][0], bb1[d][0]) for d in range(a.ndim)]
                else:
                    ext = [min(bb0[d][1], bb1[d][1]) + 1 - max(bb0[d][0], bb1[d][0]) for d in range(a.ndim)]
                m = min(ext)
                win = int(min(7, m - ((m - 1) % 2)))
                win = win if win >= 3 else 0
            out.append((code, win, ssim))
    return out


def test_the_table_holds_every_listed_case():
    names = [c.name for c in tc.SCORE_CASES]
    assert len(set(names)) == len(names)
    finite = {g: [c.shape for c in tc.SCORE_CASES if c.group == g] for g in "abd"}
    assert finite["a"] == [(6, 48, 40), (5, 48, 40), (4, 48, 40), (3, 48, 40), (2, 48, 40), (1, 48, 40), (40, 5, 48), (40, 4, 48),
                           (40, 48, 5), (40, 48, 4)]
    assert finite["b"] == [(5, 64), (6, 64), (64, 4), (3, 50), (2, 50), (6, 6)]
    assert finite["d"] == [(7, 48, 40), (8, 48, 40), (48, 7, 40), (48, 40, 8), (7, 7, 7), (8, 9, 7)]
    bands = [(c.shape, c.nan_band, c.region_mode) for c in tc.SCORE_CASES if c.group == "c"]
    want = [((24, 40, 36), (0, 9, 7)), ((24, 40, 36), (1, 17, 5)), ((24, 40, 36), (2, 20, 7)), ((24, 40, 36), (0, 3, 3)),
            ((24, 40, 36), (2, 30, 2)), ((40, 90), (0, 11, 5)), ((40, 90), (1, 0, 7)), ((40, 90), (1, 50, 3))]
    assert bands == [(s, b, m) for s, b in want for m in ("intersection", "union")]
    assert [c.shape for c in tc.E2E_CASES] == [(6, 48, 40), (5, 48, 40), (4, 48, 40), (3, 48, 40), (2, 48, 40), (1, 48, 40), (40, 5, 48),
                                               (40, 48, 4), (7, 48, 40), (8, 48, 40), (7, 7, 7), (5, 64), (64, 4), (3, 50), (2, 50), (6, 6)]
    for shape in tc.SWITCH_SHAPES + tc.INTEGER_HALF_SHAPES:
        tc.by_shape(tc.E2E_CASES, shape)
    assert [c.shape for c in tc.INTEGER_WHOLE_CASES] == tc.INTEGER_SHAPES


@pytest.mark.parametrize("case", tc.SCORE_CASES, ids=lambda c: c.name)
def test_score_case_reaches_its_window(case):
    cands = tc.candidates(case)
    res = _oracle_windows(case)
    intended = case.window if isinstance(case.window, tuple) else (case.window,) * len(cands)
    assert len(intended) == len(cands)
    alive = [i for i, (code, _, _) in enumerate(res) if code == 0]
    assert len(alive) >= 2, res
    assert [code for code, _, _ in res].count(1) >= 1, res          # the candidate that fails the 10 % test
    for i in alive:
        assert res[i][1] == intended[i], (i, cands[i], res[i], intended[i])
        if res[i][1] == 0:
            assert res[i][2] == -1
    if case.group == "c" and case.region_mode == "union":
        assert all(res[i][1] == 7 for i in alive)
    targets = {intended[i] for i in alive}
    if targets & {5, 3}:
        whole = [all(float(v).is_integer() for v in cands[i]) for i in alive]
        assert any(whole) and not all(whole), (cands, alive)


_E2E = ([(c, False) for c in tc.E2E_CASES] + [(c, True) for c in tc.INTEGER_WHOLE_CASES]
        + [(tc.by_shape(tc.E2E_CASES, s), True) for s in tc.INTEGER_HALF_SHAPES])


@pytest.mark.parametrize("case,integer", _E2E, ids=lambda v: v.name if hasattr(v, "name") else ("integer" if v else "float"))
def test_end_to_end_case_has_a_clear_winner(case, integer):
    a, b = tc.integer_crops(case) if integer else tc.crops(case)
    dbg = ro.phase_correlation_registration(a, b, return_debug=True)["debug"]
    vals = sorted(set(float(v) for v in dbg["ssim"]), reverse=True)
    assert dbg["region_mode"] == "union" and dbg["codes"].count(0) >= 2
    if case.all_minus_one:
        assert vals == [-1.0]        # the first listed candidate wins by nanargmax
        assert dbg["argmax_index"] == 0
    else:
        # 50 times the per-value bar of the score tests, and the margin of the float32 walk (kPruneMarginF32)
        assert vals[0] > -1 and vals[0] - vals[1] >= 1e-3, vals[:3]


@pytest.mark.parametrize("case", tc.INTEGER_WHOLE_CASES, ids=lambda c: c.name)
def test_integer_case_with_equal_rank_vectors_has_a_whole_pixel_winner(case):
    """Float sorts and key histograms rank the same values only when the winning shift interpolates nothing."""
    a, b = tc.integer_crops(case)
    t = ro.phase_correlation_registration(a, b)["affine_matrix"][:-1, -1]
    assert np.all(t == np.floor(t)) and np.any(t != 0), t


@pytest.mark.parametrize("shape", tc.INTEGER_HALF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_case_with_a_half_pixel_winner_and_its_exact_reference(shape):
    """The winner interpolates along the thin axis; the rank correlation of the exact tap sums stays within the end-to-end bar of
    the oracle's (measured: 3.6e-6 for 5x48x40, 5.1e-8 for 3x48x40), so both are fair references for the histogram route."""
    a, b = tc.integer_crops(tc.by_shape(tc.E2E_CASES, shape))
    want = ro.phase_correlation_registration(a, b)
    t = want["affine_matrix"][:-1, -1]
    assert np.all(t * 2 == np.floor(t * 2)) and t[0] != np.floor(t[0]), t
    assert abs(tc.exact_key_spearman(a, b, t) - want["quality"]) <= 1e-5
