"""The float32 SSIM walk of the pruned arg-max search and its float64 re-walk (csrc/mvs_score.hip: ssim_fused_batch_f32_kernel<7>,
ssim_fused_batch_kernel<7>; csrc/mvs_prune_search.h) against the oracle, through mvs_score_candidates_argmax -- the launches of
mvs_register_crops, with the search's per-candidate state handed out -- on the cases of tests/ssim_walk_cases.py.

The search reproduces the reference's nanargmax if the float32 mean SSIM of every candidate is within kPruneMarginF32 / 2 of its
float64 value: a candidate is dropped only when its bound is below best - margin, a complete candidate is left un-rewalked only when
it is margin below the best, and the final arg max compares float64 sums of re-walked candidates with float32 sums of the others.
That half margin is the bar of the error test; it is the search's own requirement, not a measured number."""
import numpy as np
import pytest

from tests import ssim_walk_cases as sc

pytestmark = pytest.mark.gpu

COUNTERS = ("reg_rewalks", "reg_cand_volumes", "reg_pruned")


def _fmt(values):
    return " ".join("%+.2e" % v for v in values)


def _search(name, candidates=None):
    """The case through mvs_score_candidates_argmax with the context's options as they stand: a dict of the per-candidate arrays
    and of what the call added to the counters."""
    from multiview_stitcher_amd import _lib, _reg_ops

    im0, im1 = sc.crops(name)
    data_range, im1_min, value_bound = sc.scoring_args(im0, im1)
    for key in COUNTERS:
        _lib.get_counter(key, reset=True)
    cands = sc.by_name(name).candidates if candidates is None else candidates
    ssim, spear, code, rounds, state = _reg_ops.score_candidates_argmax(im0, im1, cands, "union", data_range, im1_min, value_bound)
    res = {"ssim": ssim, "spear": spear, "code": code, "rounds": rounds, "state": state}
    res.update({key: _lib.get_counter(key, reset=True) for key in COUNTERS})
    return res


def _bits(state):
    from multiview_stitcher_amd import _lib

    return ((state & _lib.MVS_SCORE_COMPLETE) != 0, (state & _lib.MVS_SCORE_DROPPED) != 0, (state & _lib.MVS_SCORE_REWALKED) != 0)


def _within_score_bar(got, want):
    return np.abs(got - want) <= sc.SCORE_RTOL * np.maximum(np.abs(want), sc.SCORE_FLOOR)


def _check_states(res, want):
    """What holds for every case: every candidate scored, and ends complete or dropped, never both; a re-walked candidate is a complete
    one; nothing above 1 + slack; dropped candidates are truly out."""
    complete, dropped, rewalked = _bits(res["state"])
    assert (res["code"] == 0).all()
    assert (complete ^ dropped).all() and not (rewalked & ~complete).any(), res["state"]
    assert np.isnan(res["rounds"][~complete]).all() and np.isfinite(res["rounds"][complete]).all()
    assert (res["rounds"][complete] <= 1.0 + sc.SLACK).all() and (res["ssim"] <= 1.0 + sc.SLACK).all()
    assert res["reg_pruned"] == dropped.sum() and res["reg_rewalks"] == rewalked.sum()
    # a dropped candidate is below the oracle's best by more than half the margin, and the bound it is reported with holds for its
    # oracle value up to half the margin
    assert (want[dropped] < want.max() - sc.MARGIN / 2).all(), (want, res["state"])
    assert (res["ssim"][dropped] >= want[dropped] - sc.MARGIN / 2).all(), (res["ssim"], want)
    assert (res["ssim"][dropped] < np.max(res["rounds"][complete])).all()
    return complete, dropped, rewalked


@pytest.mark.parametrize("case", sc.ERROR_CASES, ids=lambda c: c.name)
def test_float32_rounds_stay_within_half_the_margin_of_the_oracle(hip_device, case):
    """Every complete candidate: |mean SSIM of the float32 rounds - oracle| <= kPruneMarginF32 / 2.  Measured (MI355X), worst signed
    deviation per case, in units of margin / 2: see DESIGN.md 3.3."""
    _, want, _ = sc.oracle(case.name)
    res = _search(case.name)
    complete, dropped, rewalked = _check_states(res, want)
    dev = res["rounds"] - want
    worst = dev[complete][np.argmax(np.abs(dev[complete]))]
    print(f"\nssim_f32_walk {case.name}: shape {sc.crops(case.name)[0].shape} zseg {case.zseg} complete {int(complete.sum())}/{len(want)} "
          f"dropped {int(dropped.sum())} rewalked {int(rewalked.sum())} worst signed deviation {worst:+.3e} = {worst / (sc.MARGIN / 2):+.3f} (margin / 2) "
          f"all {_fmt(dev)}")
    assert complete.sum() >= 3, res["state"]          # otherwise the case is wrong (tests/test_ssim_walk_cases_host.py)
    assert (np.abs(dev[complete]) <= sc.MARGIN / 2).all(), dev
    # the float64 walk at the same shapes: candidates that were walked again are at the bar of the score tests
    assert _within_score_bar(res["ssim"][rewalked], want[rewalked]).all(), (res["ssim"], want)
    assert (res["ssim"][complete & ~rewalked] == res["rounds"][complete & ~rewalked]).all()
    assert int(np.argmax(res["ssim"])) == int(np.argmax(want))


@pytest.mark.parametrize("case", sc.TIE_CASES, ids=lambda c: c.name)
def test_near_ties_are_decided_by_the_float64_rewalk(hip_device, case):
    _, want, want_q = sc.oracle(case.name)
    res = _search(case.name)
    complete, dropped, rewalked = _check_states(res, want)
    rounds = res["rounds"]
    dev = rounds - want
    print(f"\nssim_f32_walk {case.name}: state {res['state']} rounds - oracle {_fmt(dev)} "
          f"final - oracle {_fmt(res['ssim'] - want)} volumes {res['reg_cand_volumes']:.4f}")
    best = np.max(rounds[complete])
    near = complete & (np.nan_to_num(rounds, nan=-np.inf) >= best - sc.MARGIN)
    assert near.sum() >= 2 and (rewalked == near).all(), (res["state"], rounds)
    assert res["reg_rewalks"] == near.sum()
    # one candidate volume per re-walk on top of the rounds: complete candidates count 1, dropped ones a fraction in (0, 1)
    rounds_volumes = res["reg_cand_volumes"] - near.sum()
    assert complete.sum() <= rounds_volumes <= complete.sum() + dropped.sum() and (rounds_volumes > complete.sum()) == bool(dropped.any())
    assert _within_score_bar(res["ssim"][rewalked], want[rewalked]).all(), (res["ssim"], want)
    assert int(np.argmax(res["ssim"])) == int(np.argmax(want))
    keep = complete & ~rewalked
    assert (res["ssim"][keep] == rounds[keep]).all()
    assert (np.abs(dev[complete]) <= sc.MARGIN / 2).all(), dev
    # the rank correlation of the winner, and of no one else
    w = int(np.argmax(want))
    assert abs(res["spear"][w] - want_q[w]) <= 1e-5 and np.isnan(np.delete(res["spear"], w)).all()
    # the two candidates of the tie alone: both complete, both walked again -- 2 + 2 candidate volumes exactly
    two = _search(case.name, [case.candidates[i] for i in np.flatnonzero(near)[:2]])
    assert (two["state"] == 5).all() and two["reg_rewalks"] == 2 and two["reg_cand_volumes"] == 4.0
    # (the same walks in a launch of another width: equal up to the order of the partial sums)
    np.testing.assert_allclose(two["ssim"], res["ssim"][np.flatnonzero(near)[:2]], rtol=1e-12)
    np.testing.assert_allclose(two["rounds"], rounds[np.flatnonzero(near)[:2]], rtol=1e-12)


@pytest.mark.parametrize("case", sc.TIE_CASES, ids=lambda c: c.name)
def test_near_ties_under_the_switches_of_the_search(hip_device, case):
    from multiview_stitcher_amd import _lib

    _, want, _ = sc.oracle(case.name)
    default = _search(case.name)
    # float64 rounds: no margin, no re-walk
    _lib.set_option("ssim_f32", 0)
    try:
        res = _search(case.name)
    finally:
        _lib.set_option("ssim_f32", 1)
    complete, dropped, rewalked = _check_states(res, want)
    assert not rewalked.any() and res["reg_rewalks"] == 0
    assert complete.sum() >= 2 and _within_score_bar(res["ssim"][complete], want[complete]).all(), (res["ssim"], want)
    assert (res["rounds"][complete] == res["ssim"][complete]).all()
    assert int(np.argmax(res["ssim"])) == int(np.argmax(want)) == int(np.argmax(default["ssim"]))
    # the two kernels hand over: what the float64 rounds end with is what the float64 re-walk of the default search ends with,
    # up to the order in which the partial sums of the rounds were added
    _, _, again = _bits(default["state"])
    np.testing.assert_allclose(default["ssim"][again & complete], res["ssim"][again & complete], rtol=1e-9)
    # no search: every candidate in full by one float64 walk, reported as not pruned
    _lib.set_option("ssim_prune", 0)
    try:
        res = _search(case.name)
    finally:
        _lib.set_option("ssim_prune", 1)
    assert (res["state"] == _lib.MVS_SCORE_COMPLETE).all() and (res["rounds"] == res["ssim"]).all()
    assert res["reg_rewalks"] == 0 and res["reg_pruned"] == 0 and res["reg_cand_volumes"] == len(want)
    assert _within_score_bar(res["ssim"], want).all(), (res["ssim"], want)
    assert int(np.argmax(res["ssim"])) == int(np.argmax(want))


@pytest.mark.parametrize("name", sorted(sc.TIE_PAIRS))
def test_register_crops_decides_a_near_tie_like_the_oracle_under_every_switch(hip_device, name):
    """The product path on a pair whose enumerated candidates hold a near tie: translation, quality and status do not depend on
    the switches of the search and are the oracle's; by default the tie goes through the re-walk."""
    from multiview_stitcher_amd import _lib, _reg_ops

    a, b, want = sc.tie_pair(name)
    res = {}
    rewalks = {}
    for f32 in (1, 0):
        for prune in (1, 0):
            _lib.set_option("ssim_f32", f32)
            _lib.set_option("ssim_prune", prune)
            try:
                _lib.get_counter("reg_rewalks", reset=True)
                res[f32, prune] = _reg_ops.register_crops(a, b, 2)
                rewalks[f32, prune] = _lib.get_counter("reg_rewalks", reset=True)
            finally:
                _lib.set_option("ssim_f32", 1)
                _lib.set_option("ssim_prune", 1)
    t, quality, status, n_candidates = res[1, 1]
    for key, (t2, q2, s2, n2) in res.items():
        assert np.array_equal(t2, t) and q2 == quality and (s2, n2) == (status, n_candidates), (key, res[key], res[1, 1])
    assert status == 0 and n_candidates == len(want["debug"]["t_candidates"])
    np.testing.assert_array_equal(t, want["affine_matrix"][:-1, -1])
    assert abs(quality - want["quality"]) <= 1e-5
    assert rewalks[1, 1] >= 2 and rewalks[0, 1] == rewalks[1, 0] == rewalks[0, 0] == 0, rewalks


def test_the_search_is_deterministic_on_a_near_tie(hip_device):
    first, second = _search("tie_first_wins"), _search("tie_first_wins")
    for key in ("ssim", "rounds", "state", "spear", "code"):
        assert first[key].tobytes() == second[key].tobytes(), key
    assert all(first[key] == second[key] for key in COUNTERS)


def test_the_entry_point_refuses_missing_state_arrays(hip_device):
    import ctypes as C

    from multiview_stitcher_amd import _lib

    lib = _lib.init(0)
    im0, im1 = sc.crops("tie_first_wins")
    t = np.zeros((1, 3))
    out = np.zeros(1)
    code = np.zeros(1, np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = lib.mvs_score_candidates_argmax(0, im0.ctypes.data, im1.ctypes.data, _lib.MVS_MEM_HOST, 3, _lib.i64x3(im0.shape), t.ctypes.data_as(dp), 1, 0,
                                         1.0, 0.0, 1.0, out.ctypes.data_as(dp), out.ctypes.data_as(dp), code.ctypes.data_as(ip), None, None)
    assert rc == -1 and b"mvs_score_candidates_argmax" in lib.mvs_last_error(0)
