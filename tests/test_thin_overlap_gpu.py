"""GPU parity of candidate scoring on thin overlaps (tests/thin_overlap_cases.py): the SSIM windows 5 and 3 -- launch_ssim_passes<5>
and <3> of csrc/mvs_score.hip with their first-pass, fused y/x and last-pass kernels --, the "no SSIM" result below 3, and the lower
edge of the 7-wide fast path (shared fixed-image terms, batched fused walk, pruned arg-max search on a cropped interior 1 or 2
voxels thick), against oracle/reg_oracle.py.  tests/test_thin_overlap_host.py checks that every case reaches the path it names."""
import numpy as np
import pytest

from oracle import reg_oracle as ro
from tests import thin_overlap_cases as tc
from tests.helpers import _check_scores

pytestmark = pytest.mark.gpu

ROUTES = ("hist", "sort16", "sort32")


# ---- score level: codes, SSIM (2e-5 * max(|s|, 1e-3)) and Spearman (1e-5) of every candidate against the oracle; the materialised
# copies (quality_for_all) and the on-the-fly / batched paths bit-equal ----

@pytest.mark.parametrize("case", tc.SCORE_CASES, ids=lambda c: c.name)
def test_score_candidates_on_thin_regions(hip_device, case):
    a, b = tc.crops(case)
    _check_scores(a, b, tc.candidates(case), case.region_mode)


@pytest.mark.parametrize("case", [c for c in tc.SCORE_CASES if c.window == 0], ids=lambda c: c.name)
def test_no_ssim_below_three_gives_minus_one_and_the_oracle_quality(hip_device, case):
    """A region thinner than 3: code 0, SSIM exactly -1.0 and the oracle's Spearman coefficient for every candidate that passes the
    mask test, from both forms of the call."""
    from multiview_stitcher_amd import _reg_ops

    a, b = tc.crops(case)
    cands = tc.candidates(case)
    im0, im1 = ro.rescale_intensity_01(a), ro.rescale_intensity_01(b)
    im0nm = np.isnan(im0)
    data_range = np.nanmax([im0, im1]) - np.nanmin([im0, im1])
    im1_min = np.nanmin(im1)
    want = [ro.score_candidate(im0, im1, im0nm, t, np.sum(~np.isnan(im1)), case.region_mode, data_range, im1_min,
                               ro.get_bb_from_nanmask(~im0nm)) for t in cands]
    assert [w[0] for w in want].count(0) >= 2
    for for_all in (True, False):     # (all surviving candidates tie at -1: the rank correlation is evaluated for each of them)
        ssim, spear, codes = _reg_ops.score_candidates(im0, im1, cands, case.region_mode, data_range, im1_min, quality_for_all=for_all)
        for i, (code, s, q) in enumerate(want):
            assert codes[i] == code
            if code == 0:
                assert s == -1 and ssim[i] == -1.0
                assert abs(spear[i] - q) <= 1e-5, (i, spear[i], q)


@pytest.mark.parametrize("case", [c for c in tc.SCORE_CASES if c.group == "d"], ids=lambda c: c.name)
def test_fast_path_edge_on_the_separate_batch_launches(hip_device, case):
    """The same cases with the batched fused walk replaced by the batched z launch + y/x launch (option "ssim_two_pass")."""
    from multiview_stitcher_amd import _lib

    a, b = tc.crops(case)
    _lib.set_option("ssim_two_pass", 1)
    try:
        _check_scores(a, b, tc.candidates(case), case.region_mode)
    finally:
        _lib.set_option("ssim_two_pass", 0)


# ---- end to end: mvs_register_crops and the Python mirror against the oracle's phase_correlation_registration ----

_WANT = {}


def _oracle(case):
    """One oracle run per case, shared by the tests below (never modified)."""
    if case.name not in _WANT:
        a, b = tc.crops(case)
        _WANT[case.name] = (a, b, ro.phase_correlation_registration(a, b, return_debug=True))
    return _WANT[case.name]


@pytest.mark.parametrize("case", tc.E2E_CASES, ids=lambda c: c.name)
def test_registration_of_thin_crops_matches_oracle(hip_device, case):
    from multiview_stitcher_amd import _reg_ops, registration

    a, b, want = _oracle(case)
    up = 10 if a.ndim == 2 else 2
    mirror = registration.phase_correlation_registration(a, b, return_debug=True)
    np.testing.assert_array_equal(mirror["debug"]["t_candidates"], want["debug"]["t_candidates"])
    assert mirror["debug"]["codes"] == want["debug"]["codes"]
    np.testing.assert_array_equal(mirror["affine_matrix"], want["affine_matrix"])
    assert abs(mirror["quality"] - want["quality"]) <= 1e-5
    t, q, status, n_cand = _reg_ops.register_crops(a, b, up)
    assert status == 0 and n_cand == len(want["debug"]["t_candidates"])
    np.testing.assert_array_equal(t, want["affine_matrix"][:-1, -1])
    assert abs(q - want["quality"]) <= 1e-5
    if case.all_minus_one:
        assert set(want["debug"]["ssim"]) == {-1}


@pytest.mark.parametrize("shape", tc.SWITCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_search_switches_change_nothing_on_thin_crops(hip_device, shape):
    """The pruned arg-max search off ("ssim_prune" = 0), every shortcut for finite crops off ("materialize_shifts" = 1) and the
    defaults: one translation; quality equal (float crops take the same rank route in all three)."""
    from multiview_stitcher_amd import _lib, _reg_ops

    case = tc.by_shape(tc.E2E_CASES, shape)
    a, b, want = _oracle(case)
    counters = ("reg_pruned", "reg_candidates")
    for key in counters:
        _lib.get_counter(key, reset=True)
    default = _reg_ops.register_crops(a, b, 2)
    stats = {key: _lib.get_counter(key, reset=True) for key in counters}
    _lib.set_option("ssim_prune", 0)
    try:
        unpruned = _reg_ops.register_crops(a, b, 2)
    finally:
        _lib.set_option("ssim_prune", 1)
    _lib.set_option("materialize_shifts", 1)
    try:
        plain = _reg_ops.register_crops(a, b, 2)
    finally:
        _lib.set_option("materialize_shifts", 0)
    for res in (default, unpruned, plain):
        np.testing.assert_array_equal(res[0], want["affine_matrix"][:-1, -1])
        assert res[2:] == (0, len(want["debug"]["t_candidates"]))
    assert unpruned[1] == default[1]
    assert plain[1] == default[1]
    assert abs(default[1] - want["quality"]) <= 1e-5
    if shape == (7, 48, 40):
        # 3 walk items (one z segment, one row of 3 y tiles) against the 32 residue classes of the search
        assert stats["reg_candidates"] >= 2 and 0 <= stats["reg_pruned"] < stats["reg_candidates"], stats


@pytest.mark.parametrize("case", tc.INTEGER_WHOLE_CASES, ids=lambda c: c.name)
def test_device_resident_integer_thin_crops(hip_device, case):
    """Integer-valued finite crops with a whole-pixel winner: host arrays are ranked by float sorts ("reg_rank_sort32"), the same
    pair on the device by key histograms ("reg_rank_hist") -- the same translation, the same rank vectors, sums taken in a
    different order."""
    from multiview_stitcher_amd import _lib, _reg_ops
    from multiview_stitcher_amd.device import DeviceArray

    a, b = tc.integer_crops(case)
    for r in ROUTES:
        _lib.get_counter("reg_rank_" + r, reset=True)
    t, q, status, n_cand = _reg_ops.register_crops(a, b, 2)
    assert [_lib.get_counter("reg_rank_" + r, reset=True) for r in ROUTES] == [0.0, 0.0, 1.0]
    td, qd, status_d, n_cand_d = _reg_ops.register_crops(DeviceArray.from_host(a), DeviceArray.from_host(b), 2)
    taken = [_lib.get_counter("reg_rank_" + r, reset=True) for r in ROUTES]
    assert taken == [1.0, 0.0, 0.0], taken
    assert status == status_d == 0 and n_cand == n_cand_d
    np.testing.assert_array_equal(td, t)
    assert qd == pytest.approx(q, rel=1e-10)
    want = ro.phase_correlation_registration(a, b)
    np.testing.assert_array_equal(t, want["affine_matrix"][:-1, -1])
    assert abs(q - want["quality"]) < 1e-6


@pytest.mark.parametrize("shape", tc.INTEGER_HALF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_resident_integer_thin_crops_with_a_half_pixel_winner(hip_device, shape):
    """The same crops under the shifts of the end-to-end table: the winner is a half-pixel shift along the thin axis.  The host run
    ranks the float32 interpolated values like the oracle (equal to 1e-6), the device run ranks the exact tap sums by key
    histograms: the rank correlation of those sums to rel=1e-10, the oracle's within the end-to-end bar of 1e-5.  The two runs do
    NOT agree to rel=1e-10 here -- float32 rounding splits ties that the exact sums keep; measured on the MI355X: 0.934755804780743
    (device) against 0.934759356714978 (host = oracle) for 5x48x40, 0.9308730120774173 against 0.9308730631104712 for 3x48x40."""
    from multiview_stitcher_amd import _lib, _reg_ops
    from multiview_stitcher_amd.device import DeviceArray

    a, b = tc.integer_crops(tc.by_shape(tc.E2E_CASES, shape))
    want = ro.phase_correlation_registration(a, b)
    for r in ROUTES:
        _lib.get_counter("reg_rank_" + r, reset=True)
    t, q, status, n_cand = _reg_ops.register_crops(a, b, 2)
    assert [_lib.get_counter("reg_rank_" + r, reset=True) for r in ROUTES] == [0.0, 0.0, 1.0]
    np.testing.assert_array_equal(t, want["affine_matrix"][:-1, -1])
    assert status == 0 and abs(q - want["quality"]) < 1e-6
    td, qd, status_d, n_cand_d = _reg_ops.register_crops(DeviceArray.from_host(a), DeviceArray.from_host(b), 2)
    taken = [_lib.get_counter("reg_rank_" + r, reset=True) for r in ROUTES]
    assert taken == [1.0, 0.0, 0.0], taken
    assert status_d == 0 and n_cand_d == n_cand
    np.testing.assert_array_equal(td, t)
    assert qd == pytest.approx(tc.exact_key_spearman(a, b, t), rel=1e-10)
    assert abs(qd - want["quality"]) <= 1e-5
