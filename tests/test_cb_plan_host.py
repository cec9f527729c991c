"""CPU: the plan of a content-based chunk (csrc/mvs_cb_plan.h) compiled for the host.  The drivers of mvs_gauss.hip take every
decision that does not need the device from it -- the views' boxes and pool offsets, the lines a workgroup stages and the LDS
bytes its launch asks for, which path a chunk takes, where the sections of the scratch block lie, and for every line pass
which buffer it reads and writes and which workgroups belong to which view.  A wrong buffer index or block range corrupts
weights silently, so tests/native/cb_plan_host_test.cpp checks them as properties: see its header for the lines it prints."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GROUPS = ["boxes", "decisions", "fast_schedule", "layouts", "lines", "lines_geometry", "pair_schedule"]
# every len in 1..9000 x 6 radii x 2 axis kinds x (4 rules x 3 properties + the 2 specified decisions)
N_LINES = 9000 * 6 * 2 * (4 * 3 + 2)
PROPERTIES = [
    "T_power_of_two_in_range", "T_launch_within_64k", "T_zero_iff_smallest_does_not_fit", "pair_T_is_the_specified_decision",
    "split_T_is_the_specified_decision",
    "box_offset_multiple_of_64", "box_ranges_disjoint_in_view_order", "empty_box_is_zero_and_takes_no_pool", "box_is_the_reach",
    "row_and_table_running_sums", "pool_totals", "pool_verdict_flips_at_2_31",
    "section_starts_on_256", "sections_in_order_and_disjoint", "request_covers_the_sections", "request_not_below_the_specified_size",
    "temporaries_hold_the_largest_box", "uploaded_block_is_contiguous",
    "pair_two_filters_of_ndim_passes", "pair_filter_and_axis_order", "pair_reads_what_the_previous_pass_wrote",
    "pair_first_pass_reads_the_prepared_view", "pair_second_filter_reads_the_squared_deviation", "pair_last_pass_writes_F",
    "pair_middle_passes_hand_both_on", "pair_writes_no_buffer_it_reads", "pair_only_yz_passes_that_hand_both_on_are_split", "pair_launch_bytes",
    "fast_accepts_the_boxes", "fast_two_filters_of_ndim_passes", "fast_pass_0_reads_I", "fast_reads_what_the_previous_pass_wrote",
    "fast_writes_no_pool_it_reads", "fast_last_pass_writes_F", "fast_kinds", "fast_case_has_a_view_wholly_in_the_halo",
    "fast_view_outside_the_trimmed_chunk_has_no_blocks", "fast_last_pass_rows_are_the_trimmed_box", "fast_other_passes_take_the_whole_box",
    "fast_blocks_tile_the_launch_in_view_order", "fast_launch_bytes_are_the_views_maximum",
    "decline_view_count", "decline_matrix", "decline_short_axis", "decline_radius", "decline_line", "decline_pool", "exact_decisions",
    "lines_cover_the_box_once",
]


def test_content_based_chunk_plan_holds_its_properties(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "cb_plan_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "cb_plan_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"

    checked = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("C ")}
    assert sorted(checked) == GROUPS
    assert checked["lines"] == N_LINES
    assert all(n > 0 for n in checked.values())
    wrong = {ln.split()[1]: (int(ln.split()[2]), " ".join(ln.split()[3:])) for ln in lines if ln.startswith("W ")}
    assert sorted(wrong) == sorted(PROPERTIES)          # every property was reached
    for what, (n, first) in wrong.items():
        assert n == 0, f"{what}: {n} cases wrong, the first at {first}"
