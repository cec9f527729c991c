"""CPU: the plan of the region fuse kernels (csrc/mvs_region_plan.h) compiled for the host.  mvs_fuse_regions takes from it every
decision that does not need the device -- the boxes, which views a box lists, the "unit" / "positive" / "partial" flags that pick
a brick's shortcut in the kernels, the class and the brick width of a box, the item lists of the class kernels and the padded
per-XCD list of option "fuse_mixed".  A wrong flag gives wrong voxels in a few cells only, so
tests/native/region_plan_host_test.cpp checks every one of them by brute force over the voxels of small chunks (registered grids,
rows at the clustering limit, stairs of up to 8 views, pairs at the brick-width limits, random stairs and grids): see its header
for the lines it prints."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# box widths at which the brick width switches: each must have occurred where it decides (32 | 33 on any box, 136 | 137 on an
# overlap, 160 | 161 on a copy-class box)
GROUPS = ["breakpoints", "bricks", "declines", "mixed", "plans", "voxels",
          "width_136", "width_137", "width_160", "width_161", "width_32", "width_33"]
PROPERTIES = [
    "small_chunk_is_accepted", "regions_below_the_padding_id",
    "region_is_a_box_of_the_trimmed_chunk", "regions_tile_the_trimmed_chunk_once", "region_lists_the_views_that_meet_it",
    "view_not_flagged_partial_contains_the_box", "partial_flag_only_on_a_view_that_misses_voxels",
    "unit_bit_means_weight_1_at_every_voxel", "bit_15_means_every_view_full_and_positive", "copy_class_means_one_full_positive_view",
    "class_follows_the_view_count", "brick_width_follows_the_box_width",
    "brick_lies_in_its_region", "every_brick_of_every_region_occurs_once", "brick_counter_excludes_the_padding",
    "class_items_contiguous_and_counted", "class_voxel_counters_are_the_boxes", "no_mixed_list_without_the_option",
    "mixed_padding_items_are_0xffff_inside_the_mixed_list", "mixed_list_holds_classes_4_0_1_only",
    "mixed_classes_not_again_in_the_class_lists", "mixed_eight_stretches_of_one_length_multiple_of_4", "mixed_padding_ends_a_stretch",
    "borders_16_apart_share_a_break_point", "borders_17_apart_do_not", "break_points_sorted_unique_within_the_chunk",
    "x_shell_is_cut_on_the_rim_only",
    "declines_on_a_ninth_view_on_a_cell", "declines_on_more_than_60000_cells",
]


def test_region_plan_holds_its_properties(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "region_plan_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "region_plan_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"

    checked = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("C ")}
    assert sorted(checked) == sorted(GROUPS)
    assert all(n > 0 for n in checked.values())
    wrong = {ln.split()[1]: (int(ln.split()[2]), " ".join(ln.split()[3:])) for ln in lines if ln.startswith("W ")}
    assert sorted(wrong) == sorted(PROPERTIES)          # every property was reached
    for what, (n, first) in wrong.items():
        assert n == 0, f"{what}: {n} cases wrong, the first at {first}"
