"""CPU: csrc/mvs_fuse_chunk_plan.h compiled for the host (tests/native/fuse_chunk_plan_host_test.cpp) -- what the chunk entries of
mvs_fuse.hip decide without the device: the exact in-bounds ranges against an index-by-index walk, the translation-path records and
their refusals, the views the host tests make by hand against the real code, the route through the kernel families against the
conditions the driver evaluated inline before the header existed (kept in the C++ file as the "before" function), the layouts of the
parameter block, the brick grid and the x-weight table, and the chunk boxes of translated and turned views.  Every group prints how
many cases it checked and every property how many were wrong: the counts are asserted, so a sweep cannot shrink unnoticed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# views of the geometries tests/native/tr_view_by_hand.h lists and of the ten more this test draws (a fixed generator: a fixed number)
HAND_VIEWS = 368


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("fuse_chunk_plan") / "fuse_chunk_plan_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "fuse_chunk_plan_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    out = r.stdout.strip().splitlines()
    assert out[-1] == "done"
    return out


def _table(lines, tag):
    return {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith(tag + " ")}


def _wrong(lines, properties):
    """Every property was reached and none of its cases was wrong."""
    rows = {ln.split()[1]: (int(ln.split()[2]), " ".join(ln.split()[3:])) for ln in lines if ln.startswith("W ")}
    for what in properties:
        assert what in rows, f"{what}: never checked"
        n, first = rows[what]
        assert n == 0, f"{what}: {n} cases wrong, the first at {first}"


def test_every_property_belongs_to_a_test(lines):
    reached = sorted(ln.split()[1] for ln in lines if ln.startswith("W "))
    assert reached == sorted(VALID_RANGE + RECORDS + HAND_FIELDS + HAND_WS + ROUTES + LAYOUTS + BOXES)
    assert sorted(_table(lines, "C")) == ["boxes", "hand_views", "layouts", "records", "routes", "valid_range"]


VALID_RANGE = ["range_equals_the_walk", "empty_exactly_when_lo_exceeds_hi"]


def test_valid_range_equals_the_walk(lines):
    """4 slab lengths x 3 chunk lengths x 4 x 4 index shifts x 18 offsets (integers, halves, both neighbours of integers,
    +-(2^20 - 0.25), entirely before / after the chunk), two properties each."""
    cases = 4 * 3 * 4 * 4 * 18
    assert _table(lines, "N")["valid_range_cases"] == cases and _table(lines, "C")["valid_range"] == 2 * cases
    nonempty = _table(lines, "N")["valid_range_nonempty"]
    print("valid range:", cases, "cases,", nonempty, "of them with a voxel in bounds")
    assert cases // 4 < nonempty < cases
    _wrong(lines, VALID_RANGE)


RECORDS = ["plain_view_is_accepted", "io_is_the_whole_part_of_the_offset_plus_the_index_shifts", "fw_is_the_fraction_in_0_1_and_0_at_order_0",
           "fw_does_not_depend_on_the_chunk", "sup_flo_does_not_depend_on_the_chunk", "sup_fhi_does_not_depend_on_the_chunk",
           "sup_k_does_not_depend_on_the_chunk", "ws_does_not_depend_on_the_chunk", "io_shifts_by_d", "sup_ilo_shifts_by_d", "sup_ihi_shifts_by_d",
           "lo_shifts_by_d", "hi_shifts_by_d", "refused", "neighbour_of_a_refusal_is_accepted", "weighted_average_refusal_is_accepted_under_max"]


def test_translation_records(lines):
    """5 views x 2 orders x (accepted + 3 axes x 2); 5 views x 3 shifts of the chunk's origin x (accepted + 5 fields equal + 5 shifted);
    16 refusals (the twelve of prepare_translation_view, both sides where a test has two), 9 accepted neighbours, 5 of the
    weighted-average refusals accepted under max."""
    assert _table(lines, "C")["records"] == 5 * 2 * 7 + 5 * 3 * 11 + 16 + 9 + 5
    _wrong(lines, RECORDS)


HAND_FIELDS = ["hand_view_is_accepted", "hand_view_wnz_linear_n", "hand_view_io", "hand_view_fw", "hand_view_lo_hi", "hand_view_sup_k",
               "hand_view_sup_ilo_ihi", "hand_view_sup_flo_fhi", "hand_view_strides_span"]
HAND_WS = ["hand_view_ws"]


def test_hand_made_views_are_the_real_ones(lines):
    """make_view (tests/native/tr_view_by_hand.h) against prepare_translation_view + fill_tr_view on every view of the region plan
    test's geometries and of ten more: every field make_view sets is bit-equal (``ws``: the next test)."""
    assert _table(lines, "N")["hand_views"] == HAND_VIEWS and _table(lines, "C")["hand_views"] == 10 * HAND_VIEWS
    _wrong(lines, HAND_FIELDS)


def test_hand_made_views_have_the_real_tent_scales(lines):
    """``ws`` too is bit-equal on all 368 views.  prepare_translation_view reads the scales off the support table, from the entries
    next to its centre, and those hold min(ws_k, 2 ws_j for the other axes j): where the spacing gives one scale more than twice
    another (tiles of 72 x 200: (1.825, 5.025)) the table -- and with it the real record -- carries the clipped one (1.825, 3.65).
    make_view clips the same way; most of the geometries have such a view, so the clip is exercised, as are views without it."""
    clipped = _table(lines, "N")["hand_views_with_a_clipped_scale"]
    print("views with a clipped tent scale:", clipped, "of", HAND_VIEWS)
    assert 0 < clipped < HAND_VIEWS
    _wrong(lines, HAND_WS)


ROUTES = ["families_asked_and_the_one_that_fuses", "counters_bumped", "grids_checked_and_launched", "overflow_flag_read", "records_built"]


def test_route_table_equals_the_inline_conditions(lines):
    routes = _table(lines, "R")
    for name, count in sorted(routes.items()):
        print(f"route {name}: {count}")
    # dtypes x orders x fusions x (dct, all tr_ok, force_generic, rows_v1, no_regions) x view counts x rows / regions take x overflow
    total = 3 * 2 * 3 * 2 ** 5 * 3 * 2 * 2 * 2
    assert _table(lines, "N")["route_cases"] == total == sum(routes.values()) and _table(lines, "C")["routes"] == 5 * total
    for name in ("rows", "regions", "column", "generic", "column_generic", "rows_generic"):
        assert routes.get(name, 0) > 0, name
    # nothing else: rows, then regions, then the column kernel (with its redo) -- or the generic kernel alone, or behind the rows only
    asked_first = ("", "rows_", "regions_", "rows_regions_")
    assert set(routes) == ({"rows", "regions", "rows_regions", "generic", "rows_generic"}
                           | {a + c for a in asked_first for c in ("column", "column_generic")})
    _wrong(lines, ROUTES)


LAYOUTS = ["parts_on_256_bytes", "parts_ordered_and_disjoint", "parts_where_the_driver_had_them", "total_is_params_bytes",
           "bricks_cover_the_result_and_none_is_empty", "grid_is_the_drivers", "launch_limit_is_2_31_minus_1_blocks",
           "xtab_offsets_and_total_are_the_drivers", "xtab_scratch_is_the_drivers"]


def test_layouts_and_grid(lines):
    """6 view counts x 4; 10^3 trimmed shapes (2-D: one plane) x both grids x 2; the launch limit on a synthetic 2^31-block shape (4);
    the x-weight table (2)."""
    assert _table(lines, "C")["layouts"] == 6 * 4 + 10 ** 3 * 2 * 2 + 4 + 2
    _wrong(lines, LAYOUTS)


BOXES = ["identity_box_equals_the_walk", "turned_view_reaches_the_chunk", "turned_box_holds_every_voxel_in_bounds"]


def test_chunk_boxes(lines):
    """5 translated views x 3 axes against the walk; 4 turned views (90 and 30 degrees about z, a mirror, an anisotropic scale) of a
    9 x 14 x 11 slab in a 24 x 20 x 28 chunk: the box holds every voxel in bounds."""
    assert _table(lines, "C")["boxes"] == 5 * 3 + 4 * 2
    _wrong(lines, BOXES)
