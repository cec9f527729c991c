"""CPU: the table of tests/launch_caps.py against the sources.  Per row, (a) the cap's definition in the source text carries the
value the GPU tests of tests/test_grid_stride_gpu.py assume (and equals the constant ``_lib`` exports, where it does), and (b) every
shape of the GPU test gives more than two trips of the grid-stride loop and fewer than three (more than 1.15 where the row says so),
by the arithmetic of the entry point.  For the histogram that arithmetic is mvs_masks_plan::hist_blocks itself, compiled from the
header with the host compiler."""
import os
import shutil
import subprocess

import pytest

from tests import launch_caps as lc

IDS = [r["name"] for r in lc.ROWS]


@pytest.mark.parametrize("r", lc.ROWS, ids=IDS)
def test_the_cap_in_the_source_is_the_assumed_one(r):
    found = lc.source_value(r)
    shapes = ", ".join(str(shape) for _, shape, _ in r["cases"])
    assert found is not None, f"row '{r['name']}': the pattern {r['pattern']!r} does not match {r['source']} exactly once"
    assert found == r["cap"], (f"row '{r['name']}': {r['source']} now sets the cap to {found}, tests/launch_caps.py assumes {r['cap']}: "
                               f"update the row and enlarge its shapes ({shapes}) until they give more than {r['min_trips']} trips again")
    if r["lib_constant"]:
        from multiview_stitcher_amd import _lib

        assert getattr(_lib, r["lib_constant"]) == r["cap"], f"row '{r['name']}': _lib.{r['lib_constant']} differs from the cap in {r['source']}"


@pytest.mark.parametrize("r", lc.ROWS, ids=IDS)
def test_the_test_shapes_pass_the_first_trip_twice(r):
    assert r["min_trips"] in (2.0, 1.15)
    for label, shape, items in r["cases"]:
        t = lc.trips(items, r["per_block"], r["cap"])
        print(f"{r['name']}: {label} {shape}: {items} items, {t:.3f} trips")
        assert r["min_trips"] < t < 3.0, f"row '{r['name']}': shape {shape} ({label}) gives {t:.3f} trips of {r['cap']} x {r['per_block']} items"
        # some workgroups take one step more than others: the last trip is a partial one
        assert items % (r["cap"] * r["per_block"]) != 0


def test_trips():
    assert lc.trips(1, 256, 2048) == 1 / 256                    # less than one workgroup
    assert lc.trips(2048 * 256, 256, 2048) == 1.0               # exactly the cap: no workgroup loops
    assert lc.trips(2048 * 256 + 1, 256, 2048) > 1.0
    assert lc.trips(3 * 8192, 1, 8192) == 3.0
    assert lc.trips(1000, 4, 16384) == 1.0                      # below the cap the grid fits the items


def test_item_counts_of_the_shapes():
    assert lc.hist_rows(lc.HIST_SHAPES) == 9000 + 3 * 3200 and lc.hist_rows(lc.HIST_WINDOW_SHAPES) == 8999 + 3 * 3199
    assert lc.mask_groups((4, 80000, 20)) == 4 * 80000 * 2 and lc.mask_groups((5, 16)) == 5 and lc.mask_groups((5, 17)) == 10
    assert lc.contact_chunks((2, 5000, 70)) == 20000 and lc.contact_chunks((3, 64)) == 3
    assert lc.maxima_tiles((2, 4700, 260)) == 18800 and lc.maxima_tiles((18000, 7)) == 18000 and lc.maxima_tiles((2, 256)) == 2
    assert lc.dct_general_items((140, 142), 2) == 2 * 70 * 71 and lc.dct_general_items((5, 7), 32) == 2
    for (tile, window) in zip(lc.HIST_SHAPES, lc.HIST_WINDOW_SHAPES):
        assert window == (tile[0], tile[1] - 1, tile[2] - 3)


HIST_PROGRAM = """
#include "mvs_masks_plan.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
    using namespace mvs_masks_plan;
    for (int i = 1; i + 1 < argc; i += 2) {
        const long long rows = atoll(argv[i]), nx = atoll(argv[i + 1]);
        printf("%lld %d %d %d\\n", hist_blocks(rows, nx), kMaxBlocks, kWaves, grid_blocks(rows, kWaves));
    }
    return 0;
}
"""


def test_hist_blocks_of_the_header_stays_at_the_cap(tmp_path):
    """The grid of the histogram launch is hist_blocks(total_rows, max_nx), which grows past the cap for long rows: for the row
    lengths of the test tiles it must not, or the launch takes fewer trips than the table says.  The header's own function, and
    the table's restatement of it against the header's on a long-row case that does grow."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    src, exe = tmp_path / "hist_blocks.cpp", tmp_path / "hist_blocks"
    src.write_text(HIST_PROGRAM)
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(lc.ROOT, lc.CSRC), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    row = lc.row("masks histogram and range")
    asked = []
    for _, shapes, rows in row["cases"]:
        asked.append((rows, max(s[-1] for s in shapes)))
    asked += [(3_000_000, 1 << 29), (5, 7)]
    r = subprocess.run([str(exe)] + [str(v) for pair in asked for v in pair], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [[int(v) for v in line.split()] for line in r.stdout.strip().splitlines()]
    assert len(lines) == len(asked)
    for (rows, nx), (blocks, cap, waves, capped) in zip(asked, lines):
        assert cap == row["cap"] and waves == row["per_block"]
        assert blocks == lc.hist_blocks(rows, nx, cap, waves), (rows, nx)
    for (rows, nx), (blocks, cap, _, capped) in list(zip(asked, lines))[:len(row["cases"])]:
        assert blocks == capped == cap, f"row '{row['name']}': hist_blocks({rows}, {nx}) = {blocks}, not the cap {cap}"
    assert lines[-2][0] > row["cap"] and lines[-1][0] == 2      # rows of 2^29 voxels grow the grid; five short rows take two workgroups
