"""The grid caps of the grid-stride kernels and the shapes at which tests/test_grid_stride_gpu.py runs them past their first trip.

A capped grid-stride launch has ``min(ceil(items / per_block), cap)`` workgroups; a *trip* is one pass of its loop over
``cap * per_block`` items.  Each row of ``ROWS`` names a launch group, where its cap is defined, the value the GPU tests assume, the
items a workgroup takes per trip, and the shapes of the GPU test with the item count the entry point derives from them.
tests/test_launch_caps_host.py checks every row on the CPU: the cap in the source text is the assumed one, and every shape gives
``min_trips < trips < 3``.  Whoever raises a cap gets that failure, which names the row and the shape to enlarge, instead of a GPU
test that no longer reaches the second trip."""
import math
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("multiview-stitcher_amd", "csrc")


def trips(items, per_block, cap):
    """Passes of the grid-stride loop that the launch needs for ``items`` items: items / (workgroups * per_block) with
    workgroups = min(ceil(items / per_block), cap).  At 2.3 every workgroup steps its loop at least once, the first 30 % of the
    grid twice, and the last trip is taken by part of the grid only."""
    blocks = max(1, min(-(-items // per_block), cap))
    return items / float(blocks * per_block)


# ---- the arithmetic of the entry points ---------------------------------------------------------------------------------------------
def prod(shape):
    return int(math.prod(int(s) for s in shape))


def rows_of(shape):
    """(z, y) rows of a 2-D / 3-D tile."""
    return prod(shape[:-1])


def hist_blocks(total_rows, max_nx, cap=2048, waves=4):
    """mvs_masks_plan::hist_blocks: the capped grid, grown where a workgroup would take 2^31 voxels or more."""
    blocks = max(1, min(-(-total_rows // waves), cap))
    limit = (1 << 31) // max(max_nx, 1)
    per_block_rows = waves if limit < waves else limit // waves * waves
    need = -(-total_rows // per_block_rows)
    return max(need, blocks)


def hist_rows(shapes):
    return sum(rows_of(s) for s in shapes)


def mask_groups(shape):
    """16-voxel groups of a mask volume: rows * ceil(nx / 16)."""
    return rows_of(shape) * -(-int(shape[-1]) // 16)


def contact_chunks(shape):
    """64-voxel chunks of a label volume: rows * ceil(nx / 64)."""
    return rows_of(shape) * -(-int(shape[-1]) // 64)


def maxima_tiles(shape):
    """Tiles of 256 x positions: rows * ceil(nx / 256)."""
    return rows_of(shape) * -(-int(shape[-1]) // 256)


def dct_general_items(shape, dct_size, n_views=2):
    """(view, block) pairs of the general quality kernel."""
    return n_views * prod(-(-int(s) // min(int(dct_size), int(s))) for s in shape)


# ---- the shapes the GPU tests use ---------------------------------------------------------------------------------------------------
HIST_SHAPES = [(1, 9000, 21), (3, 3200, 13)]
HIST_WINDOW_SHAPES = [(1, 8999, 18), (3, 3199, 10)]             # the device windows [:, 1:, 3:] of the same tiles
MASK_SHAPE = (4, 80000, 20)
CONTACT_SHAPE = (2, 5000, 70)
MAXIMA_CASES = [((2, 4700, 260), (3, 5, 3)), ((18000, 7), (3, 3))]
APPLY_CASES = [((150000, 20), (7, 2)), ((40, 3800, 18), (2, 5, 2))]      # shape, nodes / cells
CELL_GRID = (6, 360, 280)
PAIR_GRID = (10, 300, 400)
RANGE_N = 2_400_000
ELEMENTWISE_SHAPE = (2300, 2000)                                # DCT interpolation and deconvolution: 2 views of it
DCT_GENERAL_SHAPE, DCT_GENERAL_SIZE = (140, 142), 2

ROWS = [
    # hist_range_kernel, hist_count_kernel: one wave per row, 4 rows per workgroup.  (hist_blocks may grow the grid past the cap
    # for rows of 2^29 voxels; the host test asserts that it does not for these.)
    dict(name="masks histogram and range", source=os.path.join(CSRC, "mvs_masks_plan.h"), cap=2048, pattern=r"constexpr int kMaxBlocks = (\d+);",
         per_block=4, min_trips=2.0, lib_constant=None,
         cases=[("host tiles", HIST_SHAPES, hist_rows(HIST_SHAPES)), ("device windows", HIST_WINDOW_SHAPES, hist_rows(HIST_WINDOW_SHAPES))]),
    # mask_threshold_kernel, mask_dilate_x_kernel, mask_dilate_lines_kernel: a lane per 16-voxel group.  Every trip of these is a
    # whole pass over a volume of 40 bytes per 16-voxel item, so 1.22 trips is what a few MB allow.
    dict(name="masks threshold and dilation", source=os.path.join(CSRC, "mvs_masks_plan.h"), cap=2048, pattern=r"constexpr int kMaxBlocks = (\d+);",
         per_block=256, min_trips=1.15, lib_constant=None, cases=[("uint8 and float32", MASK_SHAPE, mask_groups(MASK_SHAPE))]),
    # label_contacts_kernel: a wave per 64-voxel chunk
    dict(name="masks label contacts", source=os.path.join(CSRC, "mvs_masks_plan.h"), cap=2048, pattern=r"constexpr int kMaxBlocks = (\d+);",
         per_block=4, min_trips=2.0, lib_constant=None, cases=[("int32 labels", CONTACT_SHAPE, contact_chunks(CONTACT_SHAPE))]),
    # max_line_kernel (axes 2 and 1), maxima_last_kernel: a workgroup per tile of 256 x positions
    dict(name="detection local maxima", source=os.path.join(CSRC, "mvs_detect.hip"), cap=256 * 32,
         pattern=r"const dim3 g\(\(unsigned\)std::min<long long>\(T\.count, (\d+ \* \d+)\)\), b\(256\);", per_block=1, min_trips=2.0, lib_constant=None,
         cases=[("x".join(map(str, s)), s, maxima_tiles(s)) for s, _ in MAXIMA_CASES]),
    # field_warp_kernel: a wave per row, 4 rows per workgroup
    dict(name="non-rigid field warp", source=os.path.join(CSRC, "mvs_nonrigid.hip"), cap=16384, pattern=r"constexpr int kWarpMaxBlocks = (\d+);",
         per_block=4, min_trips=2.0, lib_constant=None, cases=[("x".join(map(str, s)), s, rows_of(s)) for s, _ in APPLY_CASES]),
    # intensity_apply_kernel: the same frame
    dict(name="intensity apply", source=os.path.join(CSRC, "mvs_intensity.hip"), cap=16384, pattern=r"constexpr int kApplyMaxBlocks = (\d+);",
         per_block=4, min_trips=2.0, lib_constant=None, cases=[("x".join(map(str, s)), s, rows_of(s)) for s, _ in APPLY_CASES]),
    # intensity_moments_kernel: the cap holds per record; a lane per voxel of the record's box
    dict(name="intensity cell moments", source=os.path.join("include", "mvs_hip.h"), cap=1024, pattern=r"#define MVS_INTENSITY_MAX_BLOCKS (\d+)",
         per_block=256, min_trips=2.0, lib_constant="MVS_INTENSITY_MAX_BLOCKS", cases=[("one record of the whole grid", CELL_GRID, prod(CELL_GRID))]),
    # pair_moments_kernel<T, K>: a lane per grid voxel
    dict(name="pair moments", source=os.path.join(CSRC, "mvs_pair_metrics_dev.h"), cap=2048, pattern=r"constexpr int kPairMaxBlocks = (\d+);",
         per_block=256, min_trips=2.0, lib_constant="MVS_PAIR_MAX_BLOCKS", cases=[("grid", PAIR_GRID, prod(PAIR_GRID))]),
    # finite_range_kernel: the launch is sized for 8 values per lane (its loop then steps by gridDim.x * 256, so a capped grid
    # takes 8 steps per trip counted here)
    dict(name="finite range", source=os.path.join(CSRC, "mvs_affine_mi.hip"), cap=512,
         pattern=r"const int nb = \(int\)std::min<long long>\(\(n \+ 256 \* 8 - 1\) / \(256 \* 8\), (\d+)\);", per_block=2048, min_trips=2.0,
         lib_constant=None, cases=[("values", (RANGE_N,), RANGE_N)]),
    # dct_interp_kernel (and dct_normalize_kernel, whose grid of blocks stays far below the cap): a lane per voxel
    dict(name="DCT weight interpolation", source=os.path.join(CSRC, "mvs_dct_weights.hip"), cap=256 * 32,
         pattern=r"int grid_for\(long long n\) \{ return \(int\)std::max<long long>\(1, std::min<long long>\(\(n \+ 255\) / 256, (\d+ \* \d+)\)\); \}",
         per_block=256, min_trips=2.0, lib_constant=None, cases=[("2 views", ELEMENTWISE_SHAPE, prod(ELEMENTWISE_SHAPE))]),
    # dct_quality_general: a workgroup and scratch slot per (view, block) pair, at most 4096 slots (the byte budget allows far more
    # slots of 2 x 2 blocks)
    dict(name="DCT general quality", source=os.path.join(CSRC, "mvs_dct_weights.hip"), cap=4096,
         pattern=r"n = std::max<long long>\(1, std::min<long long>\(\{n, items, (\d+)\}\)\);", per_block=1, min_trips=2.0, lib_constant=None,
         cases=[("2 views, dct_size 2", DCT_GENERAL_SHAPE, dct_general_items(DCT_GENERAL_SHAPE, DCT_GENERAL_SIZE))]),
    # the element-wise kernels of the deconvolution launched with grid_for(S) and grid_for(oz * oy * ox) of its plan header: a lane per voxel
    dict(name="deconvolution element-wise", source=os.path.join(CSRC, "mvs_deconv_plan.h"), cap=256 * 32,
         pattern=r"int grid_for\(long long n\) \{ return \(int\)std::max<long long>\(1, std::min<long long>\(\(n \+ 255\) / 256, (\d+ \* \d+)\)\); \}",
         per_block=256, min_trips=2.0, lib_constant=None, cases=[("2 views", ELEMENTWISE_SHAPE, prod(ELEMENTWISE_SHAPE))]),
]


def row(name):
    return next(r for r in ROWS if r["name"] == name)


def source_value(r):
    """The cap as the source text of the row defines it (an int; products such as ``256 * 32`` are multiplied out), or None when
    the pattern does not match exactly once."""
    import re

    with open(os.path.join(ROOT, r["source"]), encoding="utf-8") as f:
        found = re.findall(r["pattern"], f.read())
    if len(found) != 1:
        return None
    return math.prod(int(v) for v in found[0].split("*"))
