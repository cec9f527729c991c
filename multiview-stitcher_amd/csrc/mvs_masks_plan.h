// mvs_masks_plan.h -- host-only pure C++ of the sample-mask entry points (mvs_masks.hip): their limits, the half neighbourhood of the
// contact search and the launch geometry of the line and row kernels.  No HIP: tests/native/masks_plan_host_test.cpp compiles it
// with the host compiler under the address and undefined-behaviour sanitizers.
#pragma once
#include <cstdint>

namespace mvs_masks_plan {

constexpr int kMaxBins = 4096;        // MVS_HIST_MAX_BINS: uint32 bins of one workgroup in LDS (16 KiB)
constexpr int kMaxDilate = 32;        // MVS_MASK_MAX_DILATE: the x pass reads two 16-byte groups on either side of its own
constexpr int kMaxLabels = 2048;      // MVS_LABEL_MAX: the dense uint64 contact matrix is 32 MiB
constexpr int kGroup = 16;            // mask voxels per lane: one 16-byte load
constexpr int kThreads = 256;         // four waves per workgroup in every kernel of the file
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 2048;      // grid cap of the grid-stride kernels (256 CUs x 8 workgroups)
constexpr int kMaxOffsets = 13;       // half of the 26 neighbours of a voxel

// ---- the half neighbourhood ---------------------------------------------------------------------------------------------------------
// The offsets o in {-1, 0, 1}^ndim (2D: dz == 0) with 1 <= #non-zero components <= connectivity whose first non-zero component (in
// z, y, x order) is +1: of every offset and its negative exactly one.  Anti-diagonals such as (0, +1, -1) are members.  Returns their
// number: 2 / 4 in 2D (connectivity 1 / 2), 3 / 9 / 13 in 3D; 0 for arguments out of range.
struct Offset {
    int dz, dy, dx;
};

inline int half_neighbourhood(int ndim, int connectivity, Offset out[kMaxOffsets]) {
    if ((ndim != 2 && ndim != 3) || connectivity < 1 || connectivity > ndim) return 0;
    int n = 0;
    for (int dz = (ndim == 3 ? -1 : 0); dz <= (ndim == 3 ? 1 : 0); ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int nonzero = (dz != 0) + (dy != 0) + (dx != 0);
                if (nonzero < 1 || nonzero > connectivity) continue;
                const int first = dz ? dz : (dy ? dy : dx);
                if (first < 0) continue;
                out[n++] = Offset{dz, dy, dx};
            }
    return n;
}

// ---- launch geometry ----------------------------------------------------------------------------------------------------------------
// A mask row of nx voxels is worked on in groups of kGroup voxels, one lane each; the work rows of the dilation have a pitch of
// whole groups, so that every group starts on a 16-byte boundary.
inline long long row_groups(long long nx) { return (nx + kGroup - 1) / kGroup; }
inline long long padded_pitch(long long nx) { return row_groups(nx) * kGroup; }

// Workgroups of a grid-stride launch over `items` items, `per_block` of them per workgroup and step: at least 1, at most kMaxBlocks.
inline int grid_blocks(long long items, int per_block) {
    const long long want = (items + per_block - 1) / per_block;
    return (int)(want < 1 ? 1 : (want > kMaxBlocks ? kMaxBlocks : want));
}

// Workgroups of the histogram launch (one wave per row and step, kWaves rows per workgroup and step).  A workgroup counts into
// uint32 bins and flushes them once, so the rows it takes may not hold 2^32 voxels or more: with rows of at most max_nx voxels the
// grid grows beyond kMaxBlocks where kMaxBlocks workgroups would each take more than 2^31 voxels.
inline long long hist_blocks(long long total_rows, long long max_nx) {
    long long blocks = grid_blocks(total_rows, kWaves);
    const long long limit = (1LL << 31) / (max_nx < 1 ? 1 : max_nx);      // rows one workgroup may take
    const long long per_block_rows = limit < kWaves ? kWaves : limit / kWaves * kWaves;
    const long long need = (total_rows + per_block_rows - 1) / per_block_rows;
    return need > blocks ? need : blocks;
}

// Rows the workgroup `block` of `blocks` takes at most: ceil(ceil(rows / kWaves) / blocks) steps of kWaves rows.
inline long long hist_rows_per_block(long long total_rows, long long blocks) {
    const long long steps = (total_rows + kWaves - 1) / kWaves;
    return (steps + blocks - 1) / blocks * kWaves;
}

}  // namespace mvs_masks_plan
