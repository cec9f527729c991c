// mvs_components_plan.h -- host-only pure C++ of connected-component labelling (mvs_components.hip): the half neighbourhood as the
// merge launch walks it, the launch geometry, the partition of the numbering scan, scratch sizes and limits.  No HIP is needed to
// read it: tests/native/components_host_test.cpp compiles it with the host compiler under the sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "mvs_labels_plan.h"
#include "mvs_masks_plan.h"

namespace mvs_components_plan {

using mvs_labels_plan::chunks_per_wave;
using mvs_labels_plan::grid_blocks;
using mvs_labels_plan::kMaxBlocks;
using mvs_labels_plan::kThreads;
using mvs_labels_plan::kWaves;
using mvs_labels_plan::row_chunks;

constexpr long long kMaxVoxels = 0x7fffffffLL;      // linear indices and ids are int32
constexpr int kMaxRowGroups = 4;                    // neighbour rows of the half neighbourhood: (0,+1), (+1,-1), (+1,0), (+1,+1)
constexpr int kMaxScanBlocks = 2048;                // block counts one workgroup scans: 8 per thread
constexpr int kBackground = -1;                     // parent[] of a background voxel

// Voxels of a shape, or -1 above kMaxVoxels (every extent >= 1).
inline long long voxel_count(const int64_t shape[3]) {
    long long n = 1;
    for (int k = 0; k < 3; ++k) {
        if (shape[k] < 1 || shape[k] > kMaxVoxels / n) return -1;
        n *= shape[k];
    }
    return n;
}

// ---- the half neighbourhood by neighbour row ----------------------------------------------------------------------------------------
// The offsets of mvs_masks_plan::half_neighbourhood with a non-zero y or z component, grouped by the row (dz, dy) they reach; bit
// dx + 1 of dx_mask is set for every dx of the group.  (The one offset without such a component, (0, 0, +1), joins voxels of one
// run: the row launch has done that.)  Returns the number of groups: 1 in 2D, 2 / 4 / 4 in 3D (connectivity 1 / 2 / 3); 0 for
// arguments out of range.
struct RowGroup {
    int dz, dy;
    unsigned dx_mask;
};

inline int row_groups(int ndim, int connectivity, RowGroup out[kMaxRowGroups]) {
    mvs_masks_plan::Offset off[mvs_masks_plan::kMaxOffsets];
    const int n_off = mvs_masks_plan::half_neighbourhood(ndim, connectivity, off);
    int n = 0;
    for (int i = 0; i < n_off; ++i) {
        if (!off[i].dz && !off[i].dy) continue;
        int g = 0;
        while (g < n && (out[g].dz != off[i].dz || out[g].dy != off[i].dy)) ++g;
        if (g == n) out[n++] = RowGroup{off[i].dz, off[i].dy, 0u};
        out[g].dx_mask |= 1u << (off[i].dx + 1);
    }
    return n;
}

// Offsets the groups stand for, the x-only one included: the size of the half neighbourhood.
inline int offsets_of(const RowGroup* groups, int n) {
    int total = 1;
    for (int g = 0; g < n; ++g)
        for (int b = 0; b < 3; ++b) total += (groups[g].dx_mask >> b) & 1u;
    return total;
}

// ---- the numbering scan -------------------------------------------------------------------------------------------------------------
// Roots are numbered in raster order by an exclusive scan in three launches: workgroup b counts the flagged roots of the voxels
// [b * span, min((b + 1) * span, n)), one workgroup scans the `blocks` counts, workgroup b then ranks its voxels from its base.
// span is a multiple of the workgroup, blocks <= kMaxScanBlocks, and the ranges cover 0 .. n - 1 once.
struct ScanPlan {
    int blocks;
    long long span;
};

inline ScanPlan scan_plan(long long n) {
    ScanPlan p{1, kThreads};
    if (n < 1) return p;
    long long span = (n + kMaxScanBlocks - 1) / kMaxScanBlocks;
    span = (span + kThreads - 1) / kThreads * kThreads;
    p.span = span;
    p.blocks = (int)((n + span - 1) / span);
    return p;
}

// ---- scratch ------------------------------------------------------------------------------------------------------------------------
// Bytes of the call's device block after a staged host tile: parent (4 per voxel), sizes (4 more, only with min_voxels > 1), the
// block counts of the scan and its total, and the result itself when it goes to the host.  Every part on a 256-byte boundary.
inline size_t round256(size_t v) { return (v + 255) / 256 * 256; }
inline size_t parent_bytes(long long n) { return round256(sizeof(int32_t) * (size_t)n); }
inline size_t sizes_bytes(long long n, long long min_voxels) { return min_voxels > 1 ? round256(sizeof(uint32_t) * (size_t)n) : 0; }
inline size_t scan_bytes() { return round256(sizeof(int32_t) * (size_t)(kMaxScanBlocks + 1)); }

}  // namespace mvs_components_plan
