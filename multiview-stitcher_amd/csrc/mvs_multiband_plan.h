// mvs_multiband_plan.h -- host-only pure C++ of the multi-band fusion (mvs_multiband.hip): its limits, the launch geometry and, per
// axis, the extent and the global start of every pyramid level.  No HIP: tests/native/multiband_plan_host_test.cpp compiles it with
// the host compiler under the address and undefined-behaviour sanitizers.
//
// Level l + 1 decimates axis d only if levels[d] > l.  Along a decimated axis it keeps the samples at GLOBAL even indices of level l
// (coarse index K sits at fine index 2K) and holds EVERY coarse sample whose 5-tap window [2K - 2, 2K + 2] meets level l's extent
// [s, s + n): K from ceil((s - 2) / 2) to floor((s + n + 1) / 2).  That rule is what makes a chunk clipped at the stack, a chunk padded
// beyond it and the whole stack agree on every sample they share.
#pragma once
#include <cstdint>

#include "mvs_stack_frame.h"

namespace mvs_multiband_plan {

constexpr int kMaxLevels = 6;         // levels per axis: the radius 4 (2^L - 1) is 252 voxels at 6
constexpr int kMaxViews = 254;        // the winner map is one byte per voxel; 255 = no view covers it
constexpr int kNoView = 255;
constexpr int kThreads = 256;         // four waves per workgroup in every kernel of the file
constexpr int kMaxBlocks = 2048;      // grid cap of the grid-stride kernels (256 CUs x 8 workgroups)
constexpr long long kMaxIndex = 1LL << 29;   // |index_origin| and every extent stay below it: global indices (and twice a coarse one) are 32-bit in the kernels
// REDUCE tile of one workgroup and step: kTileY x kTileX coarse samples of one coarse z plane, computed from a window of
// (2 kTileY + 3) x (2 kTileX + 3) level-l samples (2 samples of apron on either side, shared end sample) held in LDS
constexpr int kTileY = 16, kTileX = 32;
constexpr int kWinY = 2 * kTileY + 3, kWinX = 2 * kTileX + 3;
constexpr int kLdsBytes = (kWinY + kTileY) * kWinX * 4;      // the window and its y-reduced rows: 13,668 bytes
constexpr int kFlagBytes = 256;       // head of the work area: the "views differ somewhere" word, cleared with its padding

inline long long floor_half(long long a) { return a >= 0 ? a / 2 : -((-a + 1) / 2); }
inline long long ceil_half(long long a) { return -floor_half(-a); }

struct Axis {
    long long start[kMaxLevels + 1];   // global index of the level's first sample
    long long n[kMaxLevels + 1];       // its extent
    int decimated[kMaxLevels];         // [l]: level l + 1 decimates this axis
};

struct Plan {
    Axis axis[3];                      // z, y, x
    int top;                           // L = the largest level count
    long long size[kMaxLevels + 1];    // samples of a level (one plane)
};

// One axis: extents and starts of levels 0 .. top for `levels` decimations of an axis of n samples that starts at global index s.
inline void plan_axis(long long s, long long n, int levels, int top, Axis* a) {
    a->start[0] = s;
    a->n[0] = n;
    for (int l = 0; l < top; ++l) {
        a->decimated[l] = levels > l;
        if (!a->decimated[l]) {
            a->start[l + 1] = a->start[l];
            a->n[l + 1] = a->n[l];
            continue;
        }
        const long long lo = ceil_half(a->start[l] - 2), hi = floor_half(a->start[l] + a->n[l] + 1);
        a->start[l + 1] = lo;
        a->n[l + 1] = hi - lo + 1;
    }
    for (int l = top; l < kMaxLevels; ++l) a->decimated[l] = 0;
}

// The whole plan.  False for arguments out of range: a level count outside 0 .. kMaxLevels, an extent < 1 or >= kMaxIndex, an origin
// beyond +-kMaxIndex.
inline bool make_plan(const int32_t levels[3], const int64_t index_origin[3], const int64_t shape[3], Plan* p) {
    p->top = 0;
    for (int d = 0; d < 3; ++d) {
        if (levels[d] < 0 || levels[d] > kMaxLevels || shape[d] < 1 || shape[d] >= kMaxIndex) return false;
        if (index_origin[d] > kMaxIndex || index_origin[d] < -kMaxIndex) return false;
        if (levels[d] > p->top) p->top = levels[d];
    }
    for (int d = 0; d < 3; ++d) plan_axis(index_origin[d], shape[d], levels[d], p->top, &p->axis[d]);
    for (int l = 0; l <= kMaxLevels; ++l) p->size[l] = l <= p->top ? p->axis[0].n[l] * p->axis[1].n[l] * p->axis[2].n[l] : 0;
    return true;
}

// Samples of levels 1 .. top of one plane: what the pyramid costs on top of level 0.
inline long long coarse_samples(const Plan& p) {
    long long s = 0;
    for (int l = 1; l <= p.top; ++l) s += p.size[l];
    return s;
}

// The device work area of one call, every part on a 256-byte boundary: flag | F0 | winner map | gD of levels 0 .. L (n_views planes
// each) | gA of levels 1 .. L | r of levels 1 .. L (one plane) | `staged_bytes` of a host result.
struct WorkArea {
    size_t flag, f0, win;
    size_t d[kMaxLevels + 1], a[kMaxLevels + 1], r[kMaxLevels + 1];      // (a[0], r[0] and the levels above the top: 0, not held)
    size_t out, total;
};

inline WorkArea work_area(const Plan& p, int n_views, size_t staged_bytes) {
    WorkArea w = {};
    mvs_stack_frame::Layout L;
    w.flag = L.take(kFlagBytes, 256);
    w.f0 = L.take((size_t)p.size[0] * 4, 256);
    w.win = L.take((size_t)p.size[0], 256);
    for (int l = 0; l <= p.top; ++l) w.d[l] = L.take((size_t)p.size[l] * 4 * n_views, 256);
    for (int l = 1; l <= p.top; ++l) w.a[l] = L.take((size_t)p.size[l] * 4 * n_views, 256);
    for (int l = 1; l <= p.top; ++l) w.r[l] = L.take((size_t)p.size[l] * 4, 256);
    w.out = L.take(staged_bytes, 1);
    w.total = L.total;
    return w;
}

// The voxels whose inputs can reach a result: 4 (2^levels - 1) per axis (required_overlap).
inline long long radius(int levels) { return 4LL * ((1LL << levels) - 1); }

// Workgroups of a grid-stride launch over `items` items, `per_block` of them per workgroup and step: at least 1, at most kMaxBlocks.
inline int grid_blocks(long long items, long long per_block) {
    const long long want = (items + per_block - 1) / per_block;
    return (int)(want < 1 ? 1 : (want > kMaxBlocks ? kMaxBlocks : want));
}

// Tiles of the REDUCE launch that writes a level of extents (ny, nx) per plane and coarse z.
constexpr long long tiles_y(long long ny) { return (ny + kTileY - 1) / kTileY; }
constexpr long long tiles_x(long long nx) { return (nx + kTileX - 1) / kTileX; }

}  // namespace mvs_multiband_plan
