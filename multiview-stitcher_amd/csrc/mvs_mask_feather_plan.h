// mvs_mask_feather_plan.h -- host-only pure C++ of mvs_mask_feather (mvs_mask_feather.hip): the integer scale of the capped squared
// distance, the z slabs the passes work in and the scratch they need.  No HIP: tests/native/mask_feather_plan_host_test.cpp compiles
// it with the host compiler under the address and undefined-behaviour sanitizers.
//
// THE SCALE.  With widths w_k in 1 .. kMaxWidth per axis, D = prod_k w_k^2 and P_k = D / w_k^2 are integers, and
// N(p) = min(D, min_q sum_k (p_k - q_k)^2 P_k) over the zero voxels q is D t^2 exactly, t the capped distance of include/mvs_hip.h.
// D <= 32^6 = 2^30; a pass adds one term j^2 P_k <= w_k^2 P_k = D to a value capped at D: at most 2^31, inside uint32.
//
// THE SLABS.  The x and y passes of a slab of `planes` output planes run over those planes and a halo of w_z planes on either side
// (cut at the mask's first and last plane), the z pass over the output planes only.  SCRATCH BOUND: two uint32 plane sets of
// planes + 2 halo planes of ny nx voxels each, 8 (planes + 2 halo) ny nx bytes, at most kSlabBudget of them unless one plane with its
// halo already needs more (the slab is then one plane: 8 (1 + 2 halo) ny nx bytes).
#pragma once
#include <cstddef>
#include <cstdint>

namespace mvs_mask_feather_plan {

constexpr int kMaxWidth = 32;                       // MVS_FEATHER_MAX_WIDTH
constexpr int kFullWeight = 252;                    // MVS_FEATHER_FULL_WEIGHT
constexpr int kGroup = 16;                          // voxels per lane of the x pass
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                    // grid cap of the grid-stride kernels
constexpr size_t kSlabBudget = (size_t)256 << 20;   // bytes of both plane sets of one slab

struct Scale {
    uint32_t D;          // the cap: t = 1
    uint32_t P[3];       // weight of one squared voxel step along z, y, x
};

// widths (z, y, x), each 1 .. kMaxWidth (the caller has checked); an axis that does not exist (2D: z) has width 1
inline Scale scale_of(const int w[3]) {
    Scale s;
    const uint32_t q[3] = {(uint32_t)(w[0] * w[0]), (uint32_t)(w[1] * w[1]), (uint32_t)(w[2] * w[2])};
    s.D = q[0] * q[1] * q[2];
    s.P[0] = q[1] * q[2];
    s.P[1] = q[0] * q[2];
    s.P[2] = q[0] * q[1];
    return s;
}

// a y / z pass changes nothing along an axis of one voxel, nor with width 1 (one step already costs D)
inline bool pass_needed(int extent, int width) { return extent > 1 && width > 1; }

// output planes per slab: `forced` (> 0: library option "feather_slab_planes") or as many as the budget holds, 1 .. nz
inline long long slab_planes(long long nz, long long ny, long long nx, int halo, long long forced, size_t budget = kSlabBudget) {
    long long s;
    if (forced > 0) {
        s = forced;
    } else {
        const long long per_plane = 8LL * ny * nx;
        s = (long long)(budget / (size_t)(per_plane < 1 ? 1 : per_plane)) - 2LL * halo;
    }
    return s < 1 ? 1 : (s > nz ? nz : s);
}

inline long long n_slabs(long long nz, long long planes) { return (nz + planes - 1) / planes; }

// slab k: its output planes [z0, z1) and the planes [h0, h1) the x and y passes cover
struct Slab {
    long long z0, z1, h0, h1;
};
inline Slab slab(long long k, long long nz, long long planes, int halo) {
    Slab s;
    s.z0 = k * planes;
    s.z1 = s.z0 + planes < nz ? s.z0 + planes : nz;
    s.h0 = s.z0 - halo > 0 ? s.z0 - halo : 0;
    s.h1 = s.z1 + halo < nz ? s.z1 + halo : nz;
    return s;
}

// bytes of ONE of the two uint32 plane sets
inline size_t plane_set_bytes(long long nz, long long ny, long long nx, long long planes, int halo) {
    long long p = planes + 2LL * halo;
    if (p > nz) p = nz;
    return (size_t)p * (size_t)ny * (size_t)nx * sizeof(uint32_t);
}

inline int grid_blocks(long long items, int per_block) {
    const long long want = (items + per_block - 1) / per_block;
    return (int)(want < 1 ? 1 : (want > kMaxBlocks ? kMaxBlocks : want));
}

}  // namespace mvs_mask_feather_plan
