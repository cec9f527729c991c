// mvs_rank_plan.h -- the one definition of how the histogram rank kernels of mvs_score.hip divide the voxels of a crop among
// their workgroups, host/device: hist_ranks_apply sizes the launch with hist_launch, hist_rank_kernel takes its share with
// hist_range, and tests/native/rank_plan_host_test.cpp compiles both for the host.
//
// The voxels are handed out in groups of 4 consecutive ones, a contiguous range of groups per workgroup.  The counting pass
// keeps 16-bit counters in LDS, and all voxels of a workgroup may share one key, so a workgroup must get at most
// kHistGroupsMax groups = 65532 voxels: hist_launch derives the number of workgroups from the number of GROUPS the kernel will
// see (ceil(n / 4), not n / 4), and hist_per then cannot exceed kHistGroupsMax.
#pragma once
#include <hip/hip_runtime.h>

namespace mvs_rank_plan {

constexpr int kHistParts = 256;              // workgroups whose private histograms are written out and folded (more: atomic flush)
constexpr long long kHistGroupsMax = 16383;  // 4-voxel groups per workgroup of the counting pass: 65532 voxels <= 65535
constexpr long long kHistGridMax = 65535;    // workgroups of the counting pass beyond which the histogram route is not taken

// workgroups of the voxel-sized kernels of mvs_score.hip (also the grid of the correlation pass)
__host__ __device__ inline int score_grid(long long n) {
    const long long b = (n + 255) / 256;
    return (int)(b < 256 * 8 ? b : 256 * 8);
}

// 4-voxel groups of n voxels (n < 2^31 - 8)
__host__ __device__ inline unsigned int hist_groups(unsigned int n) { return (n + 3u) / 4u; }
// groups per workgroup when `grid` workgroups share them
__host__ __device__ inline unsigned int hist_per(unsigned int ngroups, unsigned int grid) { return (ngroups + grid - 1u) / grid; }
// the groups [g0, g1) of workgroup `block` out of `grid` (empty for the workgroups past the last group)
__host__ __device__ inline void hist_range(unsigned int n, unsigned int grid, unsigned int block, unsigned int* g0, unsigned int* g1) {
    const unsigned int ngroups = hist_groups(n), per = hist_per(ngroups, grid);
    const unsigned long long a = (unsigned long long)block * per;
    *g0 = a < ngroups ? (unsigned int)a : ngroups;
    *g1 = a + per < ngroups ? (unsigned int)(a + per) : ngroups;
}

// the launch of the counting pass for n voxels (gb = score_grid(n)): hgb workgroups; fold: they write their histograms out
// whole (at most kHistParts of them); ok: the launch fits the grid limit
struct HistLaunch { long long hgb; bool fold, ok; };
__host__ __device__ inline HistLaunch hist_launch(long long n, int gb) {
    const long long ngroups = (n + 3) / 4;
    const long long hneed = (ngroups + kHistGroupsMax - 1) / kHistGroupsMax;
    HistLaunch h;
    h.fold = hneed <= kHistParts;
    if (h.fold) {
        long long want = (n + 8191) / 8192;          // a workgroup per 8192 voxels while the parts can be folded
        if (want > kHistParts) want = kHistParts;
        h.hgb = hneed > want ? hneed : want;
    } else {
        h.hgb = hneed > gb ? hneed : gb;
    }
    h.ok = h.hgb <= kHistGridMax;
    return h;
}

}  // namespace mvs_rank_plan
