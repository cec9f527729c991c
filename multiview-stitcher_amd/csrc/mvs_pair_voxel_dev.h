// mvs_pair_voxel_dev.h -- internal, device only: what the kernels that reduce sample pairs over an overlap grid share
// (mvs_pair_metrics.hip, mvs_intensity.hip, mvs_nonrigid.hip): the per-voxel rule of mvs_pair_moments (halfspace mask, grid index ->
// pixel, in-bounds test, linear float32 sample, finite test) and the fold of the workgroups' results by one wave (the wave step of
// the fixed merge tree is mvs_fold::wave_fold).  One copy, so that a voxel counted by any of the kernels is the same voxel with the same bits.
#pragma once
#include "mvs_fold_dev.h"
#include "mvs_sample_dev.h"
#include "mvs_pair_metrics_dev.h"

// step 1: ((a_z z + a_y y) + a_x x) + b <= 0 for every row of `hs`
__device__ __forceinline__ bool pair_mask_holds(const double (*hs)[4], int n_hs, double pz, double py, double px) {
    bool inside = true;
    for (int h = 0; h < n_hs; ++h) inside = inside && (((hs[h][0] * pz + hs[h][1] * py) + hs[h][2] * px) + hs[h][3] <= 0.0);
    return inside;
}

// grid index -> pixel: c = ((z m0 + y m1) + x m2) + offset per axis (`m`: 9 doubles row-major, `off`: 3)
__device__ __forceinline__ void pair_grid_to_pixel(const double* m, const double* off, double pz, double py, double px, double& cz, double& cy,
                                                   double& cx) {
    cz = ((pz * m[0] + py * m[1]) + px * m[2]) + off[0];
    cy = ((pz * m[3] + py * m[4]) + px * m[5]) + off[1];
    cx = ((pz * m[6] + py * m[7]) + px * m[8]) + off[2];
}

// steps 2-4 for one tile at an in-bounds-tested coordinate: false when the coordinate is out of bounds or the sample is not finite
template <typename T>
__device__ __forceinline__ bool pair_sample_finite(const DevView& V, double cz, double cy, double cx, float* v) {
    if (!view_in_bounds(V, cz, cy, cx)) return false;
    *v = sample_view<T, 1>(V, cz, cy, cx);
    return isfinite(*v);
}

// The fold of the n results p[0], p[stride], ... by one wave: lane l merges its run of ceil(n / 64) consecutive ones in index order,
// then the lanes merge in the tree of mvs_fold::wave_fold -- every result's place in the tree is a function of (n, its index) only.  Lane 0
// gets the fold.
__device__ __forceinline__ PairMoments pair_moments_fold(const PairMoments* p, long long stride, int n, int lane) {
    const int run = (n + 63) / 64;
    const int lo = lane * run, hi = min(lo + run, n);
    PairMoments r = pair_moments_empty();
    for (int i = lo; i < hi; ++i) r = pair_moments_merge(r, p[(long long)i * stride]);
    return mvs_fold::wave_fold(r);
}
