// mvs_affine_walk_dev.h -- the voxel walk the three kernels of affine_registration share: the normal equations
// (affine_neq_kernel, mvs_affine_reg.hip), the Mattes joint histogram and its gradient (mi_hist_kernel, mi_grad_kernel,
// mvs_affine_mi.hip).  Host/device: tests/native/affine_walk_host_test.cpp runs block_pos and walk_run for every block, wave
// and lane on the CPU against a plain loop over the crop.
//
// Geometry.  A block is WAVES waves over 64 consecutive x columns of one z plane and one chunk of ROWS_PER_BLOCK rows; block
// index = (z * nyc + yc) * nxb + xb.  A thread keeps its x = xb * 64 + lane (and the block its z); wave w takes the rows
// y = yc * ROWS_PER_BLOCK + w + WAVES * i, i < RUN, so only y changes along its run.  For each row the thread warps the voxel
// by the centred pose in double, splits the coordinate, takes its 4 or 8 taps and drops the sample when any value is not finite
// (the per-sample arithmetic is mvs_affine_reg_dev.h).
#pragma once
#include "mvs_affine_reg_dev.h"
#include "mvs_fold_dev.h"

namespace mvs_aw {

constexpr int WAVES = 4;      // waves of a block: wave w takes rows y0 + w, y0 + w + 4, ...
constexpr int RUN = 32;       // rows per thread: the length of a float32 run sum
constexpr int ROWS_PER_BLOCK = WAVES * RUN;

// pose and launch geometry: the leading part of every walking kernel's parameter block
struct Walk {
    const float* fixed;
    const float* moving;
    long long n[3];      // z, y, x (z = 1 in 2D)
    double A[9];         // 3x3, row-major (z, y, x); 2D uses the lower right 2x2
    double o[3];         // c + t
    double c[3];
    int nxb, nyc;        // blocks along x and y
};

// centre, c + t, pose and block counts of a crop of `shape` (z, y, x) under the pose [matrix | offset]; returns the number of blocks
inline long long set_geometry(Walk* W, const int64_t shape[3], const double matrix[9], const double offset[3]) {
    for (int k = 0; k < 3; ++k) {
        W->n[k] = shape[k];
        W->c[k] = (double)(shape[k] - 1) / 2.0;
        W->o[k] = W->c[k] + offset[k];
    }
    for (int k = 0; k < 9; ++k) W->A[k] = matrix[k];
    W->nxb = (int)((shape[2] + 63) / 64);
    W->nyc = (int)((shape[1] + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
    return (long long)W->nxb * W->nyc * shape[0];
}

struct BlockPos {
    int xb, yc;
    long long z;
};
__host__ __device__ __forceinline__ BlockPos block_pos(const Walk& P, long long block) {
    BlockPos r;
    r.xb = (int)(block % P.nxb);
    block /= P.nxb;
    r.yc = (int)(block % P.nyc);
    r.z = block / P.nyc;
    return r;
}

// The samples of one thread's run: f(fixed value, moving value, gradient, y - c_y as float) for every valid one.
template <int ND, typename F>
__host__ __device__ __forceinline__ void walk_run(const Walk& P, long long z, int yc, int wave, long long x, double dzd, double dxd, F&& f) {
    const long long ny = P.n[1], nx = P.n[2];
    if (x >= nx) return;
    // the products of the coordinate that do not change along the run (each rounds on its own, as in coord2 / coord3)
    double az[3], ax[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        az[k] = P.A[k * 3 + 0] * dzd;
        ax[k] = P.A[k * 3 + 2] * dxd;
    }
    const long long y0 = (long long)yc * ROWS_PER_BLOCK + wave;
    const float* __restrict__ frow = P.fixed + (z * ny + y0) * nx + x;
    for (int i = 0; i < RUN; ++i, frow += WAVES * nx) {
        const long long y = y0 + (long long)i * WAVES;
        if (y >= ny) break;
        const float fv = *frow;
        if (!mvs_ar::finite_f(fv)) continue;
        const double dyd = (double)y - P.c[1];
        float v, g[ND];
        if constexpr (ND == 3) {
            long long iz, iy, ix;
            float fz, fy, fx;
            if (!mvs_ar::split(((az[0] + P.A[1] * dyd) + ax[0]) + P.o[0], P.n[0], &iz, &fz)) continue;
            if (!mvs_ar::split(((az[1] + P.A[4] * dyd) + ax[1]) + P.o[1], ny, &iy, &fy)) continue;
            if (!mvs_ar::split(((az[2] + P.A[7] * dyd) + ax[2]) + P.o[2], nx, &ix, &fx)) continue;
            const float* __restrict__ m = P.moving + (iz * ny + iy) * nx + ix;
            const long long sz = ny * nx;
            const float taps[8] = {m[0], m[1], m[nx], m[nx + 1], m[sz], m[sz + 1], m[sz + nx], m[sz + nx + 1]};
            if (!mvs_ar::sample3(taps, fz, fy, fx, &v, g)) continue;
        } else {
            long long iy, ix;
            float fy, fx;
            if (!mvs_ar::split((P.A[4] * dyd + ax[1]) + P.o[1], ny, &iy, &fy)) continue;
            if (!mvs_ar::split((P.A[7] * dyd + ax[2]) + P.o[2], nx, &ix, &fx)) continue;
            const float* __restrict__ m = P.moving + iy * nx + ix;
            const float taps[4] = {m[0], m[1], m[nx], m[nx + 1]};
            if (!mvs_ar::sample2(taps, fy, fx, &v, g)) continue;
        }
        f(fv, v, g, (float)dyd);
    }
}

// ---- device only: the reductions that follow a walk ----
__device__ __forceinline__ double wave_sum(double v) { return mvs_fold::wave_fold(mvs_fold::Sums<double>{{v}}).v[0]; }

// out[j] = sum over the blocks of partials[b][j]: thread t takes b = t, t + 256, ... in order, then a fixed tree in LDS
static __global__ __launch_bounds__(256) void rows_sum_kernel(const double* __restrict__ partials, long long nblocks, int nout,
                                                              double* __restrict__ out) {
    __shared__ double s[256];
    const int j = blockIdx.x;
    double acc = 0.0;
    for (long long b = threadIdx.x; b < nblocks; b += 256) acc += partials[(size_t)b * nout + j];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[j] = s[0];
}

}  // namespace mvs_aw
