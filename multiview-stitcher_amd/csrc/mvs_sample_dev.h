// mvs_sample_dev.h -- internal: the one nearest / linear sampler of a view (DevView) that the generic fuse kernel, mvs_resample
// (mvs_fuse.hip) and the pair metrics kernel (mvs_pair_metrics.hip) share, so that a voxel sampled by any of them has the same bits;
// and the brick / view test by which the generic fuse kernel and the label fuse kernel (mvs_masks.hip) cull views.
#pragma once
#include "mvs_fuse_dev.h"

template <typename T> __device__ __forceinline__ float load_as_float(const T* p, long long i);
template <> __device__ __forceinline__ float load_as_float<unsigned char>(const unsigned char* p, long long i) { return (float)p[i]; }
template <> __device__ __forceinline__ float load_as_float<unsigned short>(const unsigned short* p, long long i) { return (float)p[i]; }
template <> __device__ __forceinline__ float load_as_float<float>(const float* p, long long i) { return p[i]; }

// second tap of a linear interpolation at the upper border: scipy maps the
// out-of-range index by mirroring (ni_interpolation.c, edge offsets), its
// weight is 0 there.
__device__ __forceinline__ int second_tap(int i0, int n) {
    int i1 = i0 + 1;
    if (i1 >= n) i1 = (n > 1) ? n - 2 : 0;
    return i1;
}

// Sample one view at in-bounds double coordinates. ORDER 1: trilinear with all
// 8 taps always loaded (0 * NaN = NaN propagates like scipy); ORDER 0: nearest
// = floor(c + 0.5).
template <typename TIn, int ORDER>
__device__ __forceinline__ float sample_view(const DevView& V, double cz, double cy, double cx) {
    const TIn* p = (const TIn*)V.data;
    if (ORDER == 0) {
        int iz = (int)floor(cz + 0.5), iy = (int)floor(cy + 0.5), ix = (int)floor(cx + 0.5);
        return load_as_float<TIn>(p, iz * V.stride_z + iy * V.stride_y + ix);
    } else {
        double fz_ = floor(cz), fy_ = floor(cy), fx_ = floor(cx);
        int iz = (int)fz_, iy = (int)fy_, ix = (int)fx_;
        float wz = (float)(cz - fz_), wy = (float)(cy - fy_), wx = (float)(cx - fx_);
        int iz1 = second_tap(iz, V.nz), iy1 = second_tap(iy, V.ny), ix1 = second_tap(ix, V.nx);
        long long b00 = iz * V.stride_z + iy * V.stride_y;
        long long b01 = iz * V.stride_z + iy1 * V.stride_y;
        long long b10 = iz1 * V.stride_z + iy * V.stride_y;
        long long b11 = iz1 * V.stride_z + iy1 * V.stride_y;
        float v000 = load_as_float<TIn>(p, b00 + ix), v001 = load_as_float<TIn>(p, b00 + ix1);
        float v010 = load_as_float<TIn>(p, b01 + ix), v011 = load_as_float<TIn>(p, b01 + ix1);
        float v100 = load_as_float<TIn>(p, b10 + ix), v101 = load_as_float<TIn>(p, b10 + ix1);
        float v110 = load_as_float<TIn>(p, b11 + ix), v111 = load_as_float<TIn>(p, b11 + ix1);
        float ux = 1.f - wx, uy = 1.f - wy, uz = 1.f - wz;
        float a00 = fmaf(v001, wx, v000 * ux);
        float a01 = fmaf(v011, wx, v010 * ux);
        float a10 = fmaf(v101, wx, v100 * ux);
        float a11 = fmaf(v111, wx, v110 * ux);
        float b0 = fmaf(a01, wy, a00 * uy);
        float b1 = fmaf(a11, wy, a10 * uy);
        return fmaf(b1, wz, b0 * uz);
    }
}

// scipy's in-bounds test of a linear sample (NI_GeometricTransform, mode "constant"): 0 <= c <= n - 1 on every axis
__device__ __forceinline__ bool view_in_bounds(const DevView& V, double cz, double cy, double cx) {
    return !(cz < 0.0 || cz > (double)(V.nz - 1) || cy < 0.0 || cy > (double)(V.ny - 1) || cx < 0.0 || cx > (double)(V.nx - 1));
}

// Conservative test: can any voxel of the brick (chunk index box lo..hi, inclusive)
// land inside view V?  Exact classification happens per voxel afterwards.
__device__ __forceinline__ bool brick_hits_view(const DevView& V, const int lo[3], const int hi[3]) {
    const int n[3] = {V.nz, V.ny, V.nx};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double cmin = V.off[d], cmax = V.off[d];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double a = V.m[d * 3 + k] * (double)lo[k], b = V.m[d * 3 + k] * (double)hi[k];
            cmin += fmin(a, b);
            cmax += fmax(a, b);
        }
        if (cmax < -1e-3 || cmin > (double)(n[d] - 1) + 1e-3) return false;
    }
    return true;
}
