// mvs_fuse_blend_dev.h -- internal: what the kernels that evaluate the full affine map per voxel (fuse_kernel and the resample / blend
// kernels of mvs_fuse.hip, fuse_weighted_kernel of mvs_fuse_weighted.hip) share beyond the sampler of mvs_sample_dev.h: the blend
// weight of a view at support-grid coordinates, the weighted-average accumulator, and the cast and the store of a lane's four
// result voxels.  One definition, so that a voxel fused by either kernel goes through the same float32 operations.
#pragma once
#include "mvs_sample_dev.h"
#include "mvs_fuse_tr.h"

constexpr int kVPT = 4;          // voxels per thread along x

// cosine ramp of weights.py:502-507: x<1 -> (cos((1-x)pi)+1)/2 == sin^2(pi x/2), clip to [0,1].
__device__ __forceinline__ float blend_ramp(float x) {
    if (!(x < 1.f)) return 1.f;
    if (x <= 0.f) return 0.f;
    float a = x * kPiHalf;
    float a2 = a * a;
    // sin(a), a in [0, pi/2], odd Taylor polynomial through a^13 (|err| < 7e-10)
    float s = fmaf(a2, 1.6059043836821613e-10f, -2.5052108385441720e-08f);
    s = fmaf(s, a2, 2.7557319223985893e-06f);
    s = fmaf(s, a2, -1.9841269841269841e-04f);
    s = fmaf(s, a2, 8.3333333333333333e-03f);
    s = fmaf(s, a2, -1.6666666666666666e-01f);
    s = fmaf(s * a2, a, a);
    // The reference rounds cos((1-x)pi) to float32 before the "+1, /2", which quantises the
    // ramp to multiples of 2^-25 near 0 (and makes weights below 2^-26 exactly 0 -- e.g. the
    // corner voxels of a tile).  Reproduce that rounding: c = fl(2w - 1), w' = (c + 1) / 2.
    const float c = fmaf(2.f, s * s, -1.f);
    return (c + 1.f) * 0.5f;
}

// Blend weight of one view at support-grid coordinates (weights.py:475-509):
// linear interpolation of the 5^n table (cval 0 outside [0,4]) then the ramp.
template <bool LDS>
__device__ __forceinline__ float blend_weight(const float* __restrict__ tab, int wnz, double cz, double cy, double cx) {
    const double zmax = (double)(wnz - 1);
    if (cz < 0.0 || cz > zmax || cy < 0.0 || cy > 4.0 || cx < 0.0 || cx > 4.0) return 0.f;
    double fz_ = floor(cz), fy_ = floor(cy), fx_ = floor(cx);
    int iz = (int)fz_, iy = (int)fy_, ix = (int)fx_;
    float wz = (float)(cz - fz_), wy = (float)(cy - fy_), wx = (float)(cx - fx_);
    int iz1 = second_tap(iz, wnz), iy1 = second_tap(iy, 5), ix1 = second_tap(ix, 5);
    int r00 = (iz * 5 + iy) * 5, r01 = (iz * 5 + iy1) * 5, r10 = (iz1 * 5 + iy) * 5, r11 = (iz1 * 5 + iy1) * 5;
    float ux = 1.f - wx, uy = 1.f - wy, uz = 1.f - wz;
    float a00 = fmaf(tab[r00 + ix1], wx, tab[r00 + ix] * ux);
    float a01 = fmaf(tab[r01 + ix1], wx, tab[r01 + ix] * ux);
    float a10 = fmaf(tab[r10 + ix1], wx, tab[r10 + ix] * ux);
    float a11 = fmaf(tab[r11 + ix1], wx, tab[r11 + ix] * ux);
    float b0 = fmaf(a01, wy, a00 * uy);
    float b1 = fmaf(a11, wy, a10 * uy);
    return blend_ramp(fmaf(b1, wz, b0 * uz));
}

// Weighted-average accumulator with an exact single-contributor state.
// The reference normalises first (w/sum(w), weights.py:325-345) and then sums v*w (_core.py:92-94):
// a voxel seen by ONE view gets weight w/w == 1 and comes out as v exactly (or 0 if w == 0).
// (acc, den) encodes: den == +0 -> empty; signbit(den) -> single view so far (acc = v, |den| = w);
// den > 0 -> two or more views (acc = sum w*v, den = sum w).
__device__ __forceinline__ void wa_update(float& acc, float& den, float w, float v) {
    const float dabs = fabsf(den);
    if (signbit(den)) {
        if (dabs == 0.f) { acc = v; den = -w; }
        else { acc = fmaf(w, v, acc * dabs); den = dabs + w; }
    } else if (den == 0.f) {
        acc = v;
        den = -w;
    } else {
        acc = fmaf(w, v, acc);
        den += w;
    }
}
__device__ __forceinline__ float wa_result(float acc, float den) {
    if (signbit(den)) return (den < 0.f) ? acc : 0.f;
    return (den > 0.f) ? acc / den : 0.f;
}

template <typename TOut> __device__ __forceinline__ TOut cast_out(float v);
template <> __device__ __forceinline__ float cast_out<float>(float v) { return v; }
// np.nan_to_num(...).astype(uint16/uint8): C truncation toward zero (_core.py:1713)
template <> __device__ __forceinline__ unsigned short cast_out<unsigned short>(float v) { return (unsigned short)(int)v; }
template <> __device__ __forceinline__ unsigned char cast_out<unsigned char>(float v) { return (unsigned char)(int)v; }

template <typename TOut> struct Vec4;
template <> struct Vec4<float> { typedef float4 type; };
template <> struct Vec4<unsigned short> { typedef ushort4 type; };
template <> struct Vec4<unsigned char> { typedef uchar4 type; };

template <typename TOut>
__device__ __forceinline__ void store_row4(TOut* out, long long row, int x0, int ox, const float r[4]) {
    if (x0 + kVPT <= ox && ((row + x0) & 3) == 0) {
        typename Vec4<TOut>::type v4;
        v4.x = cast_out<TOut>(r[0]);
        v4.y = cast_out<TOut>(r[1]);
        v4.z = cast_out<TOut>(r[2]);
        v4.w = cast_out<TOut>(r[3]);
        *reinterpret_cast<typename Vec4<TOut>::type*>(out + row + x0) = v4;
    } else {
#pragma unroll
        for (int j = 0; j < kVPT; ++j)
            if (x0 + j < ox) out[row + x0 + j] = cast_out<TOut>(r[j]);
    }
}
