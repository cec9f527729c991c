// mvs_affine_mi_dev.h -- the per-sample arithmetic of the Mattes mutual-information metric of affine_registration
// (mvs_affine_joint_hist, mvs_affine_mi_gradient).  Host/device: the kernels of mvs_affine_mi.hip and
// tests/native/affine_mi_host_test.cpp compile the same functions, and tests/affine_mi_oracle.py restates them in numpy
// (float32 mode) operation by operation.  The build uses -ffp-contract=off: every * and + below rounds on its own, in the
// order written.
//
// Coordinates, the split, the interpolation and the validity rule are those of mvs_affine_reg_dev.h (mvs_ar).  On top, with
// B = n_bins, F the fixed value and v the interpolated moving value of a valid sample, all in float32:
//   fixed bin        a = clamp(floor((F - f_lo) * f_scale + 0.5), 0, B - 1)         order-0 window; f_scale = (B - 1) / (f_hi - f_lo)
//   moving bin       u = clamp((v - m_lo) * m_scale + 1.5, 1.5, B - 2.5)            m_scale = (B - 4) / (m_hi - m_lo)
//   taps             b_k = floor(u) - 1 + k, k = 0..3: inside 0..B-1 for every input (a NaN u becomes 1.5)
//   window           beta3(u - b_k), the cubic B-spline; its derivative beta3'(u - b_k) for the gradient
//   histogram weight q_k = (long long)(beta3(u - b_k) * 2^20 + 0.5): integers, so their sums do not depend on the order
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace mvs_mi {

constexpr int MIN_BINS = 8, MAX_BINS = 64;
constexpr float WEIGHT_ONE = 1048576.0f;      // 2^20: the four weights of a sample sum to this, give or take 2

__host__ __device__ __forceinline__ int fixed_bin(float F, float f_lo, float f_scale, int B) {
    const float r = floorf((F - f_lo) * f_scale + 0.5f);
    return (int)fminf(fmaxf(r, 0.f), (float)(B - 1));        // clamped as a float: no out-of-range conversion, NaN -> 0
}

__host__ __device__ __forceinline__ float moving_coord(float v, float m_lo, float m_scale, int B) {
    const float u = (v - m_lo) * m_scale + 1.5f;
    return fminf(fmaxf(u, 1.5f), (float)B - 2.5f);
}

// first tap of the window around u (u as moving_coord returns it)
__host__ __device__ __forceinline__ int first_tap(float u) { return (int)floorf(u) - 1; }

__host__ __device__ __forceinline__ float beta3(float t) {
    const float a = fabsf(t);
    if (a < 1.f) return (float)(2.0 / 3.0) + (a * a) * (0.5f * a - 1.0f);
    if (a < 2.f) {
        const float d = 2.0f - a;
        return ((d * d) * d) * (float)(1.0 / 6.0);
    }
    return 0.f;
}

__host__ __device__ __forceinline__ float beta3_prime(float t) {
    const float a = fabsf(t);
    if (a < 1.f) return t * (1.5f * a - 2.0f);
    if (a < 2.f) {
        const float d = 2.0f - a;
        return (t < 0.f ? 0.5f : -0.5f) * (d * d);
    }
    return 0.f;
}

__host__ __device__ __forceinline__ long long quantise(float w) { return (long long)(w * WEIGHT_ONE + 0.5f); }

// the four histogram weights of a sample; returns the first tap
__host__ __device__ __forceinline__ int hist_weights(float u, long long q[4]) {
    const int b0 = first_tap(u);
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = quantise(beta3(u - (float)(b0 + k)));
    return b0;
}

// w = sum_k beta3'(u - b_k) * row[b_k], in k order; row = table + a * B
__host__ __device__ __forceinline__ float gradient_weight(float u, const float* row) {
    const int b0 = first_tap(u);
    float w = beta3_prime(u - (float)b0) * row[b0];
#pragma unroll
    for (int k = 1; k < 4; ++k) w = w + beta3_prime(u - (float)(b0 + k)) * row[b0 + k];
    return w;
}

}  // namespace mvs_mi
