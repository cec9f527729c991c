// mvs_affine_reg_dev.h -- the per-sample arithmetic of the Gauss-Newton intensity registration (mvs_affine_normal_eq).
// Host/device: the walk of mvs_affine_walk_dev.h (every kernel of affine_registration) and
// tests/native/affine_reg_host_test.cpp compile the same functions, and tests/affine_reg_oracle.py restates them in numpy
// (float32 mode) operation by operation.  The build uses -ffp-contract=off: every * and + below rounds on its own, in the
// order written.
//
// One sample of the fixed grid at voxel x (centre c = (shape - 1) / 2, pose [A | t]):
//   coordinate  p_k = ((A[k][0] * d_0 + A[k][1] * d_1) + A[k][2] * d_2) + o_k      double; d = x - c, o_k = c_k + t_k
//               (2D: p_k = (A[k][0] * d_0 + A[k][1] * d_1) + o_k)
//   split       i0 = floor(p), f = (float)(p - floor(p)); inside iff p >= 0 and p < n - 1  (i0 >= 0 and i0 + 1 <= n - 1)
//   sample      float32, linear interpolation a + f * (b - a) along x, then y, then z; the gradient is the analytic derivative
//               of that interpolant built from the same differences
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace mvs_ar {

__host__ __device__ __forceinline__ double coord3(const double* a_row, double d0, double d1, double d2, double o) {
    return ((a_row[0] * d0 + a_row[1] * d1) + a_row[2] * d2) + o;
}
__host__ __device__ __forceinline__ double coord2(const double* a_row, double d0, double d1, double o) {
    return (a_row[0] * d0 + a_row[1] * d1) + o;
}

// lower tap index and fraction of coordinate p on an axis of n samples; false when a tap would fall outside (or p is NaN)
__host__ __device__ __forceinline__ bool split(double p, long long n, long long* i0, float* f) {
    if (!(p >= 0.0 && p < (double)(n - 1))) return false;
    const double fl = floor(p);
    *i0 = (long long)fl;
    *f = (float)(p - fl);
    return true;
}

__host__ __device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }
__host__ __device__ __forceinline__ float lerp_f(float a, float d, float f) { return a + f * d; }

// taps m[2 * iy + ix]; g = (d/dy, d/dx).  false when a tap is not finite.
__host__ __device__ __forceinline__ bool sample2(const float m[4], float fy, float fx, float* v, float g[2]) {
    if (!(finite_f(m[0]) && finite_f(m[1]) && finite_f(m[2]) && finite_f(m[3]))) return false;
    const float dx0 = m[1] - m[0], dx1 = m[3] - m[2];
    const float c0 = lerp_f(m[0], dx0, fx), c1 = lerp_f(m[2], dx1, fx);
    const float dy = c1 - c0;
    *v = lerp_f(c0, dy, fy);
    g[0] = dy;
    g[1] = lerp_f(dx0, dx1 - dx0, fy);
    return true;
}

// taps m[4 * iz + 2 * iy + ix]; g = (d/dz, d/dy, d/dx).  false when a tap is not finite.
__host__ __device__ __forceinline__ bool sample3(const float m[8], float fz, float fy, float fx, float* v, float g[3]) {
    bool ok = true;
    for (int i = 0; i < 8; ++i) ok = ok && finite_f(m[i]);
    if (!ok) return false;
    const float dx00 = m[1] - m[0], dx01 = m[3] - m[2], dx10 = m[5] - m[4], dx11 = m[7] - m[6];
    const float c00 = lerp_f(m[0], dx00, fx), c01 = lerp_f(m[2], dx01, fx);
    const float c10 = lerp_f(m[4], dx10, fx), c11 = lerp_f(m[6], dx11, fx);
    const float dy0 = c01 - c00, dy1 = c11 - c10;
    const float c0 = lerp_f(c00, dy0, fy), c1 = lerp_f(c10, dy1, fy);
    const float dz = c1 - c0;
    *v = lerp_f(c0, dz, fz);
    g[0] = dz;
    g[1] = lerp_f(dy0, dy1 - dy0, fz);
    const float e0 = lerp_f(dx00, dx01 - dx00, fy), e1 = lerp_f(dx10, dx11 - dx10, fy);
    g[2] = lerp_f(e0, e1 - e0, fz);
    return true;
}

// residual of the intensity model F ~ gain * v + bias
__host__ __device__ __forceinline__ float residual(float gain, float bias, float v, float F) { return (gain * v + bias) - F; }

}  // namespace mvs_ar
