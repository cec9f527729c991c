// mvs_intensity_dev.h -- the arithmetic of tile intensity harmonisation (mvs_intensity.hip), host/device: the one cell rule that
// the planner (intensity.plan_records), both kernels and the oracle share, and the float32 arithmetic of the apply kernel.
#pragma once
#include <hip/hip_runtime.h>

#ifndef MVS_HD
#define MVS_HD __host__ __device__ __forceinline__
#endif

// Cell of the continuous pixel coordinate c along an axis of n pixels with g cells (pixel centres at integer coordinates, the
// axis spans [-0.5, n - 0.5]): clamp(floor((c + 0.5) * g / n), 0, g - 1), in double, the product before the quotient.
MVS_HD int intensity_cell(double c, int g, int n) {
    const double k = floor((c + 0.5) * (double)g / (double)n);
    return k < 0.0 ? 0 : (k > (double)(g - 1) ? g - 1 : (int)k);
}

// u + t * (v - u) in float32: three roundings (the library is built without contraction)
MVS_HD float intensity_lerp(float u, float v, float t) { return u + t * (v - u); }

// integer outputs: round half to even, saturate to [0, vmax]; a NaN becomes 0
MVS_HD float intensity_saturate(float y, float vmax) {
    const float r = rintf(y);
    return !(r >= 0.f) ? 0.f : (r > vmax ? vmax : r);
}
