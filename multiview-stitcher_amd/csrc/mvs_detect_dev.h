// mvs_detect_dev.h -- index arithmetic of the bead detection kernels (mvs_detect.hip), host/device: the kernels and
// tests/native/detect_host_test.cpp compile the same functions.
//
//   reflect      position p (any integer) of a line of `len` samples under scipy's mode="reflect" (d c b a | a b c d | d c b a;
//                numpy.pad's "symmetric"): as many reflections as it takes, and 0 on a line of one sample
//   window       the samples a rank filter of size n reads at position i (scipy, origin 0): [i - n / 2, i - n / 2 + n - 1], so an
//                even window reaches one sample further back than forward
#pragma once
#include <hip/hip_runtime.h>

namespace mvs_det {

__host__ __device__ __forceinline__ int reflect(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;      // inside the line: the common case costs one comparison
    if (len == 1) return 0;
    const int period = 2 * len;
    int q = p % period;
    if (q < 0) q += period;
    if (q >= len) q = period - 1 - q;
    return q;
}

__host__ __device__ __forceinline__ void window(int i, int n, int* lo, int* hi) {
    *lo = i - n / 2;
    *hi = *lo + n - 1;
}

}  // namespace mvs_det
