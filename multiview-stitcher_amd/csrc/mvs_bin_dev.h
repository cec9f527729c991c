// mvs_bin_dev.h -- the one definition of a block mean's arithmetic (bin_mean_kernel, bin_mean_u16x2_kernel,
// bin_mean_u16x2_batch_kernel in mvs_bin.hip; the three branches of crop_bin_kernel in mvs_fuse.hip), host/device: the kernels and
// tests/native/bin_mean_host_test.cpp compile the same function.
//
//   mean_cast    sum / count in double, cast to T like numpy's astype (truncation for the integer types) ==
//                block.mean().astype(T).  A TRUE division: an integer sum (< 2^53) is exact in double, and IEEE division rounds the
//                exact quotient, so a sum that is a multiple of the count gives exactly that integer.  sum * (1.0 / count) does not:
//                the rounded reciprocal can leave the product one ulp below the integer, which the cast then truncates to k - 1
//                (first at count 49: 39,897 of the 65,536 16-bit means).
#pragma once
#include <hip/hip_runtime.h>

namespace mvs_bin {

template <typename T, typename S>
__host__ __device__ __forceinline__ T mean_cast(S sum, double count) {
    return (T)((double)sum / count);
}

}  // namespace mvs_bin
