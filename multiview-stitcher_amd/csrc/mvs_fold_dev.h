// mvs_fold_dev.h -- the one wave / workgroup fold of the kernels' reductions (device only).
//
// A *partial* P is a trivially copyable struct with two members:
//   void merge(const P& o)               *this is the left operand, o the right one
//   P shuffled(Shuffle sh, int off)      the partial of another lane: sh(field, off) for every field
// The order of the merges is part of the results (several tests compare bits), so it is stated here and nowhere else:
//   wave stage       offsets 32, 16, .. 1: a lane is the left operand, the lane `off` above it (Down) or lane ^ off (Xor) the right one
//   workgroup stage  the value of wave 0, then the waves 1, 2, .. in order
#pragma once
#include <hip/hip_runtime.h>

namespace mvs_fold {

struct Down {
    template <typename T> __device__ __forceinline__ T operator()(T v, int off) const { return __shfl_down(v, off, 64); }
};
struct Xor {
    template <typename T> __device__ __forceinline__ T operator()(T v, int off) const { return __shfl_xor(v, off, 64); }
};

// valid in lane 0
template <typename P>
__device__ __forceinline__ P wave_fold(P a) {
    for (int off = 32; off > 0; off >>= 1) a.merge(a.shuffled(Down(), off));
    return a;
}

// valid in every lane.  Lane 0 gets the same bits as from wave_fold: every lane whose value reaches lane 0 at the step `off` has the
// bit `off` of its number clear, where lane ^ off == lane + off -- the same operands in the same order.
template <typename P>
__device__ __forceinline__ P wave_fold_all(P a) {
    for (int off = 32; off > 0; off >>= 1) a.merge(a.shuffled(Xor(), off));
    return a;
}

// valid in thread 0; every thread of the workgroup calls it, once per kernel and partial type (the slots are not guarded by a
// leading barrier).  nwaves = waves of the workgroup when they are fewer than MAXWAVES.
template <int MAXWAVES, typename P>
__device__ __forceinline__ P block_fold(P a, int nwaves = MAXWAVES) {
    __shared__ P slot[MAXWAVES];
    a = wave_fold(a);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < nwaves; ++w) a.merge(slot[w]);
    return a;
}

// valid in every thread of a workgroup of MAXWAVES waves; the leading barrier lets a kernel call it repeatedly
template <int MAXWAVES, typename P>
__device__ __forceinline__ P block_fold_all(P a) {
    __shared__ P slot[MAXWAVES];
    a = wave_fold(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = a;
    __syncthreads();
    a = slot[0];
    for (int w = 1; w < MAXWAVES; ++w) a.merge(slot[w]);
    return a;
}

// ---- the partials that more than one file uses ----------------------------------------------------------------------------------

// minimum, maximum and number of the values seen (start: INFINITY, -INFINITY, 0)
template <typename N>
struct Range {
    float mn, mx;
    N n;
    __device__ __forceinline__ void merge(const Range& o) { mn = fminf(mn, o.mn); mx = fmaxf(mx, o.mx); n += o.n; }
    template <typename S> __device__ __forceinline__ Range shuffled(S sh, int off) const { return {sh(mn, off), sh(mx, off), sh(n, off)}; }
};

// a count and the bounding box of what was counted
template <typename N>
struct CountBox {
    N n;
    int lo[3], hi[3];
    __device__ __forceinline__ void merge(const CountBox& o) {
        n += o.n;
        for (int k = 0; k < 3; ++k) { lo[k] = min(lo[k], o.lo[k]); hi[k] = max(hi[k], o.hi[k]); }
    }
    template <typename S> __device__ __forceinline__ CountBox shuffled(S sh, int off) const {
        return {sh(n, off), {sh(lo[0], off), sh(lo[1], off), sh(lo[2], off)}, {sh(hi[0], off), sh(hi[1], off), sh(hi[2], off)}};
    }
};

// K sums of one arithmetic type
template <typename T, int K = 1>
struct Sums {
    T v[K];
    __device__ __forceinline__ void merge(const Sums& o) {
        for (int k = 0; k < K; ++k) v[k] += o.v[k];
    }
    template <typename S> __device__ __forceinline__ Sums shuffled(S sh, int off) const {
        Sums o;
        for (int k = 0; k < K; ++k) o.v[k] = sh(v[k], off);
        return o;
    }
};

template <typename T>
struct Max {
    T v;
    __device__ __forceinline__ void merge(const Max& o) { v = max(v, o.v); }
    template <typename S> __device__ __forceinline__ Max shuffled(S sh, int off) const { return {sh(v, off)}; }
};

}  // namespace mvs_fold
