// mvs_gauss.hip -- content-based fusion weights (Preibisch) on the GPU (gfx950).
//
// mvs_fuse_chunk with weights == MVS_WEIGHTS_CONTENT_BASED reproduces, per output chunk (incl. halo),
// the reference's fuse_np with weights_func=weights.content_based (src/multiview_stitcher/):
//   field_ims_t[v]  = affine_transform(view v, cval=NaN)                         fusion/_core.py:1621-1633
//   field_ws_t[v]   = blending weights * ~isnan, normalised over views           _core.py:1636-1649
//   content_based:  I[bw < 1e-7] = NaN;  F_v = NG_s2((I - NG_s1(I))^2);  F = normalise(F)   weights.py:22-74
//     NG_s(U) = gaussian(U with NaN->0) / gaussian(valid mask), NaN kept            weights.py:293-322
//     gaussian = scipy.ndimage.gaussian_filter(sigma, mode="reflect", truncate=4): separable correlate1d,
//     float64 kernel and accumulation, float32 output after every axis
//   weighted_average_fusion: A = bw * F, normalise, sum_v I_v * A_v               _core.py:85-94
//   trim halo, nan_to_num, astype(input dtype)                                     _core.py:1687-1713
// The halo (2*sigma_2, weights.py:22) and the chunk grid are the caller's (fusion.fuse mirrors the
// reference's), because the reflect boundary of the Gaussians makes results depend on the chunking.
//
// Round 3: every view is processed on its BOX -- the part of the halo chunk it can reach (exact in-bounds interval for
// translations, bounding box of the mapped slab otherwise) -- instead of on the whole chunk.  Outside its box a view is NaN,
// i.e. value 0 and mask 0 in both terms of the NaN-aware Gaussian, so a line filter over the box with ZEROS beyond the ends
// that lie inside the chunk and the chunk's own REFLECTION beyond the ends that coincide with the chunk's border yields,
// at every voxel of the box, the sums the reference forms over the whole chunk line (same taps, same order: the taps that
// are skipped are exact zeros).  A chunk of a tile grid sees one view nearly whole and up to seven by a corner or a face:
// 1.3 chunk volumes of filter work instead of 8 on the 2x2x2 probe.
#include "mvs_cb_plan.h"
#include "mvs_fold_dev.h"
#include "mvs_fuse_dev.h"
#include "mvs_fuse_tr.h"
#include "mvs_fuse_chunk_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

namespace {

inline int grid_for(long long n) { return (int)std::min<long long>((n + 255) / 256, 256 * 16); }

struct Shape3 { int nz, ny, nx; };

__device__ __forceinline__ long long box_index(const CbBox& B, int z, int y, int x) {
    const int bz = z - B.lo[0], by = y - B.lo[1], bx = x - B.lo[2];
    if ((unsigned)bz >= (unsigned)B.n[0] || (unsigned)by >= (unsigned)B.n[1] || (unsigned)bx >= (unsigned)B.n[2]) return -1;
    return B.off + ((long long)bz * B.n[1] + by) * B.n[2] + bx;
}

// bw[v] *= ~isnan(I[v]) ; then normalise over views: wsum = sum_v bw (float32, view order), 0 -> 1.  One thread per chunk
// voxel; a view takes part where its box holds the voxel (elsewhere it is NaN with weight 0: adds an exact 0).
__global__ void mask_normalize_kernel(float* __restrict__ bw, const float* __restrict__ im, const CbBox* __restrict__ boxes, int nviews, Shape3 S) {
    const long long n = (long long)S.nz * S.ny * S.nx;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % S.nx);
        const long long t = i / S.nx;
        const int y = (int)(t % S.ny), z = (int)(t / S.ny);
        float wsum = 0.f;
        for (int v = 0; v < nviews; ++v) {
            const long long k = box_index(boxes[v], z, y, x);
            if (k < 0) continue;
            float w = bw[k];
            const float xv = im[k];
            if (xv != xv) w = 0.f;   // w * False
            bw[k] = w;
            wsum += w;               // np.nansum over axis 0 adds view by view in float32
        }
        if (wsum == 0.f) wsum = 1.f;
        for (int v = 0; v < nviews; ++v) {
            const long long k = box_index(boxes[v], z, y, x);
            if (k >= 0) bw[k] /= wsum;
        }
    }
}

// The same for chunks seen by at most 8 views (every tile grid): the view loop is unrolled, a view's pool index is worked out once
// per voxel in 32-bit arithmetic and kept in a register, and the masked weight is written once, already normalised (the general
// kernel stores it, re-reads it and divides in place: 20 instead of 12 bytes per view and voxel).
__device__ __forceinline__ int box_index32(const CbBox32& B, int z, int y, int x) {
    const int bz = z - B.lo[0], by = y - B.lo[1], bx = x - B.lo[2];
    if ((unsigned)bz >= (unsigned)B.n[0] || (unsigned)by >= (unsigned)B.n[1] || (unsigned)bx >= (unsigned)B.n[2]) return -1;
    return B.off + (bz * B.n[1] + by) * B.n[2] + bx;
}
// nan_masked (fast path, mvs_gauss_fast.inc): the view itself becomes NaN where its normalised weight is < 1e-7 (weights.py:54-55), so
// that "valid" is "finite" for every later pass; the final sum skips such a view there either way (its F is NaN).
__global__ __launch_bounds__(256) void mask_normalize8_kernel(float* __restrict__ bw, float* __restrict__ im, CbBoxes8 BX, int nviews, Shape3 S, int nan_masked) {
    const long long n = (long long)S.nz * S.ny * S.nx;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % S.nx);
        const long long t = i / S.nx;
        const int y = (int)(t % S.ny), z = (int)(t / S.ny);
        int kk[8];
        float w[8];
        float wsum = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            kk[v] = v < nviews ? box_index32(BX.b[v], z, y, x) : -1;
            w[v] = 0.f;
            if (kk[v] >= 0) {
                w[v] = bw[kk[v]];
                const float xv = im[kk[v]];
                if (xv != xv) w[v] = 0.f;      // w * False
                wsum += w[v];                  // np.nansum over axis 0 adds view by view in float32
            }
        }
        if (wsum == 0.f) wsum = 1.f;
#pragma unroll
        for (int v = 0; v < 8; ++v)
            if (kk[v] >= 0) {
                const float wn = w[v] / wsum;
                bw[kk[v]] = wn;
                if (nan_masked && wn < 1e-7f) im[kk[v]] = NAN;
            }
    }
}

// A = I with NaN where the (normalised) blending weight < 1e-7 (weights.py:54-55); V0 = A with NaN -> 0; M = valid mask
__global__ void prep_kernel(const float* __restrict__ im, const float* __restrict__ bw, long long n, float* __restrict__ A,
                            float* __restrict__ V0, float* __restrict__ M) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float x = im[i];
        if (bw[i] < 1e-7f) x = NAN;
        const bool ok = (x == x);
        A[i] = x;
        V0[i] = ok ? x : 0.f;
        M[i] = ok ? 1.f : 0.f;
    }
}

// Position `p` of a box line (box-relative, any integer) in the chunk's line of length `full`, reflected at the chunk's ends
// (scipy mode="reflect": d c b a | a b c d | d c b a), back in box coordinates: -1 when it falls outside the box (a zero).
__device__ __forceinline__ int box_reflect(int p, int b0, int len, int full) {
    int q = p + b0;
    if (full == 1) q = 0;
    else {
        const int period = 2 * full;
        q %= period; if (q < 0) q += period; if (q >= full) q = period - 1 - q;
    }
    q -= b0;
    return ((unsigned)q < (unsigned)len) ? q : -1;
}

// ---- the valid mask of a view as a BOX (round 5) ------------------------------------------------------------------------------
// The mask term of the NaN-aware Gaussian filters M = (view is finite) & !(normalised blending weight < 1e-7).  For an integer tile
// under a whole-pixel translation that set is a box -- the part of the tile inside the chunk minus the outermost layer, where the
// blend weight vanishes -- and a separable indicator mz(z) my(y) mx(x) stays separable under the line filters: after the z pass
// the array is A(z) my(y) mx(x), after the y pass B(z, y) mx(x), with A = float32(filter of mz) and B = float32(filter of A(z) my)
// -- the very sums the line kernels form (same order, same fused multiply-adds, same float32 roundings), on 1-D and 2-D tables
// instead of 3-D arrays.  So: (1) cb_mask_bbox_kernel counts the valid voxels of every view's box and takes their bounding box;
// count == volume of the bounding box <=> the mask IS that box (checked on the device, per view and chunk: nothing is assumed);
// (2) cb_mask_table_kernel builds A and B for both filters; (3) the mask workgroups of the z / y passes return at once, and the
// x pass -- which divides value by mask -- stages B(z, y) mx(x) instead of loading a filtered mask.  A view whose mask is not a
// box (rotated views, float tiles holding NaNs) keeps the filtered path, decided by the same record.  Per view and filter two
// of the three mask passes disappear: a third of all line-filter work and of its HBM traffic.
struct CbMaskRec { unsigned long long cnt; int lo[3]; int hi[3]; };      // lo / hi: box-local bounding box of the valid voxels
static_assert(sizeof(CbMaskRec) == 32, "CbMaskRec layout");
__device__ __forceinline__ bool cb_mask_is_box(const CbMaskRec& r) {
    if (r.cnt == 0ull) return false;
    const unsigned long long vol = (unsigned long long)(r.hi[0] - r.lo[0] + 1) * (unsigned long long)(r.hi[1] - r.lo[1] + 1) *
                                   (unsigned long long)(r.hi[2] - r.lo[2] + 1);
    return vol == r.cnt;
}

// blockIdx.y = view; the workgroups of a view stride over its box
__global__ __launch_bounds__(256) void cb_mask_bbox_kernel(const float* __restrict__ im, const float* __restrict__ bw, CbBoxes8 BX, CbMaskRec* __restrict__ recs) {
    const CbBox32 B = BX.b[blockIdx.y];
    const long long n = (long long)B.n[0] * B.n[1] * B.n[2];
    mvs_fold::CountBox<unsigned long long> a = {0, {0x7fffffff, 0x7fffffff, 0x7fffffff}, {-1, -1, -1}};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float x = im[B.off + i], w = bw[B.off + i];
        if ((x == x) && !(w < 1e-7f)) {
            const int bx = (int)(i % B.n[2]);
            const long long t = i / B.n[2];
            const int by = (int)(t % B.n[1]), bz = (int)(t / B.n[1]);
            a.merge({1, {bz, by, bx}, {bz, by, bx}});
        }
    }
    a = mvs_fold::block_fold<4>(a);
    if (threadIdx.x == 0 && a.n) {      // one set of atomics per workgroup (a few hundred per view)
        CbMaskRec* r = recs + blockIdx.y;
        atomicAdd(&r->cnt, a.n);
        for (int k = 0; k < 3; ++k) { atomicMin(&r->lo[k], a.lo[k]); atomicMax(&r->hi[k], a.hi[k]); }
    }
}

// tables of one view and filter: B(z, y) (box-local, n[0] x n[1] floats).  grid = (n[0] max over views, views, 2 filters)
__global__ __launch_bounds__(256) void cb_mask_table_kernel(const CbMaskRec* __restrict__ recs, CbBoxes8 BX, Shape3 S, int ndim, int r1,
                                                            const double* __restrict__ fw1, int r2, const double* __restrict__ fw2,
                                                            float* __restrict__ tables, const long long* __restrict__ table_off) {
    const int v = blockIdx.y, f = blockIdx.z, z = blockIdx.x;
    const CbBox32 B = BX.b[v];
    if (z >= B.n[0] || B.n[1] <= 0 || B.n[2] <= 0) return;
    const CbMaskRec R = recs[v];
    if (!cb_mask_is_box(R)) return;
    const int radius = f ? r2 : r1;
    const double* fw = f ? fw2 : fw1;
    // A(z): the z pass over the indicator of [lo0, hi0] (3D); the raw indicator itself when there is no z pass (2D: n[0] == 1)
    float Az;
    if (ndim == 3) {
        auto mz = [&](int p) -> double {
            int q = p;
            if ((unsigned)q >= (unsigned)B.n[0]) q = box_reflect(p, B.lo[0], B.n[0], S.nz);
            return (q >= 0 && q >= R.lo[0] && q <= R.hi[0]) ? 1.0 : 0.0;
        };
        double acc = mz(z) * fw[radius];
        for (int j = radius; j >= 1; --j) acc = fma(mz(z - j) + mz(z + j), fw[radius - j], acc);
        Az = (float)acc;
    } else {
        Az = (z >= R.lo[0] && z <= R.hi[0]) ? 1.f : 0.f;
    }
    float* out = tables + table_off[v * 2 + f] + (long long)z * B.n[1];
    const double a = (double)Az;
    for (int y = threadIdx.x; y < B.n[1]; y += blockDim.x) {
        auto my = [&](int p) -> double {
            int q = p;
            if ((unsigned)q >= (unsigned)B.n[1]) q = box_reflect(p, B.lo[1], B.n[1], S.ny);
            return (q >= 0 && q >= R.lo[1] && q <= R.hi[1]) ? a : 0.0;
        };
        double acc = my(y) * fw[radius];
        for (int j = radius; j >= 1; --j) acc = fma(my(y - j) + my(y + j), fw[radius - j], acc);
        out[y] = (float)acc;
    }
}

// scipy.ndimage.correlate1d with a symmetric kernel along one axis, mode="reflect": double accumulation in
// scipy's order (centre tap, then pairs from the farthest to the nearest), float32 output.  The array is a box of the chunk:
// b0 = its first position along the axis inside the chunk line, full = the chunk line's length.
__global__ __launch_bounds__(256) void gauss1d_kernel(const float* __restrict__ src, float* __restrict__ dst, Shape3 S, int axis,
                                                      int radius, const double* __restrict__ fw, int b0, int full) {
    const long long n = (long long)S.nz * S.ny * S.nx;
    const int dims[3] = {S.nz, S.ny, S.nx};
    const long long strides[3] = {(long long)S.ny * S.nx, S.nx, 1};
    const int len = dims[axis];
    const long long st = strides[axis];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % S.nx);
        const long long t = i / S.nx;
        const int y = (int)(t % S.ny), z = (int)(t / S.ny);
        const int pos = (axis == 0) ? z : (axis == 1) ? y : x;
        const long long base = i - (long long)pos * st;
        double acc = (double)src[i] * fw[radius];
        for (int j = radius; j >= 1; --j) {
            const int p0 = box_reflect(pos - j, b0, len, full), p1 = box_reflect(pos + j, b0, len, full);
            const double a0 = p0 >= 0 ? (double)src[base + (long long)p0 * st] : 0.0;
            const double a1 = p1 >= 0 ? (double)src[base + (long long)p1 * st] : 0.0;
            acc += (a0 + a1) * fw[radius - j];
        }
        dst[i] = (float)acc;
    }
}

// The same filter with the lines staged in LDS: a workgroup takes T adjacent lines, copies them (+ the reflected halo
// of `radius` samples on both sides) into LDS once and every output reads its 2 * radius + 1 taps from there -- no
// index arithmetic, no reflection and no global load per tap (the tap-by-tap kernel above spends its time there: the
// sigma = 11 filter has 89 taps).  Same accumulation order, same rounding.  LDS layout [pos + radius][line], line
// pitch T + 1 (odd) so that both access directions are bank-conflict free.
__global__ __launch_bounds__(256) void gauss1d_lds_kernel(const float* __restrict__ src, float* __restrict__ dst, GaussLines L, int radius,
                                                          const double* __restrict__ fw, int pos_fastest) {
    extern __shared__ float sl[];
    const int T = L.T, TP = T + 1, len = L.len;
    const long long l0 = (long long)blockIdx.x * T;
    const int nl = (int)min((long long)T, L.n_lines - l0);
    const int total = T * len;
    // ---- stage the lines; note whether every sample of the tile has the same bits as its first one ----
    const float first = src[(l0 / L.inner) * L.outer_stride + (l0 % L.inner)];
    int same = 1;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        int line, pos;
        if (pos_fastest) { line = idx / len; pos = idx - line * len; }
        else { pos = idx / T; line = idx - pos * T; }
        float v = 0.f;
        if (line < nl) {
            const long long l = l0 + line;
            v = src[(l / L.inner) * L.outer_stride + (l % L.inner) + (long long)pos * L.stride];
            same &= (__float_as_uint(v) == __float_as_uint(first)) ? 1 : 0;
        }
        sl[(pos + radius) * TP + line] = v;
    }
    // (only when the box line IS the chunk line -- zeros beyond an end would change the sums -- or the constant is 0)
    const bool whole = (L.b0 == 0 && L.len == L.full) || __float_as_uint(first) == 0u;
    if (__syncthreads_and(same) && whole) {
        // a constant tile (outside a view's footprint: value and mask 0; deep inside it: mask 1, and the constants the
        // earlier axes made of those): every output is the same sum, evaluated once in the order of the general path
        double acc = (double)first * fw[radius];
        for (int j = radius; j >= 1; --j) acc = fma((double)first + (double)first, fw[radius - j], acc);
        const float r = (float)acc;
        for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
            int line, pos;
            if (pos_fastest) { line = idx / len; pos = idx - line * len; }
            else { pos = idx / T; line = idx - pos * T; }
            if (line >= nl) continue;
            const long long l = l0 + line;
            dst[(l / L.inner) * L.outer_stride + (l % L.inner) + (long long)pos * L.stride] = r;
        }
        return;
    }
    // ---- halo: the chunk line reflected at the chunk's ends (d c b a | a b c d | d c b a), zeros where that falls outside
    // the box ----
    for (int idx = threadIdx.x; idx < 2 * radius * T; idx += blockDim.x) {
        const int h = idx / T, line = idx - h * T;
        const int p = (h < radius) ? (h - radius) : (len + h - radius);      // position outside [0, len)
        const int q = box_reflect(p, L.b0, len, L.full);
        sl[(p + radius) * TP + line] = (q >= 0) ? sl[(q + radius) * TP + line] : 0.f;
    }
    __syncthreads();
    // ---- filter: a thread produces K consecutive outputs of one line.  Pair j of output k needs the samples k - j and
    // k + j: over the K outputs these are two windows of K samples that slide by one (in opposite directions) when j
    // drops by one, so every step costs two LDS reads and two conversions for K (add, multiply, add) triples -- the
    // tap-by-tap form read and converted 2 (2 r + 1) samples per output and was bound by exactly that.  The windows
    // rotate through fixed registers (the j loop is unrolled K-fold); per output the order of operations is scipy's, with
    // the multiply-add fused (one rounding less in float64, 1e-16 relative: invisible after the float32 store). ----
    constexpr int K = 8;
    const int nblk = (len + K - 1) / K;
    const int qmax = len - 1 + 2 * radius;                        // last staged row of the LDS array
    for (int idx = threadIdx.x; idx < T * nblk; idx += blockDim.x) {
        const int blk = idx / T, line = idx - blk * T;
        if (line >= nl) continue;
        const int p0 = blk * K;
        const float* c = sl + line;                                // sample at position q: c[(q + radius) * TP]
        double PA[K], PB[K], acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            PA[k] = (double)c[min(p0 + k, qmax) * TP];                                  // position p0 + k - radius
            PB[k] = (double)c[min(p0 + k + 2 * radius, qmax) * TP];                     // position p0 + k + radius
            acc[k] = (double)c[min(p0 + k + radius, qmax) * TP] * fw[radius];
        }
        for (int jb = radius; jb >= 1; jb -= K) {
#pragma unroll
            for (int s = 0; s < K; ++s) {
                const int j = jb - s;
                if (j < 1) break;
                const double w = fw[radius - j];
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] = fma(PA[(k + s) % K] + PB[(k - s + K) % K], w, acc[k]);
                // windows of pair j - 1: one new sample each (positions p0 + K - 1 - (j - 1) and p0 + (j - 1))
                PA[s % K] = (double)c[min(p0 + K - j + radius, qmax) * TP];
                PB[(K - 1 - s) % K] = (double)c[(p0 + j - 1 + radius) * TP];
            }
        }
        const long long l = l0 + line;
        const long long obase = (l / L.inner) * L.outer_stride + (l % L.inner) + (long long)p0 * L.stride;
        if (L.stride == 1 && p0 + K <= len && ((obase & 3) == 0)) {
            float4* o4 = reinterpret_cast<float4*>(dst + obase);
            o4[0] = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
            o4[1] = make_float4((float)acc[4], (float)acc[5], (float)acc[6], (float)acc[7]);
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (p0 + k < len) dst[obase + (long long)k * L.stride] = (float)acc[k];
        }
    }
}

// ---- the value line and the mask line of a NaN-aware Gaussian in ONE launch (round 4) -----------------------------------------
// NG_s(U) = gaussian(U, NaN -> 0) / gaussian(valid mask): both filters read the same voxels, so a workgroup stages the T lines of
// BOTH arrays, filters both and -- on the last axis -- divides them on the spot.  What no longer travels through HBM:
//   * prep_kernel's three arrays (A, V0, M): the first pass derives value and mask from the resampled view and its normalised
//     blending weight itself (SRC_PREP; SRC_VMASK for the second filter, whose value input is the squared deviation);
//   * the separate finish kernels: the last pass of the first filter stores (A - VV / WW)^2 with NaN -> 0 (DST_SQ), the last pass
//     of the second one F = VV / WW with NaN where A is NaN (DST_F), A recomputed from the view at the output voxel;
//   * half of the launches (6 instead of 12 line passes per view) and the second staging of every line set.
// Same arithmetic as gauss1d_lds_kernel per quantity (scipy's order, double accumulation, float32 result per axis, the
// constant-tile short cut per quantity).
struct PairIO {
    const float* a; const float* b;        // SRC_AB: value / mask lines; SRC_VMASK: a = value lines
    const float* im; const float* bw;      // resampled view and normalised blending weight (SRC_PREP / SRC_VMASK / DST_SQ / DST_F)
    float* oa; float* ob;                  // DST_AB: both results; DST_SQ / DST_F: oa = the single result
    int src, dst;
    const CbMaskRec* rec;                  // the view's mask record (NULL: the mask is always filtered) ...
    const float* mtab;                     // ... and its table B(z, y) for this filter (cb_mask_table_kernel)
};

__device__ __forceinline__ float cb_valid_value(const PairIO& P, long long i) {      // A: the view with NaN where bw < 1e-7
    float x = P.im[i];
    if (P.bw[i] < 1e-7f) x = NAN;
    return x;
}

// SPLIT: the passes that are not the last of their filter need no coupling between the two quantities (DST_AB), so a workgroup
// takes ONE of them (blockIdx.y: 0 value, 1 mask) and stages twice as many lines in the same LDS (T = 32: lines along y / z then
// move in 128-byte pieces instead of 64-byte ones); still one launch per pass.
#ifndef MVS_CB_NB
#define MVS_CB_NB 8      // samples a thread requests back to back while staging (memory-level parallelism of a workgroup)
#endif
template <int SRC, int DST, bool SPLIT>
__global__ __launch_bounds__(256) void gauss1d_pair_kernel(PairIO P, GaussLines L, int radius, const double* __restrict__ fw, int pos_fastest) {
    static_assert(!SPLIT || DST == DST_AB, "split passes store both quantities as they are");
    extern __shared__ float sl[];
    // T is a power of two (host: cb_pair_T / cb_split_T), so (line, position) come out of shifts and masks; the lines' first elements
    // are worked out once per workgroup (one 64-bit division per LINE instead of two per staged and stored SAMPLE)
    constexpr int NQ = SPLIT ? 1 : 2;
    const int qs = SPLIT ? (int)blockIdx.y : 0;       // SPLIT: the quantity of this workgroup
    // the view's mask is a box (see cb_mask_bbox_kernel): its z / y passes are tables, the x pass stages B(z, y) mx(x)
    bool mbox = false;
    int mx0 = 0, mx1 = -1;
    if (P.rec) {
        const CbMaskRec R = *P.rec;
        mbox = cb_mask_is_box(R);
        mx0 = R.lo[2]; mx1 = R.hi[2];
    }
    if (SPLIT && qs == 1 && mbox) return;             // (uniform: the whole workgroup)
    const int T = L.T, TP = T + 1, len = L.len, lt = 31 - __clz(T);
    const int span = len + 2 * radius;
    float* sq[2] = {sl, sl + (SPLIT ? 0 : (size_t)(span + kGaussK) * TP)};      // (kGaussK spare rows behind each array: see the filter loop)
    __shared__ long long lbase[32];
    const long long l0 = (long long)blockIdx.x * T;
    const int nl = (int)min((long long)T, L.n_lines - l0);
    if ((int)threadIdx.x < T) {
        const long long l = min(l0 + threadIdx.x, L.n_lines - 1);
        lbase[threadIdx.x] = (l / L.inner) * L.outer_stride + (l % L.inner);
    }
    __syncthreads();
    // raw loads first, interpretation afterwards: a batch of samples is requested without any control flow in between.
    // SPLIT: two loads from X / Y -- the array itself twice where the quantity is stored as it is (value of SRC_AB / SRC_VMASK,
    // mask of SRC_AB), the view and its blending weight where it is derived from them.
    const bool direct = SPLIT && (SRC == SRC_AB || (SRC == SRC_VMASK && qs == 0));
    const float* X = !SPLIT ? nullptr : (SRC == SRC_AB ? (qs ? P.b : P.a) : (direct ? P.a : P.im));
    const float* Y = !SPLIT ? nullptr : (direct ? X : P.bw);
    auto load_raw = [&](long long i, float& r0, float& r1, float& r2, auto one_array) {
        if constexpr (SPLIT) { r0 = X[i]; r1 = decltype(one_array)::value ? r0 : Y[i]; r2 = 0.f; }
        else if constexpr (SRC == SRC_AB) { r0 = P.a[i]; r1 = mbox ? 0.f : P.b[i]; r2 = 0.f; }
        else if constexpr (SRC == SRC_PREP) { r0 = P.im[i]; r1 = P.bw[i]; r2 = 0.f; }
        else { r0 = P.im[i]; r1 = P.bw[i]; r2 = P.a[i]; }
    };
    auto interpret = [&](float r0, float r1, float r2, float& v, float& m) {      // SPLIT: the workgroup's quantity comes back in v
        if constexpr (SRC == SRC_AB) { v = r0; m = r1; }
        else {
            const bool ok = (r0 == r0) && !(r1 < 1e-7f);      // A = the view with NaN where bw < 1e-7
            m = ok ? 1.f : 0.f;
            v = (SRC == SRC_PREP) ? (ok ? r0 : 0.f) : r2;
            if constexpr (SPLIT) v = direct ? r0 : (qs ? m : v);
        }
    };
    // ---- stage the lines; note per quantity whether every sample has the bits of the first one ----
    float first[2];
    {
        float r0, r1, r2;
        load_raw(lbase[0], r0, r1, r2, std::false_type{});
        interpret(r0, r1, r2, first[0], first[1]);
        if constexpr (!SPLIT && SRC == SRC_AB) {
            if (mbox) first[1] = (0 >= mx0 && 0 <= mx1) ? P.mtab[l0] : 0.f;
        }
    }
    int same0 = 1, same1 = 1;
    // A workgroup is a short dependent chain (stage -> filter -> store) and only a few of them fit a CU, so the staging loop
    // must not pay one memory round trip per sample: the loads of NB samples are issued back to back before the first of them
    // is written to LDS.
    constexpr int NB = MVS_CB_NB;
    const int per_line = pos_fastest ? (int)blockDim.x : ((int)blockDim.x >> lt);      // positions a sweep of the workgroup covers per line
    const int my_line = pos_fastest ? 0 : (int)(threadIdx.x & (T - 1));
    const int my_pos0 = pos_fastest ? (int)threadIdx.x : (int)(threadIdx.x >> lt);
    const int sweeps = (len + per_line - 1) / per_line;
    const int n_my = pos_fastest ? sweeps * T : sweeps;             // samples of this thread: (sweep[, line]) pairs
    auto stage = [&](auto one_array) __attribute__((always_inline)) {
    for (int b0 = 0; b0 < n_my; b0 += NB) {
        float q0[NB], q1[NB], q2[NB];
        int bl[NB], bp[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int e = b0 + u;
            // pos_fastest: e = line * sweeps + sweep (threads run along a line); else e = sweep (threads run across the lines)
            const int line = pos_fastest ? e / sweeps : my_line;
            const int sweep = pos_fastest ? e - line * sweeps : e;
            const int pos = my_pos0 + sweep * per_line;
            bl[u] = line; bp[u] = pos;
            // (clamped address: the load itself is unconditional, what it returns is discarded below when out of range)
            load_raw(lbase[min(line, nl - 1)] + (long long)min(pos, len - 1) * L.stride, q0[u], q1[u], q2[u], one_array);
            if constexpr (!SPLIT && SRC == SRC_AB) {
                if (mbox) q1[u] = P.mtab[l0 + min(line, nl - 1)];      // (requested with the batch: the table entry of line l = (z, y))
            }
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int e = b0 + u;
            if (e < n_my && bp[u] < len && bl[u] < T) {
                float v = 0.f, m = 0.f;
                if (bl[u] < nl) {
                    interpret(q0[u], q1[u], q2[u], v, m);
                    if constexpr (!SPLIT && SRC == SRC_AB) {
                        if (mbox) m = (bp[u] >= mx0 && bp[u] <= mx1) ? q1[u] : 0.f;      // B(z, y) mx(x)
                    }
                    same0 &= (__float_as_uint(v) == __float_as_uint(first[0])) ? 1 : 0;
                    if (!SPLIT) same1 &= (__float_as_uint(m) == __float_as_uint(first[1])) ? 1 : 0;
                }
                sq[0][(bp[u] + radius) * TP + bl[u]] = v;
                if (!SPLIT) sq[1][(bp[u] + radius) * TP + bl[u]] = m;
            }
        }
    }
    };
    // (a quantity stored as it is needs ONE array: the second load of the general form would only occupy a slot of the batch)
    if (direct) stage(std::true_type{});
    else stage(std::false_type{});
    const bool box_is_line = (L.b0 == 0 && L.len == L.full);
    // (__syncthreads_or reduces the TRUTH of its argument, not its bits: one reduction per quantity)
    const int varies0 = __syncthreads_or(same0 ? 0 : 1);
    const int varies1 = SPLIT ? 1 : __syncthreads_or(same1 ? 0 : 1);
    bool cst[2];
    cst[0] = !varies0 && (box_is_line || __float_as_uint(first[0]) == 0u);
    cst[1] = !SPLIT && !varies1 && (box_is_line || __float_as_uint(first[1]) == 0u);
    float cval[2] = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (cst[q]) {
            double acc = (double)first[q] * fw[radius];
            for (int j = radius; j >= 1; --j) acc = fma((double)first[q] + (double)first[q], fw[radius - j], acc);
            cval[q] = (float)acc;
        }
    // ---- halo of the quantities that are filtered: chunk line reflected at the chunk's ends, zeros where that leaves the box ----
    for (int idx = threadIdx.x; idx < 2 * radius * T; idx += blockDim.x) {
        const int h = idx >> lt, line = idx & (T - 1);
        const int p = (h < radius) ? (h - radius) : (len + h - radius);
        const int q = box_reflect(p, L.b0, len, L.full);
#pragma unroll
        for (int k = 0; k < NQ; ++k)
            if (!cst[k]) sq[k][(p + radius) * TP + line] = (q >= 0) ? sq[k][(q + radius) * TP + line] : 0.f;
    }
    __syncthreads();
    // ---- filter: K consecutive outputs of one line per thread (the scheme of gauss1d_lds_kernel).  What differs is how a step
    // is fed: the windows' new samples come from two LDS pointers that move by one row per pair (no index arithmetic, no clamp:
    // the arrays end in K spare rows, whatever they hold only reaches outputs beyond the line's end, which are not stored), the
    // weights of K pairs are fetched together, and the K-pair blocks of the loop are free of branches, so that the reads and
    // conversions of a pair overlap the float64 arithmetic of the previous one. ----
    constexpr int K = kGaussK;
    const int nblk = (len + K - 1) / K;
    for (int idx = threadIdx.x; idx < T * nblk; idx += blockDim.x) {
        const int blk = idx >> lt, line = idx & (T - 1);
        if (line >= nl) continue;
        const int p0 = blk * K;
        float res[2][K];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (cst[q]) {
#pragma unroll
                for (int k = 0; k < K; ++k) res[q][k] = cval[q];
                continue;
            }
            const float* c = sq[q] + line;                  // sample at position x: c[(x + radius) * TP]
            double PA[K], PB[K], acc[K];
            const double wc = fw[radius];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                PA[k] = (double)c[(p0 + k) * TP];
                PB[k] = (double)c[(p0 + k + 2 * radius) * TP];
                acc[k] = (double)c[(p0 + k + radius) * TP] * wc;
            }
            // pair j - 1 needs one new sample per window: rows p0 + K + (radius - j) and p0 + 2 radius - 1 - (radius - j)
            const float* qa = c + (p0 + K) * TP;
            const float* qb = c + (p0 + 2 * radius - 1) * TP;
            int jb = radius;
            for (; jb >= K; jb -= K) {
                double w[K];
#pragma unroll
                for (int s = 0; s < K; ++s) w[s] = fw[radius - jb + s];
#pragma unroll
                for (int s = 0; s < K; ++s) {
#pragma unroll
                    for (int k = 0; k < K; ++k) acc[k] = fma(PA[(k + s) % K] + PB[(k - s + K) % K], w[s], acc[k]);
                    PA[s] = (double)qa[s * TP];
                    PB[K - 1 - s] = (double)qb[-s * TP];
                }
                qa += K * TP;
                qb -= K * TP;
            }
#pragma unroll
            for (int s = 0; s < K - 1; ++s) {                // the remaining jb < K pairs
                if (s >= jb) break;
                const double w = fw[radius - jb + s];
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] = fma(PA[(k + s) % K] + PB[(k - s + K) % K], w, acc[k]);
                PA[s] = (double)qa[s * TP];
                PB[K - 1 - s] = (double)qb[-s * TP];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) res[q][k] = (float)acc[k];
        }
        const long long obase = lbase[line] + (long long)p0 * L.stride;
        if constexpr (SPLIT) {
            float* o = qs ? P.ob : P.oa;
            if (L.stride == 1 && p0 + K <= len && ((obase & 3) == 0)) {
                float4* o4 = reinterpret_cast<float4*>(o + obase);
                o4[0] = make_float4(res[0][0], res[0][1], res[0][2], res[0][3]);
                o4[1] = make_float4(res[0][4], res[0][5], res[0][6], res[0][7]);
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (p0 + k < len) o[obase + (long long)k * L.stride] = res[0][k];
            }
        } else if constexpr (DST == DST_AB) {
            if (L.stride == 1 && p0 + K <= len && ((obase & 3) == 0)) {
                float4* o4 = reinterpret_cast<float4*>(P.oa + obase);
                o4[0] = make_float4(res[0][0], res[0][1], res[0][2], res[0][3]);
                o4[1] = make_float4(res[0][4], res[0][5], res[0][6], res[0][7]);
                o4 = reinterpret_cast<float4*>(P.ob + obase);
                o4[0] = make_float4(res[1][0], res[1][1], res[1][2], res[1][3]);
                o4[1] = make_float4(res[1][4], res[1][5], res[1][6], res[1][7]);
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (p0 + k < len) { P.oa[obase + (long long)k * L.stride] = res[0][k]; P.ob[obase + (long long)k * L.stride] = res[1][k]; }
            }
        } else {
            // Z = VV / WW where A is valid (weights.py:314-320); DST_SQ: (A - Z)^2 with NaN -> 0; DST_F: Z, NaN where A is NaN
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (p0 + k >= len) break;
                const long long i = obase + (long long)k * L.stride;
                const float a = cb_valid_value(P, i);
                float o;
                if constexpr (DST == DST_SQ) {
                    o = 0.f;
                    if (a == a) {
                        const float d = a - res[0][k] / res[1][k];
                        const float qd = d * d;
                        o = (qd == qd) ? qd : 0.f;
                    }
                } else {
                    o = (a == a) ? res[0][k] / res[1][k] : NAN;
                }
                P.oa[i] = o;
            }
        }
    }
}

// Z = VV / WW with WW[nan] = 1, Z[nan] = NaN (weights.py:314-320); then D = (A - Z)^2, V1 = D with NaN -> 0
__global__ void ng_finish_sq_kernel(const float* __restrict__ VV, const float* __restrict__ WW, const float* __restrict__ A,
                                    long long n, float* __restrict__ V1) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float a = A[i];
        if (a != a) { V1[i] = 0.f; continue; }
        const float zv = VV[i] / WW[i];
        const float d = a - zv;
        const float q = d * d;
        V1[i] = (q == q) ? q : 0.f;   // a finite -> q finite unless WW == 0 (cannot happen where a is valid)
    }
}

// F = VV2 / WW2 with NaN where A is NaN
__global__ void ng_finish_kernel(const float* __restrict__ VV, const float* __restrict__ WW, const float* __restrict__ A,
                                 long long n, float* __restrict__ F) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float a = A[i];
        F[i] = (a == a) ? VV[i] / WW[i] : NAN;
    }
}

template <typename TOut> __device__ __forceinline__ TOut cast_cb(float v);
template <> __device__ __forceinline__ float cast_cb<float>(float v) { return v; }
template <> __device__ __forceinline__ unsigned short cast_cb<unsigned short>(float v) { return (unsigned short)(int)v; }
template <> __device__ __forceinline__ unsigned char cast_cb<unsigned char>(float v) { return (unsigned char)(int)v; }

// normalise F over views (nansum, 0 -> 1), A = bw * Fn, normalise A, out = nansum(I * A); trimmed, nan_to_num, cast.
// Views whose box does not hold the voxel are NaN there (every term they would add is skipped by the reference's nansum).
template <typename TOut>
__global__ void cb_fuse_kernel(const float* __restrict__ im, const float* __restrict__ bw, const float* __restrict__ F,
                               const CbBox* __restrict__ boxes, int nviews, int tz, int ty, int tx, Shape3 O, TOut* __restrict__ out) {
    const long long no = (long long)O.nz * O.ny * O.nx;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < no; o += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(o % O.nx);
        const long long t = o / O.nx;
        const int y = (int)(t % O.ny), z = (int)(t / O.ny);
        float fsum = 0.f;
        for (int v = 0; v < nviews; ++v) {
            const long long k = box_index(boxes[v], z + tz, y + ty, x + tx);
            if (k < 0) continue;
            const float f = F[k];
            if (f == f) fsum += f;
        }
        if (fsum == 0.f) fsum = 1.f;
        float asum = 0.f;
        for (int v = 0; v < nviews; ++v) {
            const long long k = box_index(boxes[v], z + tz, y + ty, x + tx);
            if (k < 0) continue;
            const float a = bw[k] * (F[k] / fsum);
            if (a == a) asum += a;
        }
        if (asum == 0.f) asum = 1.f;
        float acc = 0.f;
        for (int v = 0; v < nviews; ++v) {
            const long long k = box_index(boxes[v], z + tz, y + ty, x + tx);
            if (k < 0) continue;
            const float a = bw[k] * (F[k] / fsum);
            const float p = im[k] * (a / asum);
            if (p == p) acc += p;
        }
        if (!(fabsf(acc) <= 3.4028234e38f)) acc = 0.f;
        out[o] = cast_cb<TOut>(acc);
    }
}

// cb_fuse_kernel for at most 8 views: indices, F and the weights stay in registers over the three sums (same additions in the
// same view order)
template <typename TOut>
__global__ __launch_bounds__(256) void cb_fuse8_kernel(const float* __restrict__ im, const float* __restrict__ bw, const float* __restrict__ F,
                                                       CbBoxes8 BX, int nviews, int tz, int ty, int tx, Shape3 O, TOut* __restrict__ out) {
    const long long no = (long long)O.nz * O.ny * O.nx;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < no; o += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(o % O.nx);
        const long long t = o / O.nx;
        const int y = (int)(t % O.ny), z = (int)(t / O.ny);
        int kk[8];
        float f[8], a[8];
        float fsum = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            kk[v] = v < nviews ? box_index32(BX.b[v], z + tz, y + ty, x + tx) : -1;
            f[v] = 0.f;
            if (kk[v] >= 0) {
                f[v] = F[kk[v]];
                if (f[v] == f[v]) fsum += f[v];
            }
        }
        if (fsum == 0.f) fsum = 1.f;
        float asum = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            a[v] = 0.f;
            if (kk[v] >= 0) {
                a[v] = bw[kk[v]] * (f[v] / fsum);
                if (a[v] == a[v]) asum += a[v];
            }
        }
        if (asum == 0.f) asum = 1.f;
        float acc = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v)
            if (kk[v] >= 0) {
                const float p = im[kk[v]] * (a[v] / asum);
                if (p == p) acc += p;
            }
        if (!(fabsf(acc) <= 3.4028234e38f)) acc = 0.f;
        out[o] = cast_cb<TOut>(acc);
    }
}

#include "mvs_gauss_fast.inc"

static_assert(sizeof(CbMaskRec) == 32 && sizeof(CbFastRec) == 64 && sizeof(CbPartial) == 32, "record sizes of cb_layout");
// ---- one content-based chunk: the call's arguments, its plan (mvs_cb_plan.h), the scratch pointers and what the steps derive.  The
// steps below launch on the context's stream in the order they are called; the two paths are sequences of them. ----
struct CbCall {
    MvsContext* c; const mvs_view_t* views; int n_views; const mvs_fuse_opts_t* opts; void* out;
    bool fast;                                      // the path the steps serve (set by cb_geometry)
    int dtype, ndim, cs[3], r1, r2;
    size_t es, host_bytes;
    Shape3 S, O; long long n, no;                   // the chunk with its halo, the trimmed result
    std::vector<double> w1, w2;                     // taps of both filters
    std::vector<DevView> dvs; std::vector<TrView> trv; bool tr_all;
    std::vector<CbBox> boxes; CbPool pool; CbBoxes8 bx8;
    CbFastViews VS; int Tsel[3][2][8];              // fast
    bool paired, small, mask_tables; std::vector<long long> table_off; long long table_floats;      // exact
    float *I, *BW, *F, *tmp; size_t tmp_b;          // pools; temporaries (exact: 5 / 6 of tmp_b bytes, fast: the pool T0)
    char* dblock; size_t up_bytes, rec_bytes;       // the uploaded block and what lies in it (ffw: fast, dboxes / dtable_off: exact)
    double *dfw1, *dfw2; float *ffw1, *ffw2; CbBox* dboxes; DevView* dviews_dev; char* drecs; long long* dtable_off;
    float* dtables; int4 *rows, *dmiss; double* dtabs; CbPartial* dpart; unsigned rows_grid;      // mask tables (exact), mask scan (fast)
};

void cb_begin(CbCall& K, MvsContext* c, const mvs_view_t* views, int32_t n_views, const mvs_fuse_opts_t* opts, void* out) {
    K.c = c; K.views = views; K.n_views = n_views; K.opts = opts; K.out = out;
    K.dtype = views[0].dtype; K.es = mvs_dtype_size(K.dtype); K.ndim = opts->ndim;
    for (int k = 0; k < 3; ++k) K.cs[k] = (int)opts->out_shape[k];
    K.S = {K.cs[0], K.cs[1], K.cs[2]};
    K.O = {(int)(K.cs[0] - 2 * opts->trim[0]), (int)(K.cs[1] - 2 * opts->trim[1]), (int)(K.cs[2] - 2 * opts->trim[2])};
    K.n = (long long)K.S.nz * K.S.ny * K.S.nx; K.no = (long long)K.O.nz * K.O.ny * K.O.nx;
    gaussian_taps((double)opts->sigma_1, &K.r1, &K.w1); gaussian_taps((double)opts->sigma_2, &K.r2, &K.w2);
}

// Device views in the chunk's frame and their boxes inside the chunk.  No side effect: nothing is queued, and the views' data pointers
// stay the call's until cb_stage_views (the geometry does not depend on them).  fast: the views also get their translation-path
// records; one without the closed-form blend weight sends all of them through the generic blend launch.
int cb_geometry(CbCall& K, bool fast) {
    K.fast = fast;
    { const int rc = mvs_stage_views_bytes(K.c, K.views, K.n_views, K.es, &K.host_bytes); if (rc) return rc; }
    K.dvs.resize((size_t)K.n_views); K.boxes.resize((size_t)K.n_views);
    if (fast) K.trv.resize((size_t)K.n_views);
    K.tr_all = fast && !K.c->cb_blend_generic;
    K.pool = CbPool(); K.VS = CbFastViews{}; K.VS.nv = K.n_views;
    for (int i = 0; i < K.n_views; ++i) {
        { const int rc = mvs_fill_dev_view(K.c, K.views[i], K.ndim, K.views[i].data, &K.dvs[i]); if (rc) return rc; }
        if (!fast) mvs_fuse_chunk_plan::view_to_chunk_frame(&K.dvs[i], K.opts->index_origin, K.views[i].index_offset);
        else if (!mvs_fuse_chunk_plan::tr_view_in_chunk(&K.dvs[i], K.opts->order, MVS_FUSE_WEIGHTED_AVERAGE, K.opts->out_shape, K.es, K.opts->index_origin,
                                                        K.views[i].index_offset, &K.trv[i])) K.tr_all = false;
        int lo[3], hi[3], row0, tab0;
        mvs_fuse_chunk_plan::view_chunk_box(K.dvs[i], K.opts->out_shape, lo, hi);
        const CbBox& B = K.boxes[i];
        cb_box_add(&K.pool, lo, hi, &K.boxes[i], &row0, &tab0);
        if (fast) K.VS.v[i] = CbFastView{(int)B.off, {B.n[0], B.n[1], B.n[2]}, {B.lo[0], B.lo[1], B.lo[2]}, row0, tab0, 0, 0, 0, 0, 0, 0};
    }
    return MVS_OK;
}

// Host slabs go through scratch slot 0; ev_start opens the call's timing in front of the first upload.
int cb_stage_views(CbCall& K) {
    MvsContext* c = K.c;
    char* slab_base = nullptr;
    if (K.host_bytes && !(slab_base = (char*)mvs_scratch(c, 0, K.host_bytes))) return mvs_alloc_failed(c);
    if (K.fast && !c->cb_flag_host) {      // the word the device raises when a view's mask list overflows
        MVS_HIP_TRY(c, hipHostMalloc((void**)&c->cb_flag_host, 64, hipHostMallocMapped));
        MVS_HIP_TRY(c, hipHostGetDevicePointer((void**)&c->cb_flag_dev, c->cb_flag_host, 0));
        *c->cb_flag_host = 0;
    }
    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    size_t cursor = 0;
    int rc = MVS_OK;
    for (int i = 0; i < K.n_views && !rc; ++i) rc = mvs_stage_view(c, K.views[i], K.es, slab_base, &cursor, &K.dvs[i].data);
    return rc;
}

// Taps, boxes, view records, empty mask records (count 0, inverted bounding box) and table offsets: ONE device block in the layout of
// the host staging block.  It travels through the context's pinned staging slot (waited for before it is refilled), so the call does not
// wait for its own work: with the result on the device it returns as soon as everything is queued, and the host prepares the next chunk
// while this one is filtered (the probe spent ~0.4 ms per chunk idle).  mvs_pinned_mark FOLLOWS the upload: the slot is busy until it has run.
int cb_upload_block(CbCall& K) {
    char* hp = (char*)mvs_pinned_slot(K.c, 0, K.up_bytes + 64);
    if (!hp) return mvs_alloc_failed(K.c);
    auto at = [&](const void* dev) { return hp + ((const char*)dev - K.dblock); };
    memcpy(at(K.dfw1), K.w1.data(), K.w1.size() * 8); memcpy(at(K.dfw2), K.w2.data(), K.w2.size() * 8);
    for (size_t k = 0; k < K.w1.size() && K.fast; ++k) ((float*)at(K.ffw1))[k] = (float)K.w1[k];
    for (size_t k = 0; k < K.w2.size() && K.fast; ++k) ((float*)at(K.ffw2))[k] = (float)K.w2[k];
    if (!K.fast) memcpy(at(K.dboxes), K.boxes.data(), (size_t)K.n_views * sizeof(CbBox));
    memcpy(at(K.dviews_dev), &K.dvs[0], (size_t)K.n_views * sizeof(DevView));
    const CbMaskRec empty = {0ull, {0x7fffffff, 0x7fffffff, 0x7fffffff}, {-1, -1, -1}};      // (CbFastRec begins with the same fields)
    for (int i = 0; i < K.n_views; ++i) {
        memset(at(K.drecs) + (size_t)i * K.rec_bytes, 0, K.rec_bytes);
        memcpy(at(K.drecs) + (size_t)i * K.rec_bytes, &empty, sizeof(empty));
    }
    if (!K.fast) memcpy(at(K.dtable_off), K.table_off.data(), (size_t)K.n_views * 16);
    { const int rc = mvs_upload_small(K.c, K.dblock, hp, K.up_bytes); if (rc) return rc; }
    mvs_pinned_mark(K.c, 0);
    return MVS_OK;
}

// Resampled views and blend weights on the views' boxes (two launches for all views of a chunk of <= 8), then bw *= ~isnan(view),
// normalised over the views
void cb_resample_blend_normalize(CbCall& K) {
    MvsContext* c = K.c;
    const size_t nv = (size_t)K.n_views;
    std::vector<float*> outs(2 * nv); std::vector<int64_t> shp(3 * nv); std::vector<int> b0(3 * nv);
    for (size_t i = 0; i < nv; ++i) {
        const CbBox& B = K.boxes[i];
        outs[i] = K.I + B.off; outs[nv + i] = K.BW + B.off;
        for (int k = 0; k < 3; ++k) { shp[i * 3 + k] = B.n[k]; b0[i * 3 + k] = B.lo[k]; }
    }
    mvs_launch_boxes_batch(c, &K.dvs[0], K.dviews_dev, K.n_views, K.dtype, K.opts->order, NAN, outs.data(), outs.data() + nv,
                           (const int64_t (*)[3])shp.data(), (const int (*)[3])b0.data(), K.tr_all ? K.trv.data() : nullptr);
    K.bx8 = CbBoxes8{};
    if (K.small) cb_boxes8(K.boxes.data(), K.n_views, &K.bx8);
    if (K.fast) hipLaunchKernelGGL(cb_normalize8_runs_kernel, dim3(grid_for((K.n + kCbRun - 1) / kCbRun)), dim3(256), 0, c->stream, K.BW, K.I, K.bx8, K.n_views, K.S);
    else if (K.small) hipLaunchKernelGGL(mask_normalize8_kernel, dim3(grid_for(K.n)), dim3(256), 0, c->stream, K.BW, K.I, K.bx8, K.n_views, K.S, 0);
    else hipLaunchKernelGGL(mask_normalize_kernel, dim3(grid_for(K.n)), dim3(256), 0, c->stream, K.BW, K.I, K.dboxes, K.n_views, K.S);
}

// Test / profiling switch cb_mask_count: read the views' mask records back.  exact: count the views whose mask was found to be a box;
// fast: sum the list lengths (how many voxels the masks lack inside their bounding boxes).  MVS_CB_DEBUG=1 prints every record.
int cb_mask_report(CbCall& K) {
    MvsContext* c = K.c;
    std::vector<char> hrec((size_t)K.n_views * K.rec_bytes);
    MVS_HIP_TRY(c, hipMemcpyAsync(hrec.data(), K.drecs, hrec.size(), hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < K.n_views; ++i) {
        CbFastRec r = CbFastRec();
        memcpy(&r, hrec.data() + (size_t)i * K.rec_bytes, K.rec_bytes);
        const unsigned long long vol = r.cnt ? (unsigned long long)(r.hi[0] - r.lo[0] + 1) * (unsigned long long)(r.hi[1] - r.lo[1] + 1) *
                                               (unsigned long long)(r.hi[2] - r.lo[2] + 1) : 0ull;
        c->cb_mask_views += 1;
        c->cb_mask_boxes += K.fast ? r.nmiss : ((r.cnt && vol == r.cnt) ? 1 : 0);
        if (!getenv("MVS_CB_DEBUG")) continue;
        const CbBox& B = K.boxes[(size_t)i];
        fprintf(stderr, "[cb %s] view box lo %d %d %d n %d %d %d: valid %llu, bbox %d..%d %d..%d %d..%d", K.fast ? "fast" : "mask", B.lo[0], B.lo[1], B.lo[2],
                B.n[0], B.n[1], B.n[2], r.cnt, r.lo[0], r.hi[0], r.lo[1], r.hi[1], r.lo[2], r.hi[2]);
        if (K.fast) fprintf(stderr, ", listed %d\n", r.nmiss);
        else fprintf(stderr, " (volume %llu)\n", vol);
    }
    return MVS_OK;
}

// normalise F over views, A = bw * Fn, normalise A, out = sum I * A; trimmed, cast.  ev_stop closes the call's timing behind the fuse kernel.  A host
// result is copied back and waited for; a device result is not waited for unless host slabs were staged through scratch the next call may overwrite.
int cb_epilogue(CbCall& K) {
    MvsContext* c = K.c;
    const size_t out_bytes = (size_t)K.no * K.es;
    const bool to_host = K.opts->out_mem == MVS_MEM_HOST;
    void* dout = K.out;
    if (to_host && !(dout = mvs_scratch(c, 1, out_bytes))) return mvs_alloc_failed(c);
    const int tz = (int)K.opts->trim[0], ty = (int)K.opts->trim[1], tx = (int)K.opts->trim[2];
    mvs_dispatch_dtype(K.dtype, [&](auto tag) {
        using T = decltype(tag);
        if (K.fast)
            hipLaunchKernelGGL(cb_fuse8_runs_kernel<T>, dim3(grid_for((K.no + kCbRun - 1) / kCbRun)), dim3(256), 0, c->stream, K.I, K.BW, K.F, K.bx8, K.n_views, tz, ty, tx,
                               K.O, (T*)dout);
        else if (K.small)
            hipLaunchKernelGGL(cb_fuse8_kernel<T>, dim3(grid_for(K.no)), dim3(256), 0, c->stream, K.I, K.BW, K.F, K.bx8, K.n_views, tz, ty, tx, K.O, (T*)dout);
        else
            hipLaunchKernelGGL(cb_fuse_kernel<T>, dim3(grid_for(K.no)), dim3(256), 0, c->stream, K.I, K.BW, K.F, K.dboxes, K.n_views, tz, ty, tx, K.O, (T*)dout);
    });
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    if (to_host) MVS_HIP_TRY(c, hipMemcpyAsync(K.out, dout, out_bytes, hipMemcpyDeviceToHost, c->stream));
    if (to_host || K.host_bytes) MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MVS_OK;
}

// Scratch slot 6 (layout: cb_layout): the pools, the uploaded block and what follows it, as pointers
int cb_scratch(CbCall& K) {
    const size_t n_taps = K.w1.size() + K.w2.size();
    const CbLayout Y = cb_layout(K.fast, K.pool, K.n_views, K.paired, n_taps, sizeof(DevView), K.table_floats);
    char* base = (char*)mvs_scratch(K.c, 6, Y.need);
    if (!base) return mvs_alloc_failed(K.c);
    if (!K.fast && n_taps * 8 > 32 * 1024) return mvs_fail(K.c, MVS_ERR_UNSUPPORTED, "content_based: sigma too large");
    auto at = [&](int section) { return base + Y.off[section]; };
    K.I = (float*)at(CS_I); K.BW = (float*)at(CS_BW); K.F = (float*)at(CS_F); K.tmp = (float*)at(CS_TMP); K.tmp_b = Y.tmp_b;
    K.dblock = at(CS_UP0); K.up_bytes = Y.off[CS_UP1] - Y.off[CS_UP0];
    K.dfw1 = (double*)at(CS_TAPS64); K.dfw2 = K.dfw1 + K.w1.size(); K.ffw1 = (float*)at(CS_TAPS32); K.ffw2 = K.ffw1 + K.w1.size();
    K.dboxes = (CbBox*)at(CS_BOXES); K.dviews_dev = (DevView*)at(CS_VIEWS);      // (the views' records for the batched box launches)
    K.drecs = at(CS_RECS); K.rec_bytes = K.fast ? sizeof(CbFastRec) : sizeof(CbMaskRec);
    K.dtable_off = (long long*)at(CS_TOFF); K.dtables = (float*)at(CS_TABLES); K.dtabs = (double*)at(CS_TABLES);
    K.rows = (int4*)at(CS_ROWS); K.dmiss = (int4*)at(CS_MISS); K.dpart = (CbPartial*)at(CS_PART);
    return MVS_OK;
}

// ---- steps of the exact path ----
// which passes the chunk takes and where the mask tables B(z, y) of every (view, filter) lie
void cb_exact_plan(CbCall& K) {
    K.paired = cb_paired(K.boxes.data(), K.n_views, K.ndim, K.r1, K.r2, K.c->cb_unpaired);
    K.small = cb_small(K.n_views, K.pool.floats);
    K.mask_tables = cb_mask_tables(K.paired, K.n_views, K.pool.floats, K.c->cb_mask_closed_form);
    K.table_off.assign((size_t)K.n_views * 2, 0); K.table_floats = 0;
    for (int i = 0; i < K.n_views * 2 && K.mask_tables; ++i) {
        K.table_off[(size_t)i] = K.table_floats;
        K.table_floats += ((long long)K.boxes[i / 2].n[0] * K.boxes[i / 2].n[1] + 63) / 64 * 64;
    }
}

// is every view's valid mask a box?  (device-side: record + tables, no host round trip)
void cb_exact_mask_tables(CbCall& K) {
    int max_nz = 1;
    for (const CbBox& B : K.boxes) max_nz = std::max(max_nz, B.n[0]);
    hipLaunchKernelGGL(cb_mask_bbox_kernel, dim3((unsigned)std::min<long long>((K.pool.max_box + 2047) / 2048, 512), K.n_views), dim3(256), 0, K.c->stream,
                       K.I, K.BW, K.bx8, (CbMaskRec*)K.drecs);
    hipLaunchKernelGGL(cb_mask_table_kernel, dim3(max_nz, K.n_views, 2), dim3(256), 0, K.c->stream, (const CbMaskRec*)K.drecs, K.bx8, K.S, K.ndim, K.r1, K.dfw1,
                       K.r2, K.dfw2, K.dtables, K.dtable_off);
}

// the instantiations of gauss1d_pair_kernel the schedule reaches, [split][src][dst] (a split pass hands both quantities on: DST_AB only)
#define MVS_PAIR(S_, D_, SP_) gauss1d_pair_kernel<S_, D_, SP_>
void (*const kPairKernels[2][3][3])(PairIO, GaussLines, int, const double*, int) = {
    {{MVS_PAIR(SRC_AB, DST_AB, false), MVS_PAIR(SRC_AB, DST_SQ, false), MVS_PAIR(SRC_AB, DST_F, false)},
     {MVS_PAIR(SRC_PREP, DST_AB, false), MVS_PAIR(SRC_PREP, DST_SQ, false), nullptr},
     {MVS_PAIR(SRC_VMASK, DST_AB, false), nullptr, MVS_PAIR(SRC_VMASK, DST_F, false)}},
    {{MVS_PAIR(SRC_AB, DST_AB, true), nullptr, nullptr}, {MVS_PAIR(SRC_PREP, DST_AB, true), nullptr, nullptr}, {MVS_PAIR(SRC_VMASK, DST_AB, true), nullptr, nullptr}}};
#undef MVS_PAIR

// paired passes (gauss1d_pair_kernel; schedule: cb_pair_schedule): per view 2 x ndim launches, one view after the other on the
// context's stream -- consecutive chunks overlap on ONE stream by themselves (docs/DESIGN_history.md: the forked form)
int cb_exact_paired_passes(CbCall& K) {
    float* t[5];      // 5 temporaries of the largest box, shared by the views
    for (int k = 0; k < 5; ++k) t[k] = (float*)((char*)K.tmp + (size_t)k * K.tmp_b);
    for (int v = 0; v < K.n_views; ++v) {
        const CbBox& B = K.boxes[v];
        if ((long long)B.n[0] * B.n[1] * B.n[2] == 0) continue;
        auto buf = [&](int b) -> float* { return b == kCbBufF ? K.F + B.off : (b >= 0 && b < 5) ? t[b] : nullptr; };
        CbPairPass passes[6];
        const int np = cb_pair_schedule(K.ndim, B.n, K.r1, K.r2, K.c->cb_nosplit, passes);
        for (int i = 0; i < np; ++i) {
            const CbPairPass& p = passes[i];
            const int f = p.filt, radius = f ? K.r2 : K.r1, pf = p.axis == 2 ? 1 : 0;
            const double* fw = f ? K.dfw2 : K.dfw1;
            PairIO P;
            P.im = K.I + B.off; P.bw = K.BW + B.off; P.src = p.src; P.dst = p.dst;
            P.a = buf(p.in_a); P.b = buf(p.in_b); P.oa = buf(p.out_a); P.ob = buf(p.out_b);
            P.rec = K.mask_tables ? (const CbMaskRec*)K.drecs + v : nullptr;
            P.mtab = K.mask_tables ? K.dtables + K.table_off[(size_t)v * 2 + f] : nullptr;
            GaussLines L = cb_lines(B.n, B.lo, K.cs, p.axis);
            L.T = p.T;
            const dim3 g((unsigned)((L.n_lines + L.T - 1) / L.T), p.split ? 2 : 1), b(256);
            hipLaunchKernelGGL(kPairKernels[p.split ? 1 : 0][p.src][p.dst], g, b, p.lds, K.c->stream, P, L, radius, fw, pf);
            K.c->cb_exact_paired_launches += 1;
        }
    }
    MVS_HIP_TRY(K.c, hipGetLastError());
    return MVS_OK;
}

// one Gaussian of one array of a box (separate passes): LDS-staged lines when a useful tile of them fits, else the tap-by-tap kernel
void cb_gauss_separate(CbCall& K, const float* src, float* dst, const CbBox& B, int radius, const double* fw) {
    const Shape3 Sb = {B.n[0], B.n[1], B.n[2]};
    const int gbb = grid_for((long long)B.n[0] * B.n[1] * B.n[2]);
    float* const tmp[2] = {(float*)((char*)K.tmp + 4 * K.tmp_b), (float*)((char*)K.tmp + 5 * K.tmp_b)};      // T1, T2
    const float* cur = src;
    for (int axis = 3 - K.ndim, pass = 0; axis < 3; ++axis, ++pass) {
        float* d = (axis == 2) ? dst : tmp[pass & 1];
        GaussLines L = cb_lines(B.n, B.lo, K.cs, axis);
        L.T = cb_single_T(L.len, radius, axis);
        if (L.T)
            hipLaunchKernelGGL(gauss1d_lds_kernel, dim3((unsigned)((L.n_lines + L.T - 1) / L.T)), dim3(256), cb_single_lds(L.len, radius, L.T), K.c->stream, cur, d, L,
                               radius, fw, axis == 2 ? 1 : 0);
        else hipLaunchKernelGGL(gauss1d_kernel, dim3(gbb), dim3(256), 0, K.c->stream, cur, d, Sb, axis, radius, fw, L.b0, L.full);
        (L.T ? K.c->cb_exact_lds_launches : K.c->cb_exact_tap_launches) += 1;
        cur = d;
    }
}

// separate value / mask passes (option cb_unpaired, or a line no paired tile fits): temporaries A, V0, M, T0 (+ T1, T2 of cb_gauss_separate)
void cb_exact_separate_passes(CbCall& K) {
    float *A = K.tmp, *V0 = (float*)((char*)A + K.tmp_b), *M = (float*)((char*)A + 2 * K.tmp_b), *T0 = (float*)((char*)A + 3 * K.tmp_b);
    for (int v = 0; v < K.n_views; ++v) {
        const CbBox& B = K.boxes[v];
        const long long bn = (long long)B.n[0] * B.n[1] * B.n[2];
        if (bn == 0) continue;
        const int gbb = grid_for(bn);
        float* Fv = K.F + B.off;
        hipLaunchKernelGGL(prep_kernel, dim3(gbb), dim3(256), 0, K.c->stream, K.I + B.off, K.BW + B.off, bn, A, V0, M);
        cb_gauss_separate(K, V0, T0, B, K.r1, K.dfw1);           // VV  (T0)
        cb_gauss_separate(K, M, Fv, B, K.r1, K.dfw1);            // WW  (Fv used as temporary)
        hipLaunchKernelGGL(ng_finish_sq_kernel, dim3(gbb), dim3(256), 0, K.c->stream, T0, Fv, A, bn, V0);   // V0 <- (A - Z)^2, NaN -> 0
        cb_gauss_separate(K, V0, T0, B, K.r2, K.dfw2);           // VV2 (T0)
        cb_gauss_separate(K, M, V0, B, K.r2, K.dfw2);            // WW2 (V0)
        hipLaunchKernelGGL(ng_finish_kernel, dim3(gbb), dim3(256), 0, K.c->stream, T0, V0, A, bn, Fv);
    }
}

int cb_exact_path(CbCall& K) {
    int rc = cb_geometry(K, false);
    if (!rc) rc = cb_stage_views(K);
    if (!rc) { cb_exact_plan(K); rc = cb_scratch(K); }
    if (!rc) rc = cb_upload_block(K);
    if (rc) return rc;
    K.c->cb_exact_chunks += 1;
    if (!K.small) K.c->cb_exact_large_chunks += 1;
    cb_resample_blend_normalize(K);
    if (K.mask_tables) {
        cb_exact_mask_tables(K);
        if (K.c->cb_mask_count) { rc = cb_mask_report(K); if (rc) return rc; }
    }
    if (K.paired) { rc = cb_exact_paired_passes(K); if (rc) return rc; }
    else cb_exact_separate_passes(K);
    MVS_HIP_TRY(K.c, hipGetLastError());
    return cb_epilogue(K);
}

// ---- steps of the fast path (kernels: mvs_gauss_fast.inc) ----
// the valid mask of every view: bounding box + listed voxels (sorted); tables of the box under both filters
int cb_fast_mask_scan(CbCall& K) {
    MvsContext* c = K.c;
    CbFastRec* drecs = (CbFastRec*)K.drecs;
    hipLaunchKernelGGL(cb_rows_kernel, dim3(K.rows_grid, K.n_views), dim3(256), 0, c->stream, K.I, K.VS, K.rows, K.dpart);
    hipLaunchKernelGGL(cb_rec_reduce_kernel, dim3(K.n_views), dim3(256), 0, c->stream, K.dpart, (int)K.rows_grid, drecs);
    hipLaunchKernelGGL(cb_missing_kernel, dim3((unsigned)std::min<long long>((K.pool.max_rows + 255) / 256, 1024), K.n_views), dim3(256), 0, c->stream, K.I, K.VS, K.rows,
                       drecs, K.dmiss, c->cb_flag_dev);
    hipLaunchKernelGGL(cb_sort_missing_kernel, dim3(K.n_views), dim3(kCbMissCap), 0, c->stream, drecs, K.dmiss);
    hipLaunchKernelGGL(cb_tables_kernel, dim3(3, K.n_views, 2), dim3(256), 0, c->stream, K.VS, drecs, K.S, K.ndim, K.r1, K.dfw1, K.r2, K.dfw2, K.dtabs);
    MVS_HIP_TRY(c, hipGetLastError());
    return MVS_OK;
}

// 2 * ndim line passes, each ONE launch over all views (schedule: cb_fast_schedule)
int cb_fast_line_passes(CbCall& K) {
    MvsContext* c = K.c;
    CbFastPass passes[6];
    const int np = cb_fast_schedule(K.VS, K.ndim, K.cs, K.opts->trim, K.r1, K.r2, K.Tsel, passes);
    float* const pools[3] = {K.I, K.tmp, K.F};      // kCbBufI, kCbBufT0, kCbBufFast
    for (int i = 0; i < np; ++i) {
        const CbFastPass& p = passes[i];
        if (p.nb == 0) continue;
        const int f = p.filt;
        // accumulators (option cb_taps_f64): 1 (default) = float64 for both filters, 0 = float32 for both, 2 / 3 = float64 for the first / second
        // filter only.  C3 at size, one-count flips of the fused uint16 voxels against the oracle (all of them at truncation boundaries, none
        // beyond the 1e-4 bar): 0.04 % (1; the bit-faithful passes: 0.04 %), 0.10 % (3), 0.21 % (2), 0.22 % (0) -- the noise of float32 taps
        // enters through the second filter, whose result IS the weight; the probe takes 11.8 ms with 0 and 12.4 ms with 1 (memory and latency)
        const bool f64 = c->cb_taps == 1 || (c->cb_taps == 2 && f == 0) || (c->cb_taps == 3 && f == 1);
        CbLineArgs A;
        A.src = pools[p.src_buf]; A.dst = pools[p.dst_buf]; A.I = K.I; A.S = K.S;
        A.axis = p.axis; A.radius = p.radius; A.ndim = K.ndim; A.filt = f;
        A.fwf = f ? K.ffw2 : K.ffw1; A.fwd = f ? K.dfw2 : K.dfw1; A.tabs = K.dtabs; A.recs = (const CbFastRec*)K.drecs; A.miss = K.dmiss;
#define MVS_CBL(S_, D_, PF_) do { if (f64) hipLaunchKernelGGL((cb_line_kernel<S_, D_, double, PF_>), dim3(p.nb), dim3(256), p.lds, c->stream, A, p.views); \
                                  else hipLaunchKernelGGL((cb_line_kernel<S_, D_, float, PF_>), dim3(p.nb), dim3(256), p.lds, c->stream, A, p.views); } while (0)
        if (p.dst == CBD_PLAIN) { if (p.src == CBS_NAN0) MVS_CBL(CBS_NAN0, CBD_PLAIN, false); else MVS_CBL(CBS_PLAIN, CBD_PLAIN, false); }
        else if (p.dst == CBD_SQ) MVS_CBL(CBS_PLAIN, CBD_SQ, true);
        else MVS_CBL(CBS_PLAIN, CBD_F, true);
#undef MVS_CBL
        c->cb_line_launches += 1;
    }
    MVS_HIP_TRY(c, hipGetLastError());
    return MVS_OK;
}

// The default path: mask from a box + list, one quantity per pass, all views in one launch.  *taken = false: this chunk is not its kind
// (cb_fast_accepts_chunk / _boxes: more than 8 views, a rotated / scaled view, a chunk axis shorter than a filter radius, a line that
// does not fit LDS) and the caller runs the bit-faithful passes.  It declines BEFORE any side effect: no scratch is taken, no upload is
// queued, ev_start is not recorded.
int cb_fast_path(CbCall& K, bool* taken) {
    MvsContext* c = K.c;
    *taken = false;
    bool identity = true;
    for (int i = 0; i < K.n_views && identity; ++i) identity = cb_is_identity(K.views[i].matrix);
    if (cb_fast_accepts_chunk(K.n_views, K.ndim, K.cs, K.r1, K.r2, identity) != kCbTaken) return MVS_OK;
    int rc = cb_geometry(K, true);
    if (rc || cb_fast_accepts_boxes(K.pool, K.boxes.data(), K.n_views, K.ndim, K.r1, K.r2, K.Tsel) != kCbTaken) return rc;
    K.small = true; K.paired = false; K.table_floats = 0; K.rows_grid = cb_rows_grid(K.pool.max_rows);
    rc = cb_stage_views(K);
    if (!rc) rc = cb_scratch(K);
    if (!rc) rc = cb_upload_block(K);
    if (rc) return rc;
    cb_resample_blend_normalize(K);
    rc = cb_fast_mask_scan(K);
    if (!rc && c->cb_mask_count) rc = cb_mask_report(K);
    if (!rc) rc = cb_fast_line_passes(K);
    if (!rc) rc = cb_epilogue(K);
    if (rc) return rc;
    *taken = true;
    // A mask list that overflowed raised the flag.  A host result has been waited for: the flag is read here and the caller redoes this
    // chunk through the bit-faithful passes.  A device result is not waited for: the Python side checks the flag (counter cb_overflow).
    if (K.opts->out_mem == MVS_MEM_HOST && *c->cb_flag_host) {
        *c->cb_flag_host = 0; c->cb_overflows += 1; *taken = false;
    }
    return MVS_OK;
}

}  // namespace

int mvs_fuse_content_based(MvsContext* c, const mvs_view_t* views, int32_t n_views, const mvs_fuse_opts_t* opts, void* out) {
    if (opts->order != 0 && opts->order != 1) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "content_based: order 0|1 only");
    CbCall K;
    cb_begin(K, c, views, n_views, opts, out);
    if (!c->cb_exact) {
        bool taken = false;
        const int rc = cb_fast_path(K, &taken);
        if (rc || taken) return rc;
    }
    return cb_exact_path(K);
}
