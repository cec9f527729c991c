// mvs_dct_weights.hip -- DCT Shannon-entropy fusion weights (weights.content_based_dct, weights.py:77-290 of the
// reference; Royer et al. 2016).
//
// Per view and block of the chunk (blocks of the clamped dct sizes, anchored at chunk index 0, smaller at the far edges):
//   valid   fewer than 0.2 * size non-NaN voxels -> quality 0 (:212-214)
//   fill    NaN voxels <- nanmin(block) if that is > 1e-4, else 0 (:216-219)
//   DCT     orthonormal DCT-II along every axis (scipy.fftpack.dctn(norm="ortho"), any length) (:221)
//   quality OTF branch: l2 = |d|_2, p = |d[sum(k) < r_o]| / l2, q = sign * ((2 / r_o^2) H) ** exponent (:223-240)
//           L1 branch:  dsl1 = mean |d|, p = |d| / dsl1, q = (dsl1 H) ** exponent (:242-251),  H = -sum p log2 p (p > 0)
// then Q -= nanmin over the views, normalize_weights (:253-255), and per voxel the trilinear clamped lookup into Q_v
// (affine_transform(order=1, mode="nearest"), :260-281) -- normalised again for the standalone weights, or multiplied
// into the weighted average of mvs_fuse.hip for the fused chunk (the voxel-level normalisations cancel there).
//
// Two quality paths, one workgroup per (view, block) work item:
//   LDS     every block extent <= 32: the block (x rows padded to an odd pitch) sits in LDS (<= 132 KiB), each thread
//           transforms whole lines in registers against a zero-padded 32 x 32 coefficient table read with uniform
//           (scalar) loads
//   general any extent: two ping-pong buffers and the coefficient tables in a bounded global scratch area, one slot
//           per resident workgroup, the work items striding over the slots
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mvs_internal.h"
#include "mvs_fold_dev.h"
#include "mvs_fuse_dev.h"
#include "mvs_dct_dev.h"

namespace {

constexpr int kLdsMax = 32;               // largest block extent per axis of the LDS path
constexpr int kLdsThreads = 1024;
constexpr int kGenThreads = 256;
constexpr size_t kGenBudget = (size_t)256 << 20;   // bytes of global scratch of the general path

struct DctGeom {
    int S[3];          // chunk shape (z, y, x)
    int ds[3];         // clamped block sizes (2D: ds[0] == 1)
    int nb[3];         // blocks per axis
    int nblocks;
    int otf;           // 1: OTF branch (r_o), 0: L1 branch
    double r_o;
    double exponent;
};

// orthonormal DCT-II coefficient: s_k cos(pi k (2n + 1) / (2L)), the argument reduced exactly modulo 2 pi
__device__ __forceinline__ float dct_coef(int L, int k, int n) {
    const long long m = ((long long)(2 * n + 1) * k) % (4LL * L);
    const double s = k == 0 ? sqrt(1.0 / L) : sqrt(2.0 / L);
    return (float)(s * cospi((double)m / (2.0 * L)));
}

// tables of the LDS path: T[L - 1][k][n] for L = 1..32, zero outside k, n < L
__global__ void dct_table_kernel(float* __restrict__ T) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kLdsMax * kLdsMax * kLdsMax; i += gridDim.x * blockDim.x) {
        const int n = i % kLdsMax, k = (i / kLdsMax) % kLdsMax, L = i / (kLdsMax * kLdsMax) + 1;
        T[i] = (k < L && n < L) ? dct_coef(L, k, n) : 0.f;
    }
}

struct Blk {
    int o[3], e[3];    // origin in the chunk, extent
    int px;            // x pitch of the block buffer
    int vol;
};

__device__ __forceinline__ void block_of(const DctGeom& g, int b, bool pad, Blk& k) {
    const int bx = b % g.nb[2], t = b / g.nb[2], by = t % g.nb[1], bz = t / g.nb[1];
    const int bi[3] = {bz, by, bx};
    for (int d = 0; d < 3; ++d) {
        k.o[d] = bi[d] * g.ds[d];
        k.e[d] = min(g.ds[d], g.S[d] - k.o[d]);
    }
    k.px = pad ? (k.e[2] | 1) : k.e[2];
    k.vol = k.e[0] * k.e[1] * k.e[2];
}

// sum / minimum over the workgroup, in every thread.  The folds start from 0.0 / INFINITY: partials that are all -0.0 give +0.0,
// partials that are all NaN give INFINITY.
template <int NT>
__device__ __forceinline__ double wg_sum(double v) { return 0.0 + mvs_fold::block_fold_all<NT / 64>(mvs_fold::Sums<double>{{v}}).v[0]; }

struct MinPartial {
    float v;
    __device__ __forceinline__ void merge(const MinPartial& o) { v = fminf(v, o.v); }
    template <typename S> __device__ __forceinline__ MinPartial shuffled(S sh, int off) const { return {sh(v, off)}; }
};
template <int NT>
__device__ __forceinline__ float wg_min(float v) { return fminf(INFINITY, mvs_fold::block_fold_all<NT / 64>(MinPartial{v}).v); }

__device__ __forceinline__ int buf_index(const Blk& k, int z, int y, int x) { return (z * k.e[1] + y) * k.px + x; }

// copy the block of one view into `buf`, count its valid voxels and fill the NaN ones; false: quality 0 (too few valid)
template <int NT>
__device__ bool load_block(const float* __restrict__ src, const DctGeom& g, const Blk& k, float* buf) {
    double cnt = 0.0;
    float mn = INFINITY;
    for (int i = threadIdx.x; i < k.vol; i += NT) {
        const int x = i % k.e[2], r = i / k.e[2], y = r % k.e[1], z = r / k.e[1];
        const float v = src[((long long)(k.o[0] + z) * g.S[1] + (k.o[1] + y)) * g.S[2] + k.o[2] + x];
        buf[buf_index(k, z, y, x)] = v;
        if (v == v) {
            cnt += 1.0;
            mn = fminf(mn, v);
        }
    }
    const double n_valid = wg_sum<NT>(cnt);
    if (n_valid < 0.2 * (double)k.vol) return false;
    if (n_valid < (double)k.vol) {
        const float m = wg_min<NT>(mn);
        const float fill = (double)m > 0.0001 ? m : 0.f;
        for (int i = threadIdx.x; i < k.vol; i += NT) {
            const int x = i % k.e[2], r = i / k.e[2], y = r % k.e[1], z = r / k.e[1];
            float& v = buf[buf_index(k, z, y, x)];
            if (v != v) v = fill;
        }
    }
    __syncthreads();
    return true;
}

// line `l` of the pass along `axis`: first element and stride in the block buffer
__device__ __forceinline__ void line_of(const Blk& k, int axis, int l, int& base, int& stride) {
    if (axis == 2) {
        base = l * k.px;               // l = z * e1 + y
        stride = 1;
    } else if (axis == 1) {
        const int z = l / k.e[2], x = l % k.e[2];
        base = z * k.e[1] * k.px + x;
        stride = k.px;
    } else {
        const int y = l / k.e[2], x = l % k.e[2];
        base = y * k.px + x;
        stride = k.e[1] * k.px;
    }
}

// entropy quality of the transformed block (weights.py:223-251)
template <int NT>
__device__ float block_quality(const float* buf, const DctGeom& g, const Blk& k) {
    if (g.otf) {
        double ss = 0.0;
        for (int i = threadIdx.x; i < k.vol; i += NT) {
            const int x = i % k.e[2], r = i / k.e[2], y = r % k.e[1], z = r / k.e[1];
            const double d = buf[buf_index(k, z, y, x)];
            ss += d * d;
        }
        const float l2 = (float)sqrt(wg_sum<NT>(ss));
        if (l2 == 0.f) return 0.f;
        double h = 0.0;
        for (int i = threadIdx.x; i < k.vol; i += NT) {
            const int x = i % k.e[2], r = i / k.e[2], y = r % k.e[1], z = r / k.e[1];
            if (!((double)(x + y + z) < g.r_o)) continue;
            const float p = fabsf(buf[buf_index(k, z, y, x)]) / l2;
            if (p > 0.f) h -= (double)(p * log2f(p));
        }
        h = wg_sum<NT>(h);
        float q = (float)((2.0 / (g.r_o * g.r_o)) * h);
        const float sg = q > 0.f ? 1.f : (q < 0.f ? -1.f : q);      // np.sign (0 -> 0, NaN -> NaN)
        q = powf(q, (float)g.exponent);
        return q * sg;
    }
    double sa = 0.0;
    for (int i = threadIdx.x; i < k.vol; i += NT) {
        const int x = i % k.e[2], r = i / k.e[2], y = r % k.e[1], z = r / k.e[1];
        sa += fabs((double)buf[buf_index(k, z, y, x)]);
    }
    const float dsl1 = (float)(wg_sum<NT>(sa) / (double)k.vol);
    if (dsl1 == 0.f) return 0.f;
    double h = 0.0;
    for (int i = threadIdx.x; i < k.vol; i += NT) {
        const int x = i % k.e[2], r = i / k.e[2], y = r % k.e[1], z = r / k.e[1];
        const float p = fabsf(buf[buf_index(k, z, y, x)]) / dsl1;
        if (p > 0.f) h -= (double)(p * log2f(p));
    }
    h = wg_sum<NT>(h);
    return (float)pow((double)dsl1 * h, g.exponent);      // a negative base with a fractional exponent: NaN
}

// LDS path: one workgroup per (view, block); `stack` [view][S], Q [view][nblocks]
__global__ __launch_bounds__(kLdsThreads) void dct_quality_lds(const float* __restrict__ stack, DctGeom g, const float* __restrict__ tabs,
                                                               float* __restrict__ Q) {
    extern __shared__ float4 lds4[];
    float* buf = reinterpret_cast<float*>(lds4);
    const int v = blockIdx.x / g.nblocks, b = blockIdx.x % g.nblocks;
    Blk k;
    block_of(g, b, true, k);
    const long long S = (long long)g.S[0] * g.S[1] * g.S[2];
    if (!load_block<kLdsThreads>(stack + v * S, g, k, buf)) {
        if (threadIdx.x == 0) Q[blockIdx.x] = 0.f;
        return;
    }
    for (int axis = 2; axis >= 0; --axis) {
        const int len = k.e[axis];
        if (len == 1) continue;          // the length-1 orthonormal DCT is the identity
        const int nl = k.vol / len;
        const float* T = tabs + (len - 1) * (kLdsMax * kLdsMax);
        for (int l = threadIdx.x; l < nl; l += kLdsThreads) {
            int base, stride;
            line_of(k, axis, l, base, stride);
            float xv[kLdsMax];
#pragma unroll
            for (int n = 0; n < kLdsMax; ++n) xv[n] = n < len ? buf[base + n * stride] : 0.f;
            for (int kk = 0; kk < len; ++kk) {
                const float* t = T + kk * kLdsMax;
                float acc = 0.f;
#pragma unroll
                for (int n = 0; n < kLdsMax; ++n) acc = fmaf(t[n], xv[n], acc);
                buf[base + kk * stride] = acc;
            }
        }
        __syncthreads();
    }
    const float q = block_quality<kLdsThreads>(buf, g, k);
    if (threadIdx.x == 0) Q[blockIdx.x] = q;
}

// general path: workgroup w owns scratch slot w (two block buffers + the tables of the block's three lengths) and takes
// the work items w, w + gridDim.x, ...
__global__ __launch_bounds__(kGenThreads) void dct_quality_general(const float* __restrict__ stack, DctGeom g, float* __restrict__ scratch,
                                                                   long long slot_floats, int n_items, float* __restrict__ Q) {
    const long long bvol = (long long)g.ds[0] * g.ds[1] * g.ds[2];
    float* bufA = scratch + (long long)blockIdx.x * slot_floats;
    float* bufB = bufA + bvol;
    float* tab = bufB + bvol;
    const long long S = (long long)g.S[0] * g.S[1] * g.S[2];
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int v = item / g.nblocks, b = item % g.nblocks;
        Blk k;
        block_of(g, b, false, k);
        __syncthreads();                 // (the previous item's readers of the slot are done)
        if (!load_block<kGenThreads>(stack + v * S, g, k, bufA)) {
            if (threadIdx.x == 0) Q[item] = 0.f;
            continue;
        }
        const int toff[3] = {0, k.e[0] * k.e[0], k.e[0] * k.e[0] + k.e[1] * k.e[1]};
        for (int axis = 0; axis < 3; ++axis) {
            const int L = k.e[axis];
            for (int i = threadIdx.x; i < L * L; i += kGenThreads) tab[toff[axis] + i] = dct_coef(L, i / L, i % L);
        }
        __syncthreads();
        float* in = bufA;
        float* out = bufB;
        for (int axis = 2; axis >= 0; --axis) {
            const int len = k.e[axis];
            if (len == 1) continue;
            const int nl = k.vol / len;
            const float* T = tab + toff[axis];
            for (long long it = threadIdx.x; it < (long long)nl * len; it += kGenThreads) {
                const int kk = (int)(it % len), l = (int)(it / len);
                int base, stride;
                line_of(k, axis, l, base, stride);
                const float* t = T + (long long)kk * len;
                float acc = 0.f;
                for (int n = 0; n < len; ++n) acc = fmaf(t[n], in[base + (long long)n * stride], acc);
                out[base + (long long)kk * stride] = acc;
            }
            __syncthreads();
            float* t = in;
            in = out;
            out = t;
        }
        const float q = block_quality<kGenThreads>(in, g, k);
        if (threadIdx.x == 0) Q[item] = q;
    }
}

// Q -= nanmin over the views; normalize_weights over the views (nansum, 0 -> 1) (weights.py:253-255, 325-345)
__global__ void dct_normalize_kernel(const float* __restrict__ Q, int n_views, int nblocks, float* __restrict__ Qn) {
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < nblocks; b += gridDim.x * blockDim.x) {
        float m = NAN;
        for (int v = 0; v < n_views; ++v) {
            const float q = Q[(long long)v * nblocks + b];
            if (q == q) m = (m == m) ? fminf(m, q) : q;
        }
        float sum = 0.f;
        for (int v = 0; v < n_views; ++v) {
            const float s = Q[(long long)v * nblocks + b] - m;
            Qn[(long long)v * nblocks + b] = s;
            if (s == s) sum += s;
        }
        if (sum == 0.f) sum = 1.f;
        for (int v = 0; v < n_views; ++v) Qn[(long long)v * nblocks + b] = Qn[(long long)v * nblocks + b] / sum;
    }
}

// per voxel: every view's lookup into its normalised grid, then normalize_weights over the views (weights.py:270-283)
__global__ void dct_interp_kernel(DctLookup L, int n_views, int sz, int sy, int sx, float* __restrict__ W) {
    const long long S = (long long)sz * sy * sx;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % sx), y = (int)((i / sx) % sy), z = (int)(i / ((long long)sx * sy));
        float sum = 0.f;
        for (int v = 0; v < n_views; ++v) {
            const float w = dct_lookup(L, v, (double)z, (double)y, (double)x);
            W[v * S + i] = w;
            if (w == w) sum += w;
        }
        if (sum == 0.f) sum = 1.f;
        for (int v = 0; v < n_views; ++v) W[v * S + i] = W[v * S + i] / sum;
    }
}

int grid_for(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 256 * 32)); }

// clamped block sizes, grid and branch of weights.py:165-203
int dct_geometry(MvsContext* c, const char* who, const int64_t shape[3], int ndim, const mvs_dct_opts_t* o, DctGeom* g) {
    int min_ds = 0x7fffffff;
    for (int a = 0; a < 3; ++a) {
        g->S[a] = (int)shape[a];
        if (a < 3 - ndim) {
            g->ds[a] = 1;
            g->nb[a] = 1;
            continue;
        }
        long long ds = o->dct_size[a];
        if (ds < 1) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: dct_size on axis %d must be >= 1", who, a);
        if (o->has_output_chunksize) {
            if (o->output_chunksize[a] < 1) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: output_chunksize on axis %d must be >= 1", who, a);
            ds = std::min<long long>(ds, o->output_chunksize[a]);
        }
        ds = std::min<long long>(ds, shape[a]);
        g->ds[a] = (int)ds;
        g->nb[a] = (int)std::max<long long>(1, (shape[a] + ds - 1) / ds);
        min_ds = std::min(min_ds, (int)ds);
    }
    g->nblocks = g->nb[0] * g->nb[1] * g->nb[2];
    g->otf = o->has_otf ? 1 : 0;
    g->r_o = o->has_otf ? o->otf_support_fraction * (double)min_ds : 0.0;
    g->exponent = o->exponent;
    return MVS_OK;
}

// device bytes of the quality pass beyond the stack and the two grids
size_t quality_scratch_bytes(const MvsContext* c, const DctGeom& g, int n_views, bool* lds, int* slots, long long* slot_floats) {
    *lds = !c->dct_general && g.ds[0] <= kLdsMax && g.ds[1] <= kLdsMax && g.ds[2] <= kLdsMax;
    if (*lds) return (size_t)kLdsMax * kLdsMax * kLdsMax * 4;
    const long long bvol = (long long)g.ds[0] * g.ds[1] * g.ds[2];
    *slot_floats = 2 * bvol + (long long)g.ds[0] * g.ds[0] + (long long)g.ds[1] * g.ds[1] + (long long)g.ds[2] * g.ds[2];
    const long long items = (long long)n_views * g.nblocks;
    long long n = (long long)(kGenBudget / ((size_t)*slot_floats * 4));
    n = std::max<long long>(1, std::min<long long>({n, items, 4096}));
    *slots = (int)n;
    return (size_t)n * (size_t)*slot_floats * 4;
}

// quality + normalisation of the grids (stream-ordered, nothing waited for)
int run_quality(MvsContext* c, const DctGeom& g, int n_views, const float* stack, float* Q, float* Qn, void* qscratch, bool lds, int slots,
                long long slot_floats) {
    const long long items = (long long)n_views * g.nblocks;
    if (lds) {
        const size_t lds_bytes = (size_t)g.ds[0] * g.ds[1] * (g.ds[2] | 1) * 4;
        MVS_HIP_TRY(c, hipFuncSetAttribute((const void*)dct_quality_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        hipLaunchKernelGGL(dct_table_kernel, dim3(32), dim3(256), 0, c->stream, (float*)qscratch);
        hipLaunchKernelGGL(dct_quality_lds, dim3((unsigned)items), dim3(kLdsThreads), lds_bytes, c->stream, stack, g, (const float*)qscratch, Q);
    } else {
        hipLaunchKernelGGL(dct_quality_general, dim3(slots), dim3(kGenThreads), 0, c->stream, stack, g, (float*)qscratch, slot_floats, (int)items, Q);
    }
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(dct_normalize_kernel, dim3(grid_for(g.nblocks)), dim3(256), 0, c->stream, (const float*)Q, n_views, g.nblocks, Qn);
    MVS_HIP_TRY(c, hipGetLastError());
    return MVS_OK;
}

DctLookup lookup_of(const DctGeom& g, const float* Qn) {
    DctLookup L{};
    L.q = Qn;
    L.nblocks = g.nblocks;
    for (int d = 0; d < 3; ++d) {
        L.nb[d] = g.nb[d];
        L.scale[d] = 1.0 / (double)g.ds[d];
        L.offset[d] = -((double)g.ds[d] - 1.0) / (2.0 * (double)g.ds[d]);
    }
    return L;
}

}  // namespace

extern "C" int mvs_content_dct_weights(int device, const float* views, int32_t n_views, const int64_t shape[3], int32_t ndim,
                                       const mvs_dct_opts_t* opts, float* weights_out, float* quality_out, int32_t mem) {
    MvsContext* c0 = mvs_ctx(device);
    if (!views || !shape || !opts || !weights_out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_content_dct_weights: NULL argument");
    if (n_views < 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_content_dct_weights: n_views must be >= 1");
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_content_dct_weights: ndim must be 2 or 3");
    if (mem != MVS_MEM_HOST && mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_content_dct_weights: bad mem");
    for (int k = 0; k < 3; ++k)
        if (shape[k] < 1 || shape[k] > 0x7fffffffLL) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_content_dct_weights: bad shape on axis %d", k);
    if (ndim == 2 && shape[0] != 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_content_dct_weights: 2D data has shape[0] == 1");
    const long long S = (long long)shape[0] * shape[1] * shape[2];
    if (S * n_views > (1LL << 40) || S > 0x7fffffffLL) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_content_dct_weights: too large");

    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));
    DctGeom g;
    rc = dct_geometry(c, "mvs_content_dct_weights", shape, ndim, opts, &g);
    if (rc) return rc;
    bool lds = false;
    int slots = 0;
    long long slot_floats = 0;
    const size_t qs_bytes = quality_scratch_bytes(c, g, n_views, &lds, &slots, &slot_floats);
    const size_t vol_bytes = (size_t)S * n_views * 4, grid_bytes = align_up((size_t)g.nblocks * n_views * 4);
    const bool host = mem == MVS_MEM_HOST;
    // work area: [stack | weights] (host data only) | Q | Qn | quality scratch
    const size_t off_st = 0, off_w = off_st + (host ? align_up(vol_bytes) : 0), off_q = off_w + (host ? align_up(vol_bytes) : 0);
    const size_t off_qn = off_q + grid_bytes, off_s = off_qn + grid_bytes, total = off_s + qs_bytes;
    MvsWorkArea work(c);
    rc = work.alloc(total);
    if (rc) return rc;
    char* W = (char*)work.ptr;
    const float* stack = host ? (const float*)(W + off_st) : views;
    float* dw = host ? (float*)(W + off_w) : weights_out;
    float* Q = (float*)(W + off_q);
    float* Qn = (float*)(W + off_qn);
    if (host) MVS_HIP_TRY(c, hipMemcpyAsync((void*)stack, views, vol_bytes, hipMemcpyHostToDevice, c->stream));
    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    rc = run_quality(c, g, n_views, stack, Q, Qn, W + off_s, lds, slots, slot_floats);
    if (rc) return rc;
    hipLaunchKernelGGL(dct_interp_kernel, dim3(grid_for(S)), dim3(256), 0, c->stream, lookup_of(g, Qn), (int)n_views, g.S[0], g.S[1], g.S[2], dw);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (host) MVS_HIP_TRY(c, hipMemcpyAsync(weights_out, dw, vol_bytes, back, c->stream));
    if (quality_out) MVS_HIP_TRY(c, hipMemcpyAsync(quality_out, Q, (size_t)g.nblocks * n_views * 4, back, c->stream));
    if (host) MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return work.release();
}

extern "C" int mvs_fuse_chunk_dct(int device, const mvs_view_t* views, int32_t n_views, const mvs_fuse_opts_t* opts,
                                  const mvs_dct_opts_t* dopts, void* out) {
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    rc = mvs_check_chunk_args(c, "mvs_fuse_chunk_dct", views, n_views, opts, out);
    if (rc) return rc;
    if (!dopts) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_fuse_chunk_dct: NULL/empty argument");
    if (opts->fusion != MVS_FUSE_WEIGHTED_AVERAGE || opts->weights != MVS_WEIGHTS_NONE)
        return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_fuse_chunk_dct: needs fusion weighted_average and weights none");
    for (int k = 0; k < 3; ++k)
        if (opts->index_origin[k] != 0) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_fuse_chunk_dct: index_origin must be 0");
    const long long S = (long long)opts->out_shape[0] * opts->out_shape[1] * opts->out_shape[2];
    if (S * n_views > (1LL << 40) || S > 0x7fffffffLL) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_fuse_chunk_dct: chunk too large");
    for (int i = 0; i < n_views; ++i)
        if (views[i].index_offset[0] || views[i].index_offset[1] || views[i].index_offset[2])
            return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_fuse_chunk_dct: index_offset must be 0");
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));
    DctGeom g;
    rc = dct_geometry(c, "mvs_fuse_chunk_dct", opts->out_shape, opts->ndim, dopts, &g);
    if (rc) return rc;
    bool lds = false;
    int slots = 0;
    long long slot_floats = 0;
    const size_t qs_bytes = quality_scratch_bytes(c, g, n_views, &lds, &slots, &slot_floats);
    const size_t es = mvs_dtype_size(views[0].dtype);
    size_t host_bytes = 0;
    rc = mvs_stage_views_bytes(c, views, n_views, es, &host_bytes);
    if (rc) return rc;
    // work area: host slabs | resampled stack | Q | Qn | quality scratch
    const size_t grid_bytes = align_up((size_t)g.nblocks * n_views * 4);
    const size_t off_st = host_bytes, off_q = off_st + align_up((size_t)S * n_views * 4), off_qn = off_q + grid_bytes, off_s = off_qn + grid_bytes;
    MvsWorkArea work(c);
    rc = work.alloc(off_s + qs_bytes);
    if (rc) return rc;
    char* W = (char*)work.ptr;
    float* stack = (float*)(W + off_st);
    float* Q = (float*)(W + off_q);
    float* Qn = (float*)(W + off_qn);
    // host slabs are staged once; the fuse launch reads the same device copies
    std::vector<mvs_view_t> dv(views, views + n_views);
    size_t cursor = 0;
    for (int i = 0; i < n_views; ++i) {
        rc = mvs_stage_view(c, views[i], es, W, &cursor, &dv[i].data);
        if (rc) return rc;
        dv[i].mem = MVS_MEM_DEVICE;
    }
    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    // transformed_views (_core.py:1622-1633): the views resampled onto the whole chunk, NaN outside
    for (int i = 0; i < n_views; ++i) {
        DevView d;
        rc = mvs_fill_dev_view(c, dv[i], opts->ndim, dv[i].data, &d);
        if (rc) return rc;
        mvs_launch_resample(c, d, dv[i].dtype, opts->order, NAN, stack + (long long)i * S, opts->out_shape);
        MVS_HIP_TRY(c, hipGetLastError());
    }
    rc = run_quality(c, g, n_views, stack, Q, Qn, W + off_s, lds, slots, slot_floats);
    if (rc) return rc;
    const DctLookup L = lookup_of(g, Qn);
    rc = mvs_fuse_chunk_impl(c, dv.data(), n_views, opts, out, &L, true);
    if (rc) return rc;
    if (opts->out_mem != MVS_MEM_HOST && host_bytes) MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the caller may free its slabs)
    return work.release();
}
