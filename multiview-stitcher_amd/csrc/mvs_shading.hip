// mvs_shading.hip -- shading (flat-field) correction of tiled acquisitions (intensity.estimate_shading / apply_shading) on gfx950:
// the per-pixel order statistics of the stack of all tiles and planes, and the kernel that applies a per-pixel gain / offset plane
// to a whole tile.
//
// The reference has no counterpart; the retrospective flat-field estimates of BigStitcher, MIST and BaSiC users are the model.
// mvs_stack_quantiles selects, per pixel (y, x) of the tile, the samples of given ranks among view_v(z, y, x) over all views and
// planes: a most-significant-digit radix select with 8-bit digits (mvs_stack_select.h).  A workgroup owns a strip of 128 bytes of
// one row for ALL samples, keeps the strip's 256-bin histograms in LDS and re-reads the stack once per digit and quantile; nothing
// but the results goes to global memory.  mvs_plane_apply is a copy with one multiply and one add per voxel whose lanes keep the
// coefficients of their pixels in registers while they walk z.
#include "mvs_internal.h"
#include "mvs_fuse_dev.h"
#include "mvs_intensity_dev.h"
#include "mvs_stack_select.h"
#include "mvs_tile_apply.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

using namespace mvs_stack_select;

// ---- order statistics ----------------------------------------------------------------------------------------------------------------
constexpr int kStackThreads = 1024;                         // 16 waves: 32 half waves, one plane each per step
constexpr int kStackSlots = kStackThreads / kStripLanes;    // planes in flight per step of a workgroup
constexpr int kStackUnroll = 4;                             // planes a half wave has loaded before it counts them
constexpr long long kStackMaxBlocks = 1 << 20;

struct StackView {
    const char* data;
    long long sz, sy;                                       // bytes
    long long nz;
};

struct StackArgs {
    const StackView* views;
    int n_views, n_q;
    long long H, W;
    long long n_strips, n_items;                            // strips per row; rows * strips
    double q[MVS_STACK_MAX_QUANTILES];
    float* out;                                             // (n_q, H, W)
    int* count;                                             // (H, W)
};

// where a half wave stands in the stack: plane z of view v; v == n_views: past the end
struct StackCursor {
    int v;
    long long z;
};
__device__ __forceinline__ void cursor_advance(StackCursor& c, long long by, const StackView* views, int n_views) {
    c.z += by;
    while (c.v < n_views && c.z >= views[c.v].nz) {
        c.z -= views[c.v].nz;
        ++c.v;
    }
}

// One pass over all samples of the strip: every sample whose digits above `pass` equal its pixel's prefix adds one to the bin of
// its digit.  Lane `sl` of a half wave holds the pixels xl .. xl + nvalid - 1 of the row; hist[(digit * V + k) * kStripLanes + sl]
// counts digit `digit` of its k-th pixel.
template <typename T, int V>
__device__ __forceinline__ void count_pass(const StackArgs& P, unsigned int* hist, long long y, long long xl, int nvalid, int sl, int slot, int pass,
                                           const uint32_t (&pre)[V]) {
    constexpr int D = (int)sizeof(T);
    StackCursor cur{0, 0};
    cursor_advance(cur, slot, P.views, P.n_views);
    while (cur.v < P.n_views) {
        T vals[kStackUnroll][V];
        bool live[kStackUnroll];
#pragma unroll
        for (int u = 0; u < kStackUnroll; ++u) {
            live[u] = cur.v < P.n_views && nvalid > 0;
            if (cur.v < P.n_views) {
                if (nvalid > 0) {
                    const StackView sv = P.views[cur.v];
                    const T* p = (const T*)(sv.data + cur.z * sv.sz + y * sv.sy) + xl;
                    if (nvalid == V && ((unsigned long long)p & (kWordBytes - 1)) == 0) {
                        struct alignas(kWordBytes) Word { T v[V]; };
                        const Word w = *(const Word*)p;
#pragma unroll
                        for (int k = 0; k < V; ++k) vals[u][k] = w.v[k];
                    } else {
#pragma unroll
                        for (int k = 0; k < V; ++k) vals[u][k] = k < nvalid ? p[k] : T(0);
                    }
                }
                cursor_advance(cur, kStackSlots, P.views, P.n_views);
            }
        }
#pragma unroll
        for (int u = 0; u < kStackUnroll; ++u) {
            if (!live[u]) continue;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                if (k >= nvalid) continue;
                const T v = vals[u][k];
                if (!stack_is_sample(v)) continue;
                const uint32_t key = stack_key(v);
                if (stack_prefix(key, D, pass) != pre[k]) continue;
                atomicAdd(&hist[(stack_digit(key, D, pass) * V + k) * kStripLanes + sl], 1u);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kStackThreads) void stack_quantiles_kernel(StackArgs P) {
    constexpr int D = (int)sizeof(T), V = kWordBytes / D, S = kStripBytes / D;        // digits, pixels per lane, pixels per strip
    __shared__ unsigned int hist[256 * S];                  // [digit][k][lane]: column c = k * kStripLanes + lane of pixel lane * V + k
    __shared__ uint32_t prefix[MVS_STACK_MAX_QUANTILES][S], rank[MVS_STACK_MAX_QUANTILES][S];
    __shared__ unsigned char dead[S];                       // a pixel without samples
    const int t = threadIdx.x, sl = t & (kStripLanes - 1), slot = t / kStripLanes;
    for (long long item = blockIdx.x; item < P.n_items; item += gridDim.x) {
        const long long y = item / P.n_strips;
        long long x0, x1;
        stack_strip_range(stack_plan(P.W, D), P.W, (int)(item % P.n_strips), &x0, &x1);
        const long long xl = x0 + (long long)sl * V;
        const int nvalid = (int)max(0LL, min((long long)V, x1 - xl));
        uint32_t pre[V];
#pragma unroll
        for (int k = 0; k < V; ++k) pre[k] = 0u;

        // the top digit: one pass for all quantiles
        __syncthreads();                                    // (the previous item's readers of the tables are done)
        for (int i = t; i < 256 * S; i += kStackThreads) hist[i] = 0u;
        __syncthreads();
        count_pass<T, V>(P, hist, y, xl, nvalid, sl, slot, 0, pre);
        __syncthreads();
        if (t < P.n_q * S) {
            const int j = t / S, c = t % S;
            uint32_t n = 0;
            for (int d = 0; d < 256; ++d) n += hist[d * S + c];
            const long long x = x0 + stack_column_pixel(c, V);
            if (j == 0) {
                dead[c] = n == 0u;
                if (x < x1) P.count[y * P.W + x] = (int)n;
            }
            int digit = 0;
            uint32_t r = 0;
            if (n) r = stack_bin_walk(hist + c, S, stack_rank(n, P.q[j]), &digit);
            prefix[j][c] = (uint32_t)digit;
            rank[j][c] = r;
        }
        // the further digits, per quantile
        for (int j = 0; j < P.n_q && D > 1; ++j) {
            for (int pass = 1; pass < D; ++pass) {
                __syncthreads();
                for (int i = t; i < 256 * S; i += kStackThreads) hist[i] = 0u;
#pragma unroll
                for (int k = 0; k < V; ++k) pre[k] = prefix[j][k * kStripLanes + sl];
                __syncthreads();
                count_pass<T, V>(P, hist, y, xl, nvalid, sl, slot, pass, pre);
                __syncthreads();
                if (t < S && !dead[t]) {
                    int digit = 0;
                    rank[j][t] = stack_bin_walk(hist + t, S, rank[j][t], &digit);
                    prefix[j][t] = (prefix[j][t] << 8) | (uint32_t)digit;
                }
            }
        }
        __syncthreads();
        if (t < P.n_q * S) {
            const int j = t / S, c = t % S;
            const long long x = x0 + stack_column_pixel(c, V);
            if (x < x1) P.out[((long long)j * P.H + y) * P.W + x] = dead[c] ? NAN : (float)stack_value<T>(prefix[j][c]);
        }
    }
}

// ---- apply ------------------------------------------------------------------------------------------------------------------------------
constexpr int kPlaneThreads = 256;                          // four waves, one row y each
constexpr int kPlaneRows = kPlaneThreads / 64;
constexpr int kPlaneBatch = 4;                              // planes a lane has loaded before it stores them
constexpr long long kPlaneTargetRows = 8192;               // (row, z slab) items wanted at least, so that short stacks of rows still fill the device

struct PlaneArgs : TileApplyArgs {
    int slab, n_slabs;                                      // planes per z slab; slabs
    const float2* coeff;                                    // (ny, nx): (a, b)
};

// one pixel column x of row y through the planes [z0, z1)
template <typename TIn, typename TOut>
__device__ __forceinline__ void plane_column(const PlaneArgs& P, const TIn* src, TOut* dst, int x, int z0, int z1, long long out_sz) {
    const float2 c = P.coeff[x];
    for (int z = z0; z < z1; ++z) {
        const TIn raw = src[(long long)(z - z0) * P.in_sz + x];
        dst[(long long)(z - z0) * out_sz + x] = tile_store<TOut>(c.x * (float)raw + c.y);
    }
}

// A wave takes one row y and one slab of planes.  Every lane loads the coefficient pairs of V consecutive pixels once and walks z
// with one load and one store of V elements each (16 bytes on the wider side); a scalar head up to the row's first aligned
// element and a scalar tail go pixel by pixel, as does the whole row when the input and output alignments differ or change from
// plane to plane.  A voxel is read and written by the same lane, read first: out may be the input itself.
template <typename TIn, typename TOut, int V>
__global__ __launch_bounds__(kPlaneThreads) void plane_apply_kernel(PlaneArgs P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long items = (long long)P.ny * P.n_slabs;
    const long long out_sz = (long long)P.ny * P.nx;
    using VIn = TileVec<TIn, V>;
    using VOut = TileVec<TOut, V>;
    PlaneArgs Q = P;
    for (long long item = (long long)blockIdx.x * kPlaneRows + wave; item < items; item += (long long)gridDim.x * kPlaneRows) {
        const int y = (int)(item % P.ny), z0 = (int)(item / P.ny) * P.slab, z1 = min(z0 + P.slab, P.nz);
        const TIn* src = (const TIn*)P.in + (long long)z0 * P.in_sz + (long long)y * P.in_sy;
        TOut* dst = (TOut*)P.out + (long long)z0 * out_sz + (long long)y * P.nx;
        Q.coeff = P.coeff + (long long)y * P.nx;
        // (planes keep the row's alignment iff the plane pitches are multiples of the vectors)
        const bool pitches = z1 - z0 == 1 || (!((P.in_sz * (long long)sizeof(TIn)) % (long long)(V * sizeof(TIn))) &&
                                              !((out_sz * (long long)sizeof(TOut)) % (long long)(V * sizeof(TOut))));
        const TileRowSplit split = tile_row_split((unsigned long long)src, (unsigned long long)dst, P.nx, sizeof(TIn), sizeof(TOut), V, pitches);
        const int head = split.head, nvec = split.nvec, tail = split.tail;
        for (int x = lane; x < head; x += 64) plane_column<TIn, TOut>(Q, src, dst, x, z0, z1, out_sz);
        for (int j = lane; j < nvec; j += 64) {
            const int x0 = head + j * V;
            float2 c[V];
#pragma unroll
            for (int k = 0; k < V; ++k) c[k] = Q.coeff[x0 + k];
            for (int z = z0; z < z1; z += kPlaneBatch) {        // kPlaneBatch loads in flight, then their stores
                VIn vi[kPlaneBatch];
#pragma unroll
                for (int u = 0; u < kPlaneBatch; ++u)
                    if (z + u < z1) vi[u] = *(const VIn*)(src + (long long)(z + u - z0) * P.in_sz + x0);
#pragma unroll
                for (int u = 0; u < kPlaneBatch; ++u) {
                    if (z + u >= z1) continue;
                    VOut vo;
#pragma unroll
                    for (int k = 0; k < V; ++k) vo.v[k] = tile_store<TOut>(c[k].x * (float)vi[u].v[k] + c[k].y);
                    *(VOut*)(dst + (long long)(z + u - z0) * out_sz + x0) = vo;
                }
            }
        }
        for (int x = tail + lane; x < P.nx; x += 64) plane_column<TIn, TOut>(Q, src, dst, x, z0, z1, out_sz);
    }
}

template <typename TIn, typename TOut>
void launch_plane_apply(const PlaneArgs& P, int nblocks, hipStream_t s) {
    hipLaunchKernelGGL((plane_apply_kernel<TIn, TOut, tile_vec_len<TIn, TOut>()>), dim3(nblocks), dim3(kPlaneThreads), 0, s, P);
}

}  // namespace

extern "C" int mvs_stack_quantiles(int device, const mvs_view_t* views, int32_t n_views, int32_t ndim, const double* q, int32_t n_q, float* out,
                                   int32_t* count_out) {
    const char* what = "mvs_stack_quantiles";
    MvsContext* c0 = mvs_ctx(device);
    if (!views || !q || !out || !count_out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", what);
    if (n_views < 1 || n_views > MVS_STACK_MAX_VIEWS) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: n_views must be 1..%d", what, MVS_STACK_MAX_VIEWS);
    if (n_q < 1 || n_q > MVS_STACK_MAX_QUANTILES) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: n_q must be 1..%d", what, MVS_STACK_MAX_QUANTILES);
    for (int j = 0; j < n_q; ++j)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: q[%d] = %g is not in [0, 1]", what, j, q[j]);
    const int dtype = views[0].dtype;
    const size_t es = mvs_dtype_size(dtype);
    if (!es) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: dtype %d (uint8 / uint16 / float32)", what, dtype);
    const long long H = views[0].shape[1], W = views[0].shape[2];
    long long planes = 0;
    size_t host_bytes = 0;
    for (int i = 0; i < n_views; ++i) {
        const mvs_view_t& v = views[i];
        if (!v.data) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: view %d without data", what, i);
        if (v.mem != MVS_MEM_HOST && v.mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: view %d: bad mem", what, i);
        if (v.dtype != dtype) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: the views must share one dtype (%d and %d given)", what, dtype, v.dtype);
        for (int k = 0; k < 3; ++k)
            if (v.shape[k] < 1 || v.shape[k] > 0x7fffffffLL) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: view %d: shape[%d] out of range", what, i, k);
        if (v.shape[1] != H || v.shape[2] != W) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: the views must share one (H, W)", what);
        if (ndim == 2 && v.shape[0] != 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: 2D views have shape[0] == 1", what);
        if (v.stride[2] != 1) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: view %d: the stride along x must be 1", what, i);
        planes += v.shape[0];
        if (planes > 0x7fffffffLL) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 samples per pixel", what);
        if (v.mem == MVS_MEM_HOST) host_bytes += align_up((size_t)v.shape[0] * H * W * es);
    }
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    // host views are packed into one block for the duration of the call, row by row where they are strided
    MvsWorkArea area(c);
    if (host_bytes) {
        rc = area.alloc(host_bytes);
        if (rc) return rc;
    }
    std::vector<StackView> table((size_t)n_views);
    size_t cursor = 0;
    const size_t row_bytes = (size_t)W * es;
    for (int i = 0; i < n_views; ++i) {
        const mvs_view_t& v = views[i];
        StackView& sv = table[i];
        sv.nz = v.shape[0];
        if (v.mem == MVS_MEM_DEVICE) {
            sv.data = (const char*)v.data;
            sv.sz = v.stride[0] * (long long)es;
            sv.sy = v.stride[1] * (long long)es;
            continue;
        }
        char* dst = (char*)area.ptr + cursor;
        sv.data = dst;
        sv.sy = (long long)row_bytes;
        sv.sz = (long long)(row_bytes * (size_t)H);
        const char* src = (const char*)v.data;
        if (v.stride[1] == W && (v.stride[0] == H * W || v.shape[0] == 1)) {
            MVS_HIP_TRY(c, hipMemcpyAsync(dst, src, (size_t)v.shape[0] * H * row_bytes, hipMemcpyHostToDevice, c->stream));
        } else {
            for (long long z = 0; z < v.shape[0]; ++z) {
                const char* plane = src + z * v.stride[0] * (long long)es;
                char* dplane = dst + (size_t)z * H * row_bytes;
                if (v.stride[1] == W) {
                    MVS_HIP_TRY(c, hipMemcpyAsync(dplane, plane, (size_t)H * row_bytes, hipMemcpyHostToDevice, c->stream));
                } else {
                    for (long long y = 0; y < H; ++y)
                        MVS_HIP_TRY(c, hipMemcpyAsync(dplane + (size_t)y * row_bytes, plane + y * v.stride[1] * (long long)es, row_bytes,
                                                      hipMemcpyHostToDevice, c->stream));
                }
            }
        }
        cursor += align_up((size_t)v.shape[0] * H * row_bytes);
    }

    const StackPlan plan = stack_plan(W, (int)es);
    StackArgs P;
    P.n_views = n_views;
    P.n_q = n_q;
    P.H = H;
    P.W = W;
    P.n_strips = plan.n_strips;
    P.n_items = H * (long long)plan.n_strips;
    for (int j = 0; j < MVS_STACK_MAX_QUANTILES; ++j) P.q[j] = j < n_q ? q[j] : 0.0;
    const size_t out_bytes = sizeof(float) * (size_t)n_q * H * W, count_bytes = sizeof(int) * (size_t)H * W;
    char* res = (char*)mvs_scratch(c, 1, align_up(out_bytes) + count_bytes);
    if (!res) return mvs_alloc_failed(c);
    P.out = (float*)res;
    P.count = (int*)(res + align_up(out_bytes));
    char* tab = (char*)mvs_scratch(c, 2, sizeof(StackView) * (size_t)n_views);
    if (!tab) return mvs_alloc_failed(c);
    P.views = (const StackView*)tab;
    // (pageable source: the copy has left the host buffer when the call returns)
    MVS_HIP_TRY(c, hipMemcpyAsync(tab, table.data(), sizeof(StackView) * (size_t)n_views, hipMemcpyHostToDevice, c->stream));

    const int nblocks = (int)std::min<long long>(P.n_items, kStackMaxBlocks);
    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    mvs_dispatch_dtype(dtype, [&](auto tag) {
        hipLaunchKernelGGL((stack_quantiles_kernel<decltype(tag)>), dim3(nblocks), dim3(kStackThreads), 0, c->stream, P);
    });
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    MVS_HIP_TRY(c, hipMemcpyAsync(out, P.out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipMemcpyAsync(count_out, P.count, count_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return host_bytes ? area.release() : MVS_OK;
}

extern "C" int mvs_plane_apply(int device, const mvs_view_t* view, int32_t ndim, const float* coeff, int32_t coeff_mem, void* out, int32_t out_dtype,
                               int32_t out_mem) {
    const char* what = "mvs_plane_apply";
    MvsContext* c0 = mvs_ctx(device);
    if (!view || !coeff || !out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (coeff_mem != MVS_MEM_HOST && coeff_mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: bad coeff_mem", what);
    PlaneArgs P;
    int nblocks = 0;
    hipStream_t stream = nullptr;
    auto prepare = [&](MvsContext* c, const TileApplyArgs& A) -> int {
        stream = c->stream;
        static_cast<TileApplyArgs&>(P) = A;
        P.coeff = (const float2*)coeff;
        if (coeff_mem == MVS_MEM_HOST) {
            const size_t coeff_bytes = sizeof(float) * 2 * (size_t)P.ny * P.nx;
            void* cd = mvs_scratch(c, 2, coeff_bytes);
            if (!cd) return mvs_alloc_failed(c);
            MVS_HIP_TRY(c, hipMemcpyAsync(cd, coeff, coeff_bytes, hipMemcpyHostToDevice, c->stream));
            P.coeff = (const float2*)cd;
        }
        // z slabs: as few as give kPlaneTargetRows (row, slab) items, so that a lane's coefficients serve as many planes as possible
        const long long want = (kPlaneTargetRows + P.ny - 1) / P.ny;
        P.n_slabs = (int)std::max<long long>(1, std::min<long long>(P.nz, want));
        P.slab = (P.nz + P.n_slabs - 1) / P.n_slabs;
        P.n_slabs = (P.nz + P.slab - 1) / P.slab;
        const long long items = (long long)P.ny * P.n_slabs;
        nblocks = (int)std::min<long long>((items + kPlaneRows - 1) / kPlaneRows, 1 << 20);
        return MVS_OK;
    };
    return mvs_tile_apply(device, what, view, ndim, out, out_dtype, out_mem, prepare, [&](auto tin, auto tout) {
        launch_plane_apply<decltype(tin), decltype(tout)>(P, nblocks, stream);
    });
}
