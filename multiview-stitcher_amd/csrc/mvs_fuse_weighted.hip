// mvs_fuse_weighted.hip -- mvs_fuse_chunk_weighted: the generic fuse kernel with one feathered uint8 weight tile per view
// (masks.feather) next to the image.  Per output voxel and view, in view order: the image sample, the in-bounds test and the blend
// weight b exactly as fuse_kernel (mvs_fuse.hip) forms them (mvs_sample_dev.h, mvs_fuse_blend_dev.h), then m = the linear sample of
// the weight tile / 252 at coordinates clamped into the tile, as a float32.  A view takes part where it is in bounds, its sample is not NaN and
// m > 0; the weighted average weighs it with b m, max and simple average run over the views that take part.  Bricks, the culling of
// views per brick and the epilogue (nan_to_num, halo trim, truncating cast) are fuse_kernel's; the host frame is
// mvs_fuse_chunk_plan.h's.  With m == 1 the float32 operations of a voxel are those of fuse_kernel, in the same order.
#include "mvs_internal.h"
#include "mvs_fuse_dev.h"
#include "mvs_sample_dev.h"
#include "mvs_fuse_blend_dev.h"
#include "mvs_fuse_chunk_plan.h"

#include <cmath>
#include <cstring>

using namespace mvs_fuse_chunk_plan;

namespace {

constexpr int kLdsTables = 8;    // blend tables staged in LDS per pass, as in fuse_kernel

struct WeightedParams {
    const DevView* views;
    const WeightView* wviews;
    int nviews;
    void* out;
    int oz, oy, ox;        // shape of the (trimmed) result
    int tz, ty, tx;        // trim: chunk index = result index + trim
    int nbz, nby, nbx;     // brick grid
    int bz, by;            // brick extent along z and y
};

// lower tap, upper tap (n - 1 at the upper border) and the weight of the upper tap of a coordinate clamped into [0, n - 1]
__device__ __forceinline__ void clamped_taps(double c, int n, int& i0, int& i1, double& w) {
    c = fmin(fmax(c, 0.0), (double)(n - 1));      // (a NaN coordinate becomes 0)
    const double f = floor(c);
    i0 = (int)f;
    i1 = min(i0 + 1, n - 1);
    w = c - f;
}

__device__ __forceinline__ double weight_tap(const unsigned char* p, long long i) { return (double)min((int)p[i], MVS_FEATHER_FULL_WEIGHT); }
__device__ __forceinline__ double lerp(double u, double v, double t) { return u + t * (v - u); }      // exact where u == v

// m of a view at tile coordinates: the linear sample / 252, rounded to float32 once.  The taps are small integers and the
// coefficients come from float64 coordinates, so the interpolation stays in float64: a view takes part where m > 0, and a coordinate
// an integer -+ 1e-10 (whose float32 coefficient would be 0 or 1) must classify a tile edge as scipy's float64 sum does.  lerp is
// exact where the taps are equal: an all-252 tile gives exactly 1.
__device__ __forceinline__ float sample_weight(const WeightView& W, double cz, double cy, double cx) {
    int iz, iz1, iy, iy1, ix, ix1;
    double wz, wy, wx;
    clamped_taps(cz, W.nz, iz, iz1, wz);
    clamped_taps(cy, W.ny, iy, iy1, wy);
    clamped_taps(cx, W.nx, ix, ix1, wx);
    const unsigned char* p = W.data;
    const long long b00 = iz * W.stride_z + iy * W.stride_y, b01 = iz * W.stride_z + iy1 * W.stride_y;
    double s = lerp(lerp(weight_tap(p, b00 + ix), weight_tap(p, b00 + ix1), wx), lerp(weight_tap(p, b01 + ix), weight_tap(p, b01 + ix1), wx), wy);
    if (iz1 != iz) {
        const long long b10 = iz1 * W.stride_z + iy * W.stride_y, b11 = iz1 * W.stride_z + iy1 * W.stride_y;
        const double s1 = lerp(lerp(weight_tap(p, b10 + ix), weight_tap(p, b10 + ix1), wx), lerp(weight_tap(p, b11 + ix), weight_tap(p, b11 + ix1), wx), wy);
        s = lerp(s, s1, wz);
    }
    return (float)(s / (double)MVS_FEATHER_FULL_WEIGHT);
}

template <typename TIn, typename TOut, int ORDER, int FUSION>
__global__ __launch_bounds__(256) void fuse_weighted_kernel(WeightedParams P) {
    __shared__ int s_act[64];
    __shared__ int s_nact;
    __shared__ float s_edt[kLdsTables][128];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    int b = blockIdx.x;
    const int bx = b % P.nbx;
    b /= P.nbx;
    const int byi = b % P.nby;
    const int bzi = b / P.nby;

    const int lx = lane & 15, ly = lane >> 4;
    int z, y;
    if (P.bz == 4) {
        z = bzi * 4 + wave;
        y = byi * 4 + ly;
    } else {
        z = bzi;
        y = byi * 16 + wave * 4 + ly;
    }
    const int x0 = bx * kBrickX + lx * kVPT;
    const bool row_ok = (z < P.oz) && (y < P.oy) && (x0 < P.ox);

    int lo[3] = {bzi * P.bz + P.tz, byi * P.by + P.ty, bx * kBrickX + P.tx};
    int hi[3] = {min(bzi * P.bz + P.bz, P.oz) - 1 + P.tz, min(byi * P.by + P.by, P.oy) - 1 + P.ty,
                 min(bx * kBrickX + kBrickX, P.ox) - 1 + P.tx};

    const double pz = (double)(z + P.tz), py = (double)(y + P.ty);
    const double px0 = (double)(x0 + P.tx);

    float acc[kVPT], den[kVPT];
#pragma unroll
    for (int j = 0; j < kVPT; ++j) {
        acc[j] = (FUSION == MVS_FUSE_MAX) ? -INFINITY : 0.f;
        den[j] = 0.f;
    }

    for (int base = 0; base < P.nviews; base += 64) {
        __syncthreads();
        if (wave == 0) {
            int v = base + lane;
            bool act = false;
            if (v < P.nviews) act = brick_hits_view(P.views[v], lo, hi);
            unsigned long long mask = __ballot(act);
            if (act) s_act[__popcll(mask & ((1ull << lane) - 1ull))] = v;
            if (lane == 0) s_nact = __popcll(mask);
        }
        __syncthreads();
        const int nact = s_nact;
        if (FUSION == MVS_FUSE_WEIGHTED_AVERAGE) {
            const int ncopy = min(nact, kLdsTables) * 125;
            for (int i = tid; i < ncopy; i += 256) {
                int a = i / 125, k = i - a * 125;
                s_edt[a][k] = P.views[s_act[a]].edt[k];
            }
            __syncthreads();
        }
        if (!row_ok) continue;

        for (int a = 0; a < nact; ++a) {
            const int vi = __builtin_amdgcn_readfirstlane(s_act[a]);
            const DevView& V = P.views[vi];
            const WeightView& W = P.wviews[vi];
            const bool has_w = W.data != nullptr;
            // row part of scipy's coordinate sum: (0 + z*m0) + y*m1
            const double rz = pz * V.m[0] + py * V.m[1];
            const double ry = pz * V.m[3] + py * V.m[4];
            const double rx = pz * V.m[6] + py * V.m[7];
            const double zmax = (double)(V.nz - 1), ymax = (double)(V.ny - 1), xmax = (double)(V.nx - 1);
            double qz = 0, qy = 0, qx = 0;
            if (has_w) {
                qz = pz * W.m[0] + py * W.m[1];
                qy = pz * W.m[3] + py * W.m[4];
                qx = pz * W.m[6] + py * W.m[7];
            }
            double wz0 = 0, wy0 = 0, wx0 = 0;
            if (FUSION == MVS_FUSE_WEIGHTED_AVERAGE) {
                wz0 = ((pz * V.wm[0] + py * V.wm[1]) + px0 * V.wm[2]) + V.woff[0];
                wy0 = ((pz * V.wm[3] + py * V.wm[4]) + px0 * V.wm[5]) + V.woff[1];
                wx0 = ((pz * V.wm[6] + py * V.wm[7]) + px0 * V.wm[8]) + V.woff[2];
            }
#pragma unroll
            for (int j = 0; j < kVPT; ++j) {
                const double px = px0 + (double)j;
                const double cz = (rz + px * V.m[2]) + V.off[0];
                const double cy = (ry + px * V.m[5]) + V.off[1];
                const double cx = (rx + px * V.m[8]) + V.off[2];
                const bool inb = !(cz < 0.0 || cz > zmax || cy < 0.0 || cy > ymax || cx < 0.0 || cx > xmax);
                if (!inb) continue;
                const float val = sample_view<TIn, ORDER>(V, cz, cy, cx);
                if (val != val) continue;   // NaN voxels are invalid (weights masked by ~isnan)
                float m = 1.f;
                if (has_w) {
                    m = sample_weight(W, (qz + px * W.m[2]) + W.off[0], (qy + px * W.m[5]) + W.off[1], (qx + px * W.m[8]) + W.off[2]);
                    if (!(m > 0.f)) continue;
                }
                if (FUSION == MVS_FUSE_WEIGHTED_AVERAGE) {
                    const double dj = (double)j;
                    const double cwz = wz0 + dj * V.wm[2], cwy = wy0 + dj * V.wm[5], cwx = wx0 + dj * V.wm[8];
                    float w;
                    if (a < kLdsTables) w = blend_weight<true>(s_edt[a], V.wnz, cwz, cwy, cwx);
                    else w = blend_weight<false>(V.edt, V.wnz, cwz, cwy, cwx);
                    wa_update(acc[j], den[j], w * m, val);
                } else if (FUSION == MVS_FUSE_MAX) {
                    acc[j] = fmaxf(acc[j], val);
                    // the views that take part, counted as the simple average counts them.  (Not `den[j] = 1.f` as in fuse_kernel: hipcc
                    // then emitted the store on the path of a view without a tile only, and every voxel of a view with one came out 0.)
                    den[j] += 1.f;
                } else {
                    acc[j] += val;
                    den[j] += 1.f;
                }
            }
        }
    }
    if (!row_ok) return;

    float r[kVPT];
#pragma unroll
    for (int j = 0; j < kVPT; ++j) {
        float o;
        if (FUSION == MVS_FUSE_MAX) o = (den[j] > 0.f) ? acc[j] : 0.f;
        else if (FUSION == MVS_FUSE_WEIGHTED_AVERAGE) o = wa_result(acc[j], den[j]);
        else o = (den[j] > 0.f) ? acc[j] / den[j] : 0.f;
        if (o != o) o = 0.f;   // nan_to_num
        r[j] = o;
    }
    store_row4<TOut>((TOut*)P.out, ((long long)z * P.oy + y) * (long long)P.ox, x0, P.ox, r);
}

template <typename T>
void launch_fuse_weighted(const WeightedParams& P, int order, int fusion, int nblocks, hipStream_t s) {
#define MVS_LAUNCH(O, F) hipLaunchKernelGGL((fuse_weighted_kernel<T, T, O, F>), dim3(nblocks), dim3(256), 0, s, P)
    if (order == 0) {
        if (fusion == MVS_FUSE_WEIGHTED_AVERAGE) MVS_LAUNCH(0, MVS_FUSE_WEIGHTED_AVERAGE);
        else if (fusion == MVS_FUSE_MAX) MVS_LAUNCH(0, MVS_FUSE_MAX);
        else MVS_LAUNCH(0, MVS_FUSE_SIMPLE_AVERAGE);
    } else {
        if (fusion == MVS_FUSE_WEIGHTED_AVERAGE) MVS_LAUNCH(1, MVS_FUSE_WEIGHTED_AVERAGE);
        else if (fusion == MVS_FUSE_MAX) MVS_LAUNCH(1, MVS_FUSE_MAX);
        else MVS_LAUNCH(1, MVS_FUSE_SIMPLE_AVERAGE);
    }
#undef MVS_LAUNCH
}

// What the entry requires of the weight tiles beyond mvs_check_chunk_args of the views
int check_weight_views(MvsContext* c, const char* what, const mvs_view_t* wviews, int n_views, int ndim) {
    for (int i = 0; i < n_views; ++i) {
        const mvs_view_t& w = wviews[i];
        if (!w.data) continue;
        if (w.dtype != MVS_U8) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: weight tile %d: weight tiles are uint8", what, i);
        if (w.mem != MVS_MEM_HOST && w.mem != MVS_MEM_DEVICE) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: weight tile %d: bad mem", what, i);
        for (int k = 0; k < 3; ++k) {
            if (w.shape[k] < 1 || w.shape[k] > 0x7fffffffLL) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: weight tile %d: shape[%d] out of range", what, i, k);
            if (w.index_offset[k] != 0) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: weight tile %d: a weight tile is whole (index_offset 0)", what, i);
        }
        if (ndim == 2 && w.shape[0] != 1) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: weight tile %d: 2D tiles have shape[0] == 1", what, i);
        if (w.stride[2] != 1) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: weight tile %d: the stride along x must be 1", what, i);
    }
    return MVS_OK;
}

}  // namespace

extern "C" int mvs_fuse_chunk_weighted(int device, const mvs_view_t* views, const mvs_view_t* wviews, int32_t n_views, const mvs_fuse_opts_t* opts,
                                       void* out) {
    const char* what = "mvs_fuse_chunk_weighted";
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    rc = mvs_check_chunk_args(c, what, views, n_views, opts, out);
    if (rc) return rc;
    if (!wviews) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: NULL/empty argument", what);
    if (opts->weights != MVS_WEIGHTS_NONE) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: view weights cannot be combined with weights %d", what, opts->weights);
    if ((rc = check_weight_views(c, what, wviews, n_views, opts->ndim))) return rc;
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    const int dtype = views[0].dtype;
    const size_t es = mvs_dtype_size(dtype);
    int64_t os[3];
    for (int k = 0; k < 3; ++k) os[k] = opts->out_shape[k] - 2 * opts->trim[k];
    const BrickGrid G = brick_grid(kGenericBricks, os);
    if (!G.fits_one_launch()) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: chunk too large for one launch", what);

    // host slabs and host weight tiles go through scratch slot 0, the records through the pinned slot into scratch slot 2
    size_t slab_bytes = 0, tile_bytes = 0;
    if ((rc = mvs_stage_views_bytes(c, views, n_views, es, &slab_bytes))) return rc;
    for (int i = 0; i < n_views; ++i) {
        size_t nb = 0;
        if (wviews[i].data && (rc = mvs_stage_views_bytes(c, &wviews[i], 1, 1, &nb))) return rc;
        tile_bytes += nb;
    }
    const size_t host_bytes = slab_bytes + tile_bytes;
    char* stage = nullptr;
    if (host_bytes && !(stage = (char*)mvs_scratch(c, 0, host_bytes))) return mvs_alloc_failed(c);
    const size_t rec_bytes = align_up(sizeof(DevView) * (size_t)n_views), total = rec_bytes + align_up(sizeof(WeightView) * (size_t)n_views);
    DevView* hviews = (DevView*)mvs_pinned(c, total);
    if (!hviews) return mvs_alloc_failed(c);
    DevView* dviews = (DevView*)mvs_scratch(c, 2, total);
    if (!dviews) return mvs_alloc_failed(c);
    WeightView* hw = (WeightView*)((char*)hviews + rec_bytes);
    size_t cursor = 0;
    for (int i = 0; i < n_views; ++i) {
        const void* dptr;
        if ((rc = mvs_stage_view(c, views[i], es, stage, &cursor, &dptr))) return rc;
        if ((rc = mvs_fill_dev_view(c, views[i], opts->ndim, dptr, &hviews[i]))) return rc;
        hviews[i].tr_ok = 0;
        view_to_chunk_frame(&hviews[i], opts->index_origin, views[i].index_offset);
        dptr = nullptr;
        if (wviews[i].data && (rc = mvs_stage_view(c, wviews[i], 1, stage, &cursor, &dptr))) return rc;
        mvs_view_t w = wviews[i];
        if (w.data && w.mem == MVS_MEM_HOST) {      // (staged C-contiguous)
            w.stride[1] = w.shape[2];
            w.stride[0] = w.shape[1] * w.shape[2];
        }
        fill_weight_view(w, dptr, opts->index_origin, &hw[i]);
    }
    if ((rc = mvs_upload_small(c, dviews, hviews, total))) return rc;
    mvs_pinned_mark(c, 0);

    const size_t out_bytes = (size_t)os[0] * os[1] * os[2] * es;
    void* dout = out;
    if (opts->out_mem == MVS_MEM_HOST && !(dout = mvs_scratch(c, 1, out_bytes))) return mvs_alloc_failed(c);

    WeightedParams P;
    P.views = dviews;
    P.wviews = (const WeightView*)((const char*)dviews + rec_bytes);
    P.nviews = n_views;
    P.out = dout;
    P.oz = (int)os[0]; P.oy = (int)os[1]; P.ox = (int)os[2];
    P.tz = (int)opts->trim[0]; P.ty = (int)opts->trim[1]; P.tx = (int)opts->trim[2];
    P.nbz = G.nbz; P.nby = G.nby; P.nbx = G.nbx;
    P.bz = G.bz; P.by = G.by;
    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    mvs_dispatch_dtype(dtype, [&](auto tag) { launch_fuse_weighted<decltype(tag)>(P, opts->order, opts->fusion, (int)G.nblocks, c->stream); });
    MVS_HIP_TRY(c, hipGetLastError());
    c->fuse_weighted_chunks += 1;
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    if (opts->out_mem == MVS_MEM_HOST) {
        MVS_HIP_TRY(c, hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, c->stream));
        MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else if (host_bytes) {
        MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return MVS_OK;
}
