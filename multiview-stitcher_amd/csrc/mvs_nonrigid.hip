// mvs_nonrigid.hip -- non-rigid tile refinement (nonrigid.fit_fields / apply_fields) on gfx950: block matching over the overlap grid
// of a pair, and the kernel that warps a whole tile by a coarse displacement field.
//
// The reference has no counterpart; BigStitcher's non-rigid fusion is the model.  Every view carries a grid of cells with one
// displacement vector per cell (mvs_intensity_dev.h: the cell rule).  The fit needs, per block of a pair's overlap grid, the shift
// that aligns the two tiles best: mvs_block_match gives the six moments of every integer shift of a search window, with the voxel
// rule and the reduction of mvs_pair_moments (mvs_pair_voxel_dev.h, mvs_pair_metrics_dev.h); the peak, its sub-pixel refinement and
// the solve are host algebra (nonrigid.py).  mvs_field_warp is a gather: I'(p) = I(clamp(p + d(p))), d interpolated multilinearly
// between the cell centres as mvs_intensity_apply interpolates its coefficients.
#include "mvs_internal.h"
#include "mvs_fuse_dev.h"
#include "mvs_pair_voxel_dev.h"
#include "mvs_pair_frame.h"
#include "mvs_intensity_dev.h"
#include "mvs_tile_apply.h"

#include <algorithm>
#include <cmath>
#include <cstring>

static_assert(MVS_BLOCKMATCH_MAX_FLOATS * sizeof(float) <= 60 * 1024, "the static LDS of the block-match kernel");
static_assert(sizeof(mvs_block_t) == 48, "a block is six int64");
static_assert(MVS_FIELD_MAX_NODES == MVS_INTENSITY_MAX_CELLS, "one cell rule, one table format");

namespace {

// ---- block matching ---------------------------------------------------------------------------------------------------------------
constexpr int kMatchThreads = 256;
constexpr int kMatchWaves = kMatchThreads / 64;

struct MatchArgs {
    DevView fixed, moving;                          // matrix / offset: grid index -> pixel of the tile
    double hs[MVS_PAIR_MAX_HALFSPACES][4];          // a_z, a_y, a_x, b in grid index coordinates
    int n_hs;
    int r[3];
    const mvs_block_t* blocks;
    PairMoments* out;                               // n_blocks * S rows
};
static_assert(sizeof(MatchArgs) <= 4096, "kernel arguments");

// One workgroup per block.  samples[0, nf) holds the block of the fixed tile, samples[nf, nf + ng) the block of the moving tile grown
// by r on every side, both x fastest, NaN where a pair with that sample is not counted.  The host has checked nf + ng <=
// MVS_BLOCKMATCH_MAX_FLOATS; block voxel (z, y, x) under shift index (sz, sy, sx), 0 <= s_k <= 2 r_k, reads grown voxel
// (z + sz, y + sy, x + sx), and 0 <= z + sz < n_z + 2 r_z by construction (likewise y, x).
template <typename T>
__global__ __launch_bounds__(kMatchThreads) void block_match_kernel(MatchArgs P) {
    __shared__ float samples[MVS_BLOCKMATCH_MAX_FLOATS];
    const mvs_block_t B = P.blocks[blockIdx.x];
    const int nz = (int)B.n[0], ny = (int)B.n[1], nx = (int)B.n[2];
    const int gz = nz + 2 * P.r[0], gy = ny + 2 * P.r[1], gx = nx + 2 * P.r[2];
    const int nf = nz * ny * nx, ng = gz * gy * gx;
    const float nan = __int_as_float(0x7fc00000);
    float* F = samples;
    float* M = samples + nf;

    for (int i = threadIdx.x; i < nf; i += kMatchThreads) {
        const int t = i / nx;
        const double px = (double)(B.lo[2] + i % nx), py = (double)(B.lo[1] + t % ny), pz = (double)(B.lo[0] + t / ny);
        float v = nan, f;
        if (pair_mask_holds(P.hs, P.n_hs, pz, py, px)) {
            double cz, cy, cx;
            pair_grid_to_pixel(P.fixed.m, P.fixed.off, pz, py, px, cz, cy, cx);
            if (pair_sample_finite<T>(P.fixed, cz, cy, cx, &f)) v = f;
        }
        F[i] = v;
    }
    for (int i = threadIdx.x; i < ng; i += kMatchThreads) {
        const int t = i / gx;
        const double px = (double)(B.lo[2] - P.r[2] + i % gx), py = (double)(B.lo[1] - P.r[1] + t % gy), pz = (double)(B.lo[0] - P.r[0] + t / gy);
        double cz, cy, cx;
        pair_grid_to_pixel(P.moving.m, P.moving.off, pz, py, px, cz, cy, cx);
        float v;
        M[i] = pair_sample_finite<T>(P.moving, cz, cy, cx, &v) ? v : nan;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wy = 2 * P.r[1] + 1, wx = 2 * P.r[2] + 1;
    const int S = (2 * P.r[0] + 1) * wy * wx;
    // a lane's voxels l, l + 64, ...: (z, y, x) advances by 64 voxels without a division
    const int dx = 64 % nx, dy = (64 / nx) % ny, dz = 64 / (nx * ny);
    const int x0 = lane % nx, y0 = (lane / nx) % ny, z0 = lane / (nx * ny);
    PairMoments* rows = P.out + (long long)blockIdx.x * S;
    for (int s = wave; s < S; s += kMatchWaves) {
        const int sx = s % wx, sy = (s / wx) % wy, sz = s / (wx * wy);
        const int shift = (sz * gy + sy) * gx + sx;
        PairSums acc = PairSums{0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int x = x0, y = y0, z = z0;
        for (int i = lane; i < nf; i += 64) {
            const float f = F[i], m = M[(z * gy + y) * gx + x + shift];
            if (!isnan(f) && !isnan(m)) pair_sums_add(acc, f, m);
            x += dx;
            if (x >= nx) { x -= nx; ++y; }
            y += dy;
            if (y >= ny) { y -= ny; ++z; }
            z += dz;
        }
        const PairMoments w = mvs_fold::wave_fold(pair_sums_to_moments(acc));
        if (lane == 0) rows[s] = w;
    }
}

// ---- warp --------------------------------------------------------------------------------------------------------------------------
constexpr int kWarpThreads = 256;                   // four waves, one row each per step
constexpr int kWarpRows = kWarpThreads / 64;
constexpr int kWarpMaxBlocks = 16384;

struct WarpArgs : TileApplyArgs {
    DevView view;                                   // the input tile for sample_view: data, strides, shape
    const float* field;                             // (gz, gy, gx, 3)
    const int* cell[3];                             // per axis and pixel: lower cell index ...
    const float* frac[3];                           // ... and interpolation weight
    int gz, gy, gx, has_z;
};

__device__ __forceinline__ double warp_clamp(double c, int n) {
    const double hi = (double)(n - 1);
    return !(c >= 0.0) ? 0.0 : (c > hi ? hi : c);   // min(max(c, 0), n - 1); a NaN (an overflow of the interpolation) goes to 0, never out of bounds
}

template <typename TIn, typename TOut>
__device__ __forceinline__ TOut warp_voxel(const WarpArgs& P, const float* d, int z, int y, int x) {
    const int i = min(max(P.cell[2][x], 0), P.gx - 1);      // (a table entry outside the cells cannot leave the row's vectors)
    const int i1 = min(i + 1, P.gx - 1);
    const float t = P.frac[2][x];
    const float dz = P.has_z ? intensity_lerp(d[3 * i], d[3 * i1], t) : 0.f;
    const float dy = intensity_lerp(d[3 * i + 1], d[3 * i1 + 1], t), dx = intensity_lerp(d[3 * i + 2], d[3 * i1 + 2], t);
    const double cz = warp_clamp((double)z + (double)dz, P.nz), cy = warp_clamp((double)y + (double)dy, P.ny);
    const double cx = warp_clamp((double)x + (double)dx, P.nx);
    return tile_store<TOut>(sample_view<TIn, 1>(P.view, cz, cy, cx));
}

// A wave takes one row (z, y) at a time.  Its first gx lanes interpolate the row's displacement vectors along z, then y, into LDS;
// then every lane interpolates along x, clamps and gathers V consecutive voxels per step and stores them at once (16 bytes), with a
// scalar head up to the first aligned output element of the row and a scalar tail.
template <typename TIn, typename TOut, int V>
__global__ __launch_bounds__(kWarpThreads) void field_warp_kernel(WarpArgs P) {
    __shared__ float row_d[kWarpRows][MVS_FIELD_MAX_NODES * 3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long rows = (long long)P.nz * P.ny;
    TOut* out = (TOut*)P.out;
    using VOut = TileVec<TOut, V>;
    for (long long base = (long long)blockIdx.x * kWarpRows; base < rows; base += (long long)gridDim.x * kWarpRows) {
        const long long row = base + wave;
        const bool live = row < rows;
        const int z = live ? (int)(row / P.ny) : 0, y = live ? (int)(row % P.ny) : 0;
        __syncthreads();                            // the readers of the previous step are done with row_d
        if (live && lane < P.gx) {
            const int iz = min(max(P.cell[0][z], 0), P.gz - 1), iy = min(max(P.cell[1][y], 0), P.gy - 1);
            const int iz1 = min(iz + 1, P.gz - 1), iy1 = min(iy + 1, P.gy - 1);
            const float tz = P.frac[0][z], ty = P.frac[1][y];
            const float* c00 = P.field + 3 * (((long long)iz * P.gy + iy) * P.gx + lane);
            const float* c10 = P.field + 3 * (((long long)iz1 * P.gy + iy) * P.gx + lane);
            const float* c01 = P.field + 3 * (((long long)iz * P.gy + iy1) * P.gx + lane);
            const float* c11 = P.field + 3 * (((long long)iz1 * P.gy + iy1) * P.gx + lane);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                row_d[wave][3 * lane + k] = intensity_lerp(intensity_lerp(c00[k], c10[k], tz), intensity_lerp(c01[k], c11[k], tz), ty);
        }
        __syncthreads();
        if (!live) continue;
        const float* d = row_d[wave];
        TOut* dst = out + row * P.nx;
        const TileRowSplit split = tile_row_split((unsigned long long)dst, (unsigned long long)dst, P.nx, sizeof(TOut), sizeof(TOut), V, true);
        const int head = split.head, nvec = split.nvec, tail = split.tail;
        for (int x = lane; x < head; x += 64) dst[x] = warp_voxel<TIn, TOut>(P, d, z, y, x);
        for (int j = lane; j < nvec; j += 64) {
            const int x0 = head + j * V;
            VOut vo;
#pragma unroll
            for (int k = 0; k < V; ++k) vo.v[k] = warp_voxel<TIn, TOut>(P, d, z, y, x0 + k);
            *(VOut*)(dst + x0) = vo;
        }
        for (int x = tail + lane; x < P.nx; x += 64) dst[x] = warp_voxel<TIn, TOut>(P, d, z, y, x);
    }
}

template <typename TIn, typename TOut>
void launch_warp(const WarpArgs& P, int nblocks, hipStream_t s) {
    hipLaunchKernelGGL((field_warp_kernel<TIn, TOut, 16 / (int)sizeof(TOut)>), dim3(nblocks), dim3(kWarpThreads), 0, s, P);
}

// bytes [lo, hi) a tile view covers in its memory
void view_extent(const mvs_view_t* v, const char** lo, const char** hi) {
    const long long es = (long long)mvs_dtype_size(v->dtype);
    const long long sz = v->mem == MVS_MEM_HOST ? v->shape[1] * v->shape[2] : v->stride[0], sy = v->mem == MVS_MEM_HOST ? v->shape[2] : v->stride[1];
    *lo = (const char*)v->data;
    *hi = *lo + ((v->shape[0] - 1) * sz + (v->shape[1] - 1) * sy + v->shape[2]) * es;
}

}  // namespace

extern "C" int mvs_block_match(int device, const mvs_view_t* fixed, const mvs_view_t* moving, int32_t ndim, const double* halfspaces,
                               int32_t n_halfspaces, const mvs_block_t* blocks, int32_t n_blocks, const int32_t radius[3], double* out) {
    const char* what = "mvs_block_match";
    MvsContext* c0 = mvs_ctx(device);
    if (!fixed || !moving || !blocks || !radius || !out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    int rc = mvs_pair_check_counts(c0, what, ndim, halfspaces, n_halfspaces);
    if (rc) return rc;
    long long S = 1;
    for (int k = 0; k < 3; ++k) {
        if (radius[k] < 0 || (k < 3 - ndim && radius[k] != 0)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: radius[%d] = %d (0 along z in 2D)", what, k, (int)radius[k]);
        if (radius[k] > MVS_BLOCKMATCH_MAX_RADIUS)
            return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: radius[%d] = %d exceeds %d", what, k, (int)radius[k], MVS_BLOCKMATCH_MAX_RADIUS);
        S *= 2 * radius[k] + 1;
    }
    if (n_blocks < 1 || n_blocks > MVS_BLOCKMATCH_MAX_BLOCKS || (long long)n_blocks * S * (long long)sizeof(PairMoments) > MVS_BLOCKMATCH_MAX_RESULT_BYTES)
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: n_blocks must be 1..%d and the result at most %d bytes (%d blocks of %lld shifts given)", what,
                        MVS_BLOCKMATCH_MAX_BLOCKS, MVS_BLOCKMATCH_MAX_RESULT_BYTES, (int)n_blocks, S);
    rc = mvs_pair_check_views(c0, what, fixed, moving, ndim);
    if (rc) return rc;
    for (int b = 0; b < n_blocks; ++b) {
        const mvs_block_t& B = blocks[b];
        long long nf = 1, ng = 1;
        for (int k = 0; k < 3; ++k) {
            if (B.n[k] < 1 || B.n[k] > MVS_BLOCKMATCH_MAX_FLOATS || B.lo[k] < -0x3fffffffLL || B.lo[k] > 0x3fffffffLL || (k < 3 - ndim && (B.n[k] != 1 || B.lo[k] != 0)))
                return B.n[k] > MVS_BLOCKMATCH_MAX_FLOATS ? mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: block %d: %lld voxels along axis %d", what, b, (long long)B.n[k], k)
                                                          : mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: block %d: bad box on axis %d", what, b, k);
            nf *= B.n[k];
            ng *= B.n[k] + 2 * radius[k];
        }
        if (nf + ng > MVS_BLOCKMATCH_MAX_FLOATS)
            return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: block %d: %lld + %lld samples exceed the %d that fit the LDS", what, b, nf, ng, MVS_BLOCKMATCH_MAX_FLOATS);
    }
    MatchArgs P;
    for (int k = 0; k < 3; ++k) P.r[k] = radius[k];
    const size_t block_bytes = sizeof(mvs_block_t) * (size_t)n_blocks, out_bytes = sizeof(PairMoments) * (size_t)n_blocks * (size_t)S;
    auto prepare = [&](MvsContext* c, void**, void** dev) -> int {
        void* dblocks = mvs_scratch(c, 2, block_bytes);
        if (!dblocks) return mvs_alloc_failed(c);
        P.blocks = (const mvs_block_t*)dblocks;
        P.out = (PairMoments*)mvs_scratch(c, 1, out_bytes);
        if (!(*dev = P.out)) return mvs_alloc_failed(c);
        // (pageable source: the copy has left the host buffer when the call returns)
        MVS_HIP_TRY(c, hipMemcpyAsync(dblocks, blocks, block_bytes, hipMemcpyHostToDevice, c->stream));
        return MVS_OK;
    };
    return mvs_pair_frame(device, fixed, moving, ndim, halfspaces, n_halfspaces, P, out, out_bytes, prepare,
        [&](auto tag, hipStream_t s) { hipLaunchKernelGGL((block_match_kernel<decltype(tag)>), dim3(n_blocks), dim3(kMatchThreads), 0, s, P); }, [](hipStream_t, void*) {});
}

extern "C" int mvs_field_warp(int device, const mvs_view_t* view, int32_t ndim, const int32_t nodes[3], const float* field, const void* tables,
                              void* out, int32_t out_dtype, int32_t out_mem) {
    const char* what = "mvs_field_warp";
    MvsContext* c0 = mvs_ctx(device);
    if (!view || !nodes || !field || !tables || !out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", what);
    for (int k = 0; k < 3; ++k)
        if (nodes[k] < 1 || nodes[k] > MVS_FIELD_MAX_NODES || (k < 3 - ndim && nodes[k] != 1))
            return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: nodes[%d] = %d, must be 1..%d (and 1 along z in 2D)", what, k, (int)nodes[k], MVS_FIELD_MAX_NODES);
    const size_t n_cells = (size_t)nodes[0] * nodes[1] * nodes[2];
    for (size_t i = 0; i < 3 * n_cells; ++i)
        if (!std::isfinite(field[i]) && !(ndim == 2 && i % 3 == 0)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: the field must be finite", what);
    int rc = mvs_check_tile_view(c0, what, view, ndim);
    if (rc) return rc;
    for (int k = 0; k < 3; ++k)
        if (view->shape[k] < 1 || view->shape[k] > 0x7fffffffLL) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: view shape[%d] out of range", what, k);
    if (view->mem == out_mem && mvs_dtype_size(out_dtype)) {
        const char *lo, *hi;
        view_extent(view, &lo, &hi);
        const char* olo = (const char*)out;
        const char* ohi = olo + (size_t)view->shape[0] * view->shape[1] * view->shape[2] * mvs_dtype_size(out_dtype);
        if (olo < hi && lo < ohi) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: out overlaps the view (the kernel gathers: never in place)", what);
    }
    WarpArgs P = {};
    int nblocks = 0;
    hipStream_t stream = nullptr;
    auto prepare = [&](MvsContext* c, const TileApplyArgs& A) -> int {
        stream = c->stream;
        static_cast<TileApplyArgs&>(P) = A;
        P.gz = nodes[0]; P.gy = nodes[1]; P.gx = nodes[2];
        P.has_z = ndim == 3;
        P.view.data = A.in;
        P.view.stride_z = A.in_sz; P.view.stride_y = A.in_sy;
        P.view.nz = A.nz; P.view.ny = A.ny; P.view.nx = A.nx;
        const float* dfield = nullptr;
        int rc2 = mvs_tile_apply_tables(c, view, field, sizeof(float) * 3 * n_cells, tables, (const void**)&dfield, P.cell, P.frac);
        if (rc2) return rc2;
        P.field = dfield;
        const long long rows = (long long)P.nz * P.ny;
        nblocks = (int)std::min<long long>((rows + kWarpRows - 1) / kWarpRows, kWarpMaxBlocks);
        return MVS_OK;
    };
    return mvs_tile_apply(device, what, view, ndim, out, out_dtype, out_mem, prepare, [&](auto tin, auto tout) {
        launch_warp<decltype(tin), decltype(tout)>(P, nblocks, stream);
    });
}
