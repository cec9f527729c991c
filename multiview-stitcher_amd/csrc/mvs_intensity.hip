// mvs_intensity.hip -- tile intensity harmonisation (intensity.fit_maps / apply_maps) on gfx950: the sample moments of a pair's
// overlap split by the coefficient cells of both tiles, and the kernel that applies a fitted gain / offset map to a whole tile.
//
// The reference has no counterpart; BigStitcher's "intensity adjustment in overlaps" is the model.  Every view carries a grid of
// cells with a gain a and an offset b per cell (mvs_intensity_dev.h: the cell rule).  The fit needs, per pair of cells of two
// overlapping tiles, the six moments of the sample pairs that fall into both; mvs_intensity_pair_moments gathers them with the
// voxel rule and the reduction of mvs_pair_moments (mvs_pair_voxel_dev.h, mvs_pair_metrics_dev.h) for all records of a call in one
// launch.  mvs_intensity_apply is a copy with a handful of float32 operations per voxel: I' = a(p) I + b(p), a and b interpolated
// multilinearly between the cell centres.
#include "mvs_internal.h"
#include "mvs_fuse_dev.h"
#include "mvs_pair_voxel_dev.h"
#include "mvs_pair_frame.h"
#include "mvs_intensity_dev.h"
#include "mvs_tile_apply.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

static_assert(kPairBlockThreads == MVS_INTENSITY_BLOCK_VOXELS, "constants of include/mvs_hip.h");
static_assert(sizeof(mvs_intensity_record_t) == 72, "a record is six int64 and six int32");

namespace {

constexpr int kWaves = kPairBlockThreads / 64;

// ---- moments per cell pair ---------------------------------------------------------------------------------------------------------
struct IntensityArgs {
    DevView fixed, moving;                          // matrix / offset: grid index -> pixel of the tile
    double hs[MVS_PAIR_MAX_HALFSPACES][4];          // a_z, a_y, a_x, b in grid index coordinates
    int n_hs, n_records;
    int cells_f[3], cells_m[3];
    const mvs_intensity_record_t* recs;
    const int* first_block;                         // n_records + 1: workgroups [first_block[r], first_block[r + 1]) belong to record r
    PairMoments* partial;                           // one per workgroup
};
static_assert(sizeof(IntensityArgs) <= 4096, "kernel arguments");

// workgroups of a record: a function of its voxel count only
int record_blocks(const mvs_intensity_record_t& r) {
    const long long n = (long long)r.n[0] * r.n[1] * r.n[2];
    return (int)std::max<long long>(1, std::min<long long>((n + kPairBlockThreads - 1) / kPairBlockThreads, MVS_INTENSITY_MAX_BLOCKS));
}

template <typename T>
__global__ __launch_bounds__(kPairBlockThreads) void intensity_moments_kernel(IntensityArgs P) {
    int r = 0, hi = P.n_records;                    // the last record whose first workgroup is not after this one
    while (hi - r > 1) {
        const int mid = (r + hi) >> 1;
        if (P.first_block[mid] <= (int)blockIdx.x) r = mid; else hi = mid;
    }
    const mvs_intensity_record_t R = P.recs[r];
    const int b0 = P.first_block[r];
    const long long nb = P.first_block[r + 1] - b0;
    const long long ny = R.n[1], nx = R.n[2], n = R.n[0] * ny * nx;

    PairSums acc = PairSums{0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long i = (long long)((int)blockIdx.x - b0) * kPairBlockThreads + threadIdx.x; i < n; i += nb * kPairBlockThreads) {
        const long long t = i / nx;
        const double px = (double)(R.lo[2] + i % nx), py = (double)(R.lo[1] + t % ny), pz = (double)(R.lo[0] + t / ny);
        if (!pair_mask_holds(P.hs, P.n_hs, pz, py, px)) continue;
        double fz, fy, fx;
        pair_grid_to_pixel(P.fixed.m, P.fixed.off, pz, py, px, fz, fy, fx);
        double cz, cy, cx;
        pair_grid_to_pixel(P.moving.m, P.moving.off, pz, py, px, cz, cy, cx);
        // the cell tests come before the samples (they are cheaper, and a conservative box holds voxels of other cells)
        if (!view_in_bounds(P.fixed, fz, fy, fx) || !view_in_bounds(P.moving, cz, cy, cx)) continue;
        if (intensity_cell(fz, P.cells_f[0], P.fixed.nz) != R.cell_f[0] || intensity_cell(fy, P.cells_f[1], P.fixed.ny) != R.cell_f[1] ||
            intensity_cell(fx, P.cells_f[2], P.fixed.nx) != R.cell_f[2])
            continue;
        if (intensity_cell(cz, P.cells_m[0], P.moving.nz) != R.cell_m[0] || intensity_cell(cy, P.cells_m[1], P.moving.ny) != R.cell_m[1] ||
            intensity_cell(cx, P.cells_m[2], P.moving.nx) != R.cell_m[2])
            continue;
        float f, v;
        if (!pair_sample_finite<T>(P.fixed, fz, fy, fx, &f) || !pair_sample_finite<T>(P.moving, cz, cy, cx, &v)) continue;
        pair_sums_add(acc, f, v);
    }

    __shared__ PairMoments lds[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const PairMoments w = mvs_fold::wave_fold(pair_sums_to_moments(acc));
    if (lane == 0) lds[wave] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        PairMoments m = lds[0];
        for (int k = 1; k < kWaves; ++k) m = pair_moments_merge(m, lds[k]);
        P.partial[blockIdx.x] = m;
    }
}

// One wave per record folds the results of the record's workgroups (pair_moments_fold, mvs_pair_voxel_dev.h).
__global__ __launch_bounds__(64) void intensity_fold_kernel(const PairMoments* partial, const int* first_block, PairMoments* out) {
    const int r = blockIdx.x, b0 = first_block[r];
    const PairMoments m = pair_moments_fold(partial + b0, 1, first_block[r + 1] - b0, threadIdx.x);
    if (threadIdx.x == 0) out[r] = m;
}

// ---- apply ------------------------------------------------------------------------------------------------------------------------
constexpr int kApplyThreads = 256;                  // four waves, one row each per step
constexpr int kApplyRows = kApplyThreads / 64;
constexpr int kApplyMaxBlocks = 16384;

// (gz, gy, gx come last on purpose: placed right after TileApplyArgs, 4 bytes later than they once were, the same kernels compile
// to up to 49 more VGPRs and lose up to three occupancy steps -- profiles/tile_apply_ab.txt, section 2)
struct ApplyArgs : TileApplyArgs {
    const float* coeff;                             // (gz, gy, gx, 2)
    const int* cell[3];                             // per axis and pixel: lower cell index ...
    const float* frac[3];                           // ... and interpolation weight
    int gz, gy, gx;
};

template <typename TIn, typename TOut>
__device__ __forceinline__ TOut apply_voxel(const ApplyArgs& P, const float2* ab, int x, TIn raw) {
    const int i = min(max(P.cell[2][x], 0), P.gx - 1);      // (a table entry outside the cells cannot leave the row's pairs)
    const int i1 = min(i + 1, P.gx - 1);
    const float t = P.frac[2][x];
    const float2 c0 = ab[i], c1 = ab[i1];
    const float a = intensity_lerp(c0.x, c1.x, t), b = intensity_lerp(c0.y, c1.y, t);
    return tile_store<TOut>(a * (float)raw + b);
}

// A wave takes one row (z, y) at a time.  Its first gx lanes interpolate the row's coefficient pairs along z, then y, into LDS; then
// every lane moves V consecutive voxels per step with one load and one store of V elements each (16 bytes on the wider side), with
// a scalar head up to the first aligned element of the row and a scalar tail.  Rows whose input and output alignments differ
// (a strided window copied into a dense array) go element by element.  A voxel is read and written by the same lane, read first:
// out may be the input itself.
template <typename TIn, typename TOut, int V>
__global__ __launch_bounds__(kApplyThreads) void intensity_apply_kernel(ApplyArgs P) {
    __shared__ float2 row_ab[kApplyRows][MVS_INTENSITY_MAX_CELLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long rows = (long long)P.nz * P.ny;
    const TIn* in = (const TIn*)P.in;
    TOut* out = (TOut*)P.out;
    using VIn = TileVec<TIn, V>;
    using VOut = TileVec<TOut, V>;
    for (long long base = (long long)blockIdx.x * kApplyRows; base < rows; base += (long long)gridDim.x * kApplyRows) {
        const long long row = base + wave;
        const bool live = row < rows;
        const int z = live ? (int)(row / P.ny) : 0, y = live ? (int)(row % P.ny) : 0;
        __syncthreads();                            // the readers of the previous step are done with row_ab
        if (live && lane < P.gx) {
            const int iz = min(max(P.cell[0][z], 0), P.gz - 1), iy = min(max(P.cell[1][y], 0), P.gy - 1);
            const int iz1 = min(iz + 1, P.gz - 1), iy1 = min(iy + 1, P.gy - 1);
            const float tz = P.frac[0][z], ty = P.frac[1][y];
            const float2* C = (const float2*)P.coeff;
            const float2 c00 = C[((long long)iz * P.gy + iy) * P.gx + lane], c10 = C[((long long)iz1 * P.gy + iy) * P.gx + lane];
            const float2 c01 = C[((long long)iz * P.gy + iy1) * P.gx + lane], c11 = C[((long long)iz1 * P.gy + iy1) * P.gx + lane];
            float2 r;
            r.x = intensity_lerp(intensity_lerp(c00.x, c10.x, tz), intensity_lerp(c01.x, c11.x, tz), ty);
            r.y = intensity_lerp(intensity_lerp(c00.y, c10.y, tz), intensity_lerp(c01.y, c11.y, tz), ty);
            row_ab[wave][lane] = r;
        }
        __syncthreads();
        if (!live) continue;
        const float2* ab = row_ab[wave];
        const TIn* src = in + (long long)z * P.in_sz + (long long)y * P.in_sy;
        TOut* dst = out + row * P.nx;
        const TileRowSplit split = tile_row_split((unsigned long long)src, (unsigned long long)dst, P.nx, sizeof(TIn), sizeof(TOut), V, true);
        const int head = split.head, nvec = split.nvec, tail = split.tail;
        for (int x = lane; x < head; x += 64) dst[x] = apply_voxel<TIn, TOut>(P, ab, x, src[x]);
        for (int j = lane; j < nvec; j += 64) {
            const int x0 = head + j * V;
            const VIn vi = *(const VIn*)(src + x0);
            VOut vo;
#pragma unroll
            for (int k = 0; k < V; ++k) vo.v[k] = apply_voxel<TIn, TOut>(P, ab, x0 + k, vi.v[k]);
            *(VOut*)(dst + x0) = vo;
        }
        for (int x = tail + lane; x < P.nx; x += 64) dst[x] = apply_voxel<TIn, TOut>(P, ab, x, src[x]);
    }
}

template <typename TIn, typename TOut>
void launch_apply(const ApplyArgs& P, int nblocks, hipStream_t s) {
    hipLaunchKernelGGL((intensity_apply_kernel<TIn, TOut, tile_vec_len<TIn, TOut>()>), dim3(nblocks), dim3(kApplyThreads), 0, s, P);
}

int check_cells(MvsContext* c, const char* what, const int32_t cells[3], int ndim) {
    for (int k = 0; k < 3; ++k)
        if (cells[k] < 1 || cells[k] > MVS_INTENSITY_MAX_CELLS || (k < 3 - ndim && cells[k] != 1))
            return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: cells[%d] = %d, must be 1..%d (and 1 along z in 2D)", what, k, (int)cells[k], MVS_INTENSITY_MAX_CELLS);
    return MVS_OK;
}

}  // namespace

extern "C" int mvs_intensity_pair_moments(int device, const mvs_view_t* fixed, const mvs_view_t* moving, int32_t ndim, const int32_t cells_f[3],
                                          const int32_t cells_m[3], const double* halfspaces, int32_t n_halfspaces,
                                          const mvs_intensity_record_t* records, int32_t n_records, double* out) {
    const char* what = "mvs_intensity_pair_moments";
    MvsContext* c0 = mvs_ctx(device);
    if (!fixed || !moving || !cells_f || !cells_m || !records || !out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    int rc = mvs_pair_check_counts(c0, what, ndim, halfspaces, n_halfspaces);
    if (rc) return rc;
    if (n_records < 1 || n_records > MVS_INTENSITY_MAX_RECORDS)
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: n_records must be 1..%d", what, MVS_INTENSITY_MAX_RECORDS);
    rc = check_cells(c0, what, cells_f, ndim);
    if (!rc) rc = check_cells(c0, what, cells_m, ndim);
    if (!rc) rc = mvs_pair_check_views(c0, what, fixed, moving, ndim);
    if (rc) return rc;
    std::vector<int> first_block((size_t)n_records + 1);
    first_block[0] = 0;
    for (int r = 0; r < n_records; ++r) {
        const mvs_intensity_record_t& R = records[r];
        for (int k = 0; k < 3; ++k) {
            if (R.n[k] < 1 || R.n[k] > 0x7fffffffLL || R.lo[k] < -0x7fffffffLL || R.lo[k] > 0x7fffffffLL || (k < 3 - ndim && (R.n[k] != 1 || R.lo[k] != 0)))
                return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: record %d: bad box on axis %d", what, r, k);
            if (R.cell_f[k] < 0 || R.cell_f[k] >= cells_f[k] || R.cell_m[k] < 0 || R.cell_m[k] >= cells_m[k])
                return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: record %d: cell index out of range on axis %d", what, r, k);
        }
        if ((double)R.n[0] * (double)R.n[1] * (double)R.n[2] > 9e15) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: record %d: box too large", what, r);
        first_block[r + 1] = first_block[r] + record_blocks(R);
    }
    IntensityArgs P;
    P.n_records = n_records;
    memcpy(P.cells_f, cells_f, sizeof(P.cells_f));
    memcpy(P.cells_m, cells_m, sizeof(P.cells_m));
    const int total_blocks = first_block[n_records];
    const size_t out_bytes = sizeof(PairMoments) * (size_t)n_records;
    auto prepare = [&](MvsContext* c, void** host, void** dev) -> int {
        const size_t rec_bytes = align_up(sizeof(mvs_intensity_record_t) * (size_t)n_records), fb_bytes = align_up(sizeof(int) * ((size_t)n_records + 1));
        char* tables = (char*)mvs_scratch(c, 2, rec_bytes + fb_bytes);
        if (!tables) return mvs_alloc_failed(c);
        P.recs = (const mvs_intensity_record_t*)tables;
        P.first_block = (const int*)(tables + rec_bytes);
        P.partial = (PairMoments*)mvs_scratch(c, 1, sizeof(PairMoments) * (size_t)total_blocks);
        if (!P.partial) return mvs_alloc_failed(c);
        const int rc2 = mvs_mailbox(c, out_bytes, host, dev);
        if (rc2) return rc2;
        // (pageable sources: both copies have left the host buffers when the calls return)
        MVS_HIP_TRY(c, hipMemcpyAsync(tables, records, sizeof(mvs_intensity_record_t) * (size_t)n_records, hipMemcpyHostToDevice, c->stream));
        MVS_HIP_TRY(c, hipMemcpyAsync(tables + rec_bytes, first_block.data(), sizeof(int) * ((size_t)n_records + 1), hipMemcpyHostToDevice, c->stream));
        return MVS_OK;
    };
    return mvs_pair_frame(device, fixed, moving, ndim, halfspaces, n_halfspaces, P, out, out_bytes, prepare,
        [&](auto tag, hipStream_t s) { hipLaunchKernelGGL((intensity_moments_kernel<decltype(tag)>), dim3(total_blocks), dim3(kPairBlockThreads), 0, s, P); },
        [&](hipStream_t s, void* dev) { hipLaunchKernelGGL(intensity_fold_kernel, dim3(n_records), dim3(64), 0, s, (const PairMoments*)P.partial, P.first_block, (PairMoments*)dev); });
}

extern "C" int mvs_intensity_apply(int device, const mvs_view_t* view, int32_t ndim, const int32_t cells[3], const float* coeff, const void* tables,
                                   void* out, int32_t out_dtype, int32_t out_mem) {
    const char* what = "mvs_intensity_apply";
    MvsContext* c0 = mvs_ctx(device);
    if (!view || !cells || !coeff || !tables || !out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    int rc = check_cells(c0, what, cells, ndim);
    if (rc) return rc;
    ApplyArgs P;
    int nblocks = 0;
    hipStream_t stream = nullptr;
    auto prepare = [&](MvsContext* c, const TileApplyArgs& A) -> int {
        stream = c->stream;
        static_cast<TileApplyArgs&>(P) = A;
        P.gz = cells[0]; P.gy = cells[1]; P.gx = cells[2];
        // coefficients and tables: scratch slot 2 (tables: per axis z, y, x the int32 lower cell of every pixel, then its float32 weight)
        const void* dcoeff = nullptr;
        const int rc2 = mvs_tile_apply_tables(c, view, coeff, sizeof(float) * 2 * (size_t)cells[0] * cells[1] * cells[2], tables, &dcoeff, P.cell, P.frac);
        if (rc2) return rc2;
        P.coeff = (const float*)dcoeff;
        const long long rows = (long long)P.nz * P.ny;
        nblocks = (int)std::min<long long>((rows + kApplyRows - 1) / kApplyRows, kApplyMaxBlocks);
        return MVS_OK;
    };
    return mvs_tile_apply(device, what, view, ndim, out, out_dtype, out_mem, prepare, [&](auto tin, auto tout) {
        launch_apply<decltype(tin), decltype(tout)>(P, nblocks, stream);
    });
}
