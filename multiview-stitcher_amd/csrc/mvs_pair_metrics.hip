// mvs_pair_metrics.hip -- registration quality metrics: the sample moments of a fixed and a moving tile on their overlap grid (gfx950).
//
// Replaces, per directed pair of metrics.tile_pair_image_metrics (src/multiview_stitcher/metrics.py:708-742, 87-124, 42-79):
//   1 + K x transformation.transform_sim (scipy.ndimage.affine_transform, order 1, cval NaN) of the two tiles onto the overlap grid,
//   the halfspace mask of the intersection (mv_graph.get_mask_from_halfspace), and the float64 sums of normalized_cross_correlation
// with ONE gather-and-reduce pass: per grid voxel the mask, one linear sample of the fixed tile and K of the moving tile, and six
// running moments per candidate.  No volume is written; the fixed tile is read once for all K candidates.
//
// Sampling is the code of mvs_resample (mvs_sample_dev.h: coordinates in double with scipy's operation order, float32 taps), so the
// samples have the bits mvs_resample would have written.  The reduction is deterministic: shifted sums per thread, then Chan's
// pairwise update in a fixed tree (lanes by shuffle, waves through LDS, one record per workgroup, a second launch for the records);
// no floating-point atomics, no completion counters, and a grid that depends on the voxel count only.
#include "mvs_internal.h"
#include "mvs_fuse_dev.h"
#include "mvs_pair_voxel_dev.h"

#include <algorithm>
#include <cmath>
#include <cstring>

static_assert(kPairBlockThreads == MVS_PAIR_BLOCK_VOXELS && kPairMaxBlocks == MVS_PAIR_MAX_BLOCKS, "constants of include/mvs_hip.h");
static_assert(sizeof(PairMoments) == MVS_PAIR_MOMENTS_LEN * sizeof(double), "a record is one row of the result");

namespace {

constexpr int kWaves = kPairBlockThreads / 64;

struct PairArgs {
    DevView fixed, moving;                          // of `moving` only data, shape and strides are used
    double cm[MVS_PAIR_MAX_CANDIDATES][9];          // grid index -> moving pixel, per candidate
    double co[MVS_PAIR_MAX_CANDIDATES][3];
    double hs[MVS_PAIR_MAX_HALFSPACES][4];          // a_z, a_y, a_x, b in grid index coordinates
    int n_cand, n_hs;
    int gz, gy, gx;
    PairMoments* records;                           // [workgroup][candidate]
};
static_assert(sizeof(PairArgs) <= 4096, "kernel arguments");

template <typename T, int KMAX>
__global__ __launch_bounds__(kPairBlockThreads) void pair_moments_kernel(PairArgs P) {
    PairSums acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = PairSums{0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

    const long long n = (long long)P.gz * P.gy * P.gx;
    for (long long i = (long long)blockIdx.x * kPairBlockThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kPairBlockThreads) {
        const int x = (int)(i % P.gx);
        const long long t = i / P.gx;
        const int y = (int)(t % P.gy);
        const int z = (int)(t / P.gy);
        const double pz = (double)z, py = (double)y, px = (double)x;
        if (!pair_mask_holds(P.hs, P.n_hs, pz, py, px)) continue;
        double fz, fy, fx;
        pair_grid_to_pixel(P.fixed.m, P.fixed.off, pz, py, px, fz, fy, fx);
        float f;
        if (!pair_sample_finite<T>(P.fixed, fz, fy, fx, &f)) continue;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k >= P.n_cand) continue;
            double cz, cy, cx;
            pair_grid_to_pixel(P.cm[k], P.co[k], pz, py, px, cz, cy, cx);
            float v;
            if (pair_sample_finite<T>(P.moving, cz, cy, cx, &v)) pair_sums_add(acc[k], f, v);
        }
    }

    __shared__ PairMoments lds[kWaves][KMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const PairMoments r = wave_merge(pair_sums_to_moments(acc[k]));
        if (lane == 0) lds[wave][k] = r;
    }
    __syncthreads();
    if ((int)threadIdx.x < P.n_cand && (int)threadIdx.x < KMAX) {
        PairMoments r = lds[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) r = pair_moments_merge(r, lds[w][threadIdx.x]);
        P.records[(long long)blockIdx.x * P.n_cand + threadIdx.x] = r;
    }
}

// One wave per candidate: lane l folds its run of ceil(n_records / 64) consecutive records in index order, then the lanes merge
// in the tree of wave_merge -- every record's place in the tree is a function of (n_records, its index) only.
__global__ __launch_bounds__(64) void pair_moments_fold_kernel(const PairMoments* records, int n_records, int n_cand, PairMoments* out) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const int run = (n_records + 63) / 64;
    const int lo = lane * run, hi = min(lo + run, n_records);
    PairMoments r = pair_moments_empty();
    for (int i = lo; i < hi; ++i) r = pair_moments_merge(r, records[(long long)i * n_cand + k]);
    r = wave_merge(r);
    if (lane == 0) out[k] = r;
}

template <typename T>
void launch_pair_moments(const PairArgs& P, int nblocks, hipStream_t s) {
#define MVS_PM(K) hipLaunchKernelGGL((pair_moments_kernel<T, K>), dim3(nblocks), dim3(kPairBlockThreads), 0, s, P)
    if (P.n_cand <= 1) MVS_PM(1);
    else if (P.n_cand <= 2) MVS_PM(2);
    else if (P.n_cand <= 4) MVS_PM(4);
    else MVS_PM(8);
#undef MVS_PM
}

}  // namespace

extern "C" int mvs_pair_moments(int device, const mvs_view_t* fixed, const mvs_view_t* moving, int32_t n_candidates,
                                const double* cand_matrix, const double* cand_offset, int32_t ndim, const int64_t grid_shape[3],
                                const double* halfspaces, int32_t n_halfspaces, double* out) {
    MvsContext* c0 = mvs_ctx(device);
    if (!fixed || !moving || !cand_matrix || !cand_offset || !grid_shape || !out)
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_pair_moments: NULL argument");
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_pair_moments: ndim must be 2 or 3");
    if (n_candidates < 1 || n_candidates > MVS_PAIR_MAX_CANDIDATES)
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_pair_moments: n_candidates must be 1..%d", MVS_PAIR_MAX_CANDIDATES);
    if (n_halfspaces < 0 || n_halfspaces > MVS_PAIR_MAX_HALFSPACES || (n_halfspaces > 0 && !halfspaces))
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_pair_moments: n_halfspaces must be 0..%d (with their equations)", MVS_PAIR_MAX_HALFSPACES);
    for (int k = 0; k < 3; ++k)
        if (grid_shape[k] < 1 || grid_shape[k] > 0x7fffffffLL || (k < 3 - ndim && grid_shape[k] != 1))
            return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_pair_moments: grid_shape must be positive (and 1 along z in 2D)");
    const mvs_view_t* both[2] = {fixed, moving};
    for (const mvs_view_t* v : both) {
        const int rc = mvs_check_tile_view(c0, "mvs_pair_moments", v, ndim);
        if (rc) return rc;
    }
    if (fixed->dtype != moving->dtype)
        return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_pair_moments: the views must share one dtype (%d and %d given)", fixed->dtype, moving->dtype);
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    PairArgs P;
    DevView* dv[2] = {&P.fixed, &P.moving};
    rc = mvs_stage_tile_views(c, both, 2, ndim, nullptr, dv);
    if (rc) return rc;
    memcpy(P.cm, cand_matrix, sizeof(double) * 9 * n_candidates);
    memcpy(P.co, cand_offset, sizeof(double) * 3 * n_candidates);
    if (n_halfspaces) memcpy(P.hs, halfspaces, sizeof(double) * 4 * n_halfspaces);
    P.n_cand = n_candidates;
    P.n_hs = n_halfspaces;
    P.gz = (int)grid_shape[0]; P.gy = (int)grid_shape[1]; P.gx = (int)grid_shape[2];

    const long long n = (long long)grid_shape[0] * grid_shape[1] * grid_shape[2];
    const int nblocks = (int)std::min<long long>((n + kPairBlockThreads - 1) / kPairBlockThreads, kPairMaxBlocks);
    P.records = (PairMoments*)mvs_scratch(c, 1, sizeof(PairMoments) * (size_t)nblocks * n_candidates);
    if (!P.records) return mvs_alloc_failed(c);
    void *mb_host = nullptr, *mb_dev = nullptr;
    rc = mvs_mailbox(c, sizeof(PairMoments) * (size_t)n_candidates, &mb_host, &mb_dev);
    if (rc) return rc;

    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    mvs_dispatch_dtype(fixed->dtype, [&](auto tag) { launch_pair_moments<decltype(tag)>(P, nblocks, c->stream); });
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(pair_moments_fold_kernel, dim3(n_candidates), dim3(64), 0, c->stream, P.records, nblocks, n_candidates, (PairMoments*)mb_dev);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(out, mb_host, sizeof(PairMoments) * (size_t)n_candidates);
    return MVS_OK;
}
