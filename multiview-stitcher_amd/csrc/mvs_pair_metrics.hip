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
#include "mvs_pair_frame.h"

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
        const PairMoments r = mvs_fold::wave_fold(pair_sums_to_moments(acc[k]));
        if (lane == 0) lds[wave][k] = r;
    }
    __syncthreads();
    if ((int)threadIdx.x < P.n_cand && (int)threadIdx.x < KMAX) {
        PairMoments r = lds[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) r = pair_moments_merge(r, lds[w][threadIdx.x]);
        P.records[(long long)blockIdx.x * P.n_cand + threadIdx.x] = r;
    }
}

// One wave per candidate folds the candidate's record of every workgroup (pair_moments_fold, mvs_pair_voxel_dev.h).
__global__ __launch_bounds__(64) void pair_moments_fold_kernel(const PairMoments* records, int n_records, int n_cand, PairMoments* out) {
    const PairMoments r = pair_moments_fold(records + blockIdx.x, n_cand, n_records, threadIdx.x);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
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
    const char* what = "mvs_pair_moments";
    MvsContext* c0 = mvs_ctx(device);
    if (!fixed || !moving || !cand_matrix || !cand_offset || !grid_shape || !out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", what);      // (here too: n_candidates comes before the halfspaces)
    if (n_candidates < 1 || n_candidates > MVS_PAIR_MAX_CANDIDATES)
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: n_candidates must be 1..%d", what, MVS_PAIR_MAX_CANDIDATES);
    int rc = mvs_pair_check_counts(c0, what, ndim, halfspaces, n_halfspaces);
    if (rc) return rc;
    for (int k = 0; k < 3; ++k)
        if (grid_shape[k] < 1 || grid_shape[k] > 0x7fffffffLL || (k < 3 - ndim && grid_shape[k] != 1))
            return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: grid_shape must be positive (and 1 along z in 2D)", what);
    rc = mvs_pair_check_views(c0, what, fixed, moving, ndim);
    if (rc) return rc;

    PairArgs P;
    memcpy(P.cm, cand_matrix, sizeof(double) * 9 * n_candidates);
    memcpy(P.co, cand_offset, sizeof(double) * 3 * n_candidates);
    P.n_cand = n_candidates;
    P.gz = (int)grid_shape[0]; P.gy = (int)grid_shape[1]; P.gx = (int)grid_shape[2];
    const long long n = (long long)grid_shape[0] * grid_shape[1] * grid_shape[2];
    const int nblocks = (int)std::min<long long>((n + kPairBlockThreads - 1) / kPairBlockThreads, kPairMaxBlocks);
    const size_t out_bytes = sizeof(PairMoments) * (size_t)n_candidates;
    auto prepare = [&](MvsContext* c, void** host, void** dev) -> int {
        P.records = (PairMoments*)mvs_scratch(c, 1, sizeof(PairMoments) * (size_t)nblocks * n_candidates);
        if (!P.records) return mvs_alloc_failed(c);
        return mvs_mailbox(c, out_bytes, host, dev);
    };
    return mvs_pair_frame(device, fixed, moving, ndim, halfspaces, n_halfspaces, P, out, out_bytes, prepare,
        [&](auto tag, hipStream_t s) { launch_pair_moments<decltype(tag)>(P, nblocks, s); },
        [&](hipStream_t s, void* dev) { hipLaunchKernelGGL(pair_moments_fold_kernel, dim3(n_candidates), dim3(64), 0, s, P.records, nblocks, n_candidates, (PairMoments*)dev); });
}
