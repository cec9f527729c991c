// mvs_marker.hip -- the device side of marker-based (bead) registration on gfx950: mvs_knn, mvs_marker_descriptors and
// mvs_marker_score (include/mvs_hip.h).
//
// The reference's registration_marker_based (src/multiview_stitcher/registration.py:595-1379) spends its time in three places:
//   * cKDTree queries -- k = 2 for the neighbour scale (:619), k = required + 2 for the descriptor neighbourhoods (:662-664),
//     k = descriptors per point + 1 in DESCRIPTOR space (:743-746), k = 1 per ICP iteration (:1095-1097).  In a space of 6 to 15
//     dimensions a k-d tree hardly prunes; here all of them are one brute-force kernel, mvs_knn.
//   * the Python loops that build one sorted distance vector per (point, neighbour subset) (:666-690): mvs_marker_descriptors.
//   * the RANSAC loop that scores one hypothesis at a time against all candidates (:947-981): mvs_marker_score scores all of them.
// Everything else (thresholds, the ratio test, sampling, the model fits, ranking, ICP bookkeeping) is host work on a few hundred
// numbers and stays in Python (_marker_reg.py).
//
// All coordinate and distance arithmetic is float64, a distance is sqrt(sum_d (a_d - b_d)^2) of the DIFFERENCES, summed in axis
// order without contraction: bead coordinates are world coordinates (1e6 with sub-pixel differences), where the expanded form
// |a|^2 + |b|^2 - 2ab cancels.
#include "mvs_internal.h"
#include "mvs_fold_dev.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int KNN_BLOCK = 256;    // queries per workgroup: one per thread
constexpr int KNN_TILE = 256;     // reference rows staged per step: MVS_KNN_MAX_DIM * 256 * 8 B = 30 KiB of LDS, 5 workgroups per CU

// The running top-k of one query: ascending distances in registers (every index below is a compile-time constant once the
// loops are unrolled; a dynamically indexed array would live in scratch).  A candidate goes in front of the first entry it is
// strictly smaller than: references arrive by ascending index, so equal distances keep the lower index first.
template <int KT>
__device__ __forceinline__ void topk_insert(double (&bd)[KT], int32_t (&bi)[KT], double d, int32_t i) {
#pragma unroll
    for (int j = KT - 1; j >= 0; --j) {
        if (j > 0 && d < bd[j - 1]) {
            bd[j] = bd[j - 1];
            bi[j] = bi[j - 1];
        } else if (d < bd[j]) {
            bd[j] = d;
            bi[j] = i;
        }
    }
}

// DIM > 0: the dimension as a template parameter; DIM == 0: `dim` at run time (1 .. MVS_KNN_MAX_DIM), unrolled to the maximum with
// uniform guards so that the query's coordinates stay in registers.  grid = ceil(n_query / 256).
// The tile is component-major (tile[c * KNN_TILE + r]): in the inner loop all lanes read ONE address per component (a broadcast).
// Threads past n_query stay in the loop for its barriers; rows past n_ref are not visited (the bound is uniform).
template <int DIM, int KT>
__global__ __launch_bounds__(KNN_BLOCK) void knn_kernel(const double* __restrict__ ref, long long n_ref, const double* __restrict__ query,
                                                        long long n_query, int dim, int k, int32_t* __restrict__ idx_out,
                                                        double* __restrict__ dist_out) {
    constexpr int QD = DIM ? DIM : MVS_KNN_MAX_DIM;
    __shared__ double tile[QD * KNN_TILE];
    const int nd = DIM ? DIM : dim;
    const long long q = (long long)blockIdx.x * KNN_BLOCK + threadIdx.x;
    const bool live = q < n_query;
    double qc[QD];
#pragma unroll
    for (int c = 0; c < QD; ++c) qc[c] = (live && c < nd) ? query[q * nd + c] : 0.0;
    double bd[KT];
    int32_t bi[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) {
        bd[j] = INFINITY;
        bi[j] = -1;
    }
    // a squared sum above `lim` cannot enter the list: sqrt(s) >= bd[KT - 1] then (the factor covers the roundings of the
    // product and of the root; the floor covers a last entry so small that its square underflows).  It spares the root of
    // nearly every pair and decides nothing: what passes is compared as a distance.
    double lim = INFINITY;
    for (long long t0 = 0; t0 < n_ref; t0 += KNN_TILE) {
        const int rows = (int)std::min<long long>(KNN_TILE, n_ref - t0);
        __syncthreads();
        for (int e = threadIdx.x; e < rows * nd; e += KNN_BLOCK) {
            const int r = e / nd, c = e - r * nd;
            tile[c * KNN_TILE + r] = ref[t0 * nd + e];
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < QD; ++c) {
                if (DIM || c < nd) {
                    const double df = qc[c] - tile[c * KNN_TILE + r];
                    s += df * df;
                }
            }
            if (s <= lim) {
                const double d = sqrt(s);
                if (d < bd[KT - 1]) {
                    topk_insert<KT>(bd, bi, d, (int32_t)(t0 + r));
                    lim = fmax(bd[KT - 1] * bd[KT - 1] * (1.0 + 0x1p-50), 1e-279);
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < KT; ++j) {
        if (j < k) {
            idx_out[q * k + j] = bi[j];
            dist_out[q * k + j] = bd[j];
        }
    }
}

template <int DIM>
void launch_knn_k(int kt, dim3 g, hipStream_t st, const double* ref, long long n_ref, const double* query, long long n_query, int dim, int k,
                  int32_t* idx, double* dist) {
    const dim3 b(KNN_BLOCK);
    switch (kt) {
        case 1: hipLaunchKernelGGL((knn_kernel<DIM, 1>), g, b, 0, st, ref, n_ref, query, n_query, dim, k, idx, dist); break;
        case 2: hipLaunchKernelGGL((knn_kernel<DIM, 2>), g, b, 0, st, ref, n_ref, query, n_query, dim, k, idx, dist); break;
        case 8: hipLaunchKernelGGL((knn_kernel<DIM, 8>), g, b, 0, st, ref, n_ref, query, n_query, dim, k, idx, dist); break;
        default: hipLaunchKernelGGL((knn_kernel<DIM, 16>), g, b, 0, st, ref, n_ref, query, n_query, dim, k, idx, dist); break;
    }
}

// ---- descriptors ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int binom(int n, int k) {      // n <= 14: no overflow
    if (k < 0 || k > n) return 0;
    int r = 1;
    for (int j = 1; j <= k; ++j) r = r * (n - k + j) / j;
    return r;
}

__device__ __forceinline__ void cmpxchg(double& a, double& b) {
    const double lo = fmin(a, b), hi = fmax(a, b);
    a = lo;
    b = hi;
}

// One thread per (point, subset): subset s of the point's `required` neighbours in itertools.combinations order (lexicographic in
// the positions of the neighbour list), the NN + 1 points gathered (the point itself first), their pairwise distances in
// itertools.combinations(range(NN + 1), 2) order, sorted ascending by an odd-even transposition network (a fixed sequence of
// compare-exchanges).  A neighbour index outside [0, n) (the -1 of a short kNN row) gives a row of NaN.
template <int NN>
__global__ __launch_bounds__(256) void descriptor_kernel(const double* __restrict__ pts, long long n, int ndim, const int32_t* __restrict__ nbr,
                                                         int required, int n_sub, double* __restrict__ out) {
    constexpr int M = NN + 1, L = M * (M - 1) / 2;
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= n * n_sub) return;
    const long long p = row / n_sub;
    int rem = (int)(row - p * n_sub);
    int sel[NN];
    int start = 0;
#pragma unroll
    for (int j = 0; j < NN; ++j) {
        int c = start;
        for (; c < required; ++c) {
            const int cnt = binom(required - c - 1, NN - j - 1);
            if (rem < cnt) break;
            rem -= cnt;
        }
        sel[j] = c;
        start = c + 1;
    }
    double P[M][3];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        long long i = p;
        if (j > 0) {
            const int s = sel[j - 1];
            i = s < required ? (long long)nbr[p * required + s] : -1;
        }
        if (i < 0 || i >= n) ok = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) P[j][a] = (ok && a < ndim) ? pts[i * ndim + a] : 0.0;
    }
    double v[L];
    int e = 0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
#pragma unroll
        for (int j = i + 1; j < M; ++j) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {      // (axes past ndim add +0.0: nothing changes)
                const double df = P[i][a] - P[j][a];
                s += df * df;
            }
            v[e++] = sqrt(s);
        }
    }
#pragma unroll
    for (int pass = 0; pass < L; ++pass) {
#pragma unroll
        for (int i = pass & 1; i + 1 < L; i += 2) cmpxchg(v[i], v[i + 1]);
    }
#pragma unroll
    for (int i = 0; i < L; ++i) out[row * L + i] = ok ? v[i] : NAN;
}

// ---- hypothesis scoring --------------------------------------------------------------------------------------------------------
// One wave per hypothesis (4 per workgroup).  Lane l takes correspondences l, l + 64, ... in that order, then the lanes are folded
// by shuffles with offsets 32, 16, ..., 1: a fixed tree, no floating-point atomics, so equal inputs give equal bits.
// residual = || A f + t - m ||, rows as ((a0 f0 + a1 f1) + a2 f2) + t; an inlier has residual <= max_error.
__global__ __launch_bounds__(256) void score_kernel(const double* __restrict__ aff, int n_hyp, const double* __restrict__ fx,
                                                    const double* __restrict__ mv, long long n_corr, int ndim, double max_error,
                                                    int32_t* __restrict__ count_out, double* __restrict__ sum_out) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (h >= n_hyp) return;                        // (whole waves leave: the shuffles below see complete waves)
    const int w = ndim + 1;
    const double* A = aff + (long long)h * w * w;
    double a[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) a[r][c] = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (r < ndim && c < ndim) a[r][c] = A[r * w + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        if (r < ndim) a[r][3] = A[r * w + ndim];
    int cnt = 0;
    double sum = 0.0;
    for (long long i = lane; i < n_corr; i += 64) {
        double f[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (c < ndim) {
                f[c] = fx[i * ndim + c];
                m[c] = mv[i * ndim + c];
            }
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (r < ndim) {
                double y = a[r][0] * f[0];
                if (ndim > 1) y += a[r][1] * f[1];
                if (ndim > 2) y += a[r][2] * f[2];
                const double df = (y + a[r][3]) - m[r];
                s += df * df;
            }
        const double res = sqrt(s);
        if (res <= max_error) {
            ++cnt;
            sum += res;
        }
    }
    cnt = mvs_fold::wave_fold(mvs_fold::Sums<int>{{cnt}}).v[0];
    sum = mvs_fold::wave_fold(mvs_fold::Sums<double>{{sum}}).v[0];
    if (lane == 0) {
        count_out[h] = cnt;
        sum_out[h] = sum;
    }
}

bool bad_mem(int32_t mem) { return mem != MVS_MEM_HOST && mem != MVS_MEM_DEVICE; }

constexpr int64_t kMaxRows = (int64_t)1 << 30;     // rows of a point set: indices are int32, a launch has fewer than 2^24 workgroups

}  // namespace

extern "C" int mvs_knn(int device, const double* ref, int32_t ref_mem, int64_t n_ref, const double* query, int32_t query_mem,
                       int64_t n_query, int32_t dim, int32_t k, int32_t* idx_out, double* dist_out) {
    MvsContext* c0 = mvs_ctx(device);
    if (!ref || !query || !idx_out || !dist_out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_knn: NULL argument");
    if (bad_mem(ref_mem) || bad_mem(query_mem)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_knn: bad mem");
    if (dim < 1 || k < 1 || n_ref < 1 || n_query < 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_knn: dim, k, n_ref and n_query must be positive");
    if (dim > MVS_KNN_MAX_DIM) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_knn: dim %d above MVS_KNN_MAX_DIM (%d)", (int)dim, MVS_KNN_MAX_DIM);
    if (k > MVS_KNN_MAX_K) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_knn: k %d above MVS_KNN_MAX_K (%d)", (int)k, MVS_KNN_MAX_K);
    if (n_ref > kMaxRows || n_query > kMaxRows) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_knn: more than 2^30 rows");
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    const size_t ref_bytes = (size_t)n_ref * dim * sizeof(double), query_bytes = (size_t)n_query * dim * sizeof(double);
    const bool shared = ref == query && ref_mem == query_mem && n_ref == n_query;      // a set against itself: staged once
    const size_t ref_stage = ref_mem == MVS_MEM_HOST ? align_up(ref_bytes) : 0;
    const size_t query_stage = (query_mem == MVS_MEM_HOST && !shared) ? align_up(query_bytes) : 0;
    const size_t idx_bytes = (size_t)n_query * k * sizeof(int32_t), dist_bytes = (size_t)n_query * k * sizeof(double);
    MvsWorkArea wa(c);
    rc = wa.alloc(ref_stage + query_stage + align_up(idx_bytes) + align_up(dist_bytes));
    if (rc) return rc;
    char* p = (char*)wa.ptr;
    const double* dref = ref;
    const double* dquery = query;
    if (ref_mem == MVS_MEM_HOST) {
        MVS_HIP_TRY(c, hipMemcpyAsync(p, ref, ref_bytes, hipMemcpyHostToDevice, c->stream));
        dref = (const double*)p;
    }
    if (shared) dquery = dref;
    else if (query_mem == MVS_MEM_HOST) {
        MVS_HIP_TRY(c, hipMemcpyAsync(p + ref_stage, query, query_bytes, hipMemcpyHostToDevice, c->stream));
        dquery = (const double*)(p + ref_stage);
    }
    int32_t* didx = (int32_t*)(p + ref_stage + query_stage);
    double* ddist = (double*)(p + ref_stage + query_stage + align_up(idx_bytes));

    const int kt = k <= 1 ? 1 : (k <= 2 ? 2 : (k <= 8 ? 8 : 16));
    const dim3 g((unsigned)((n_query + KNN_BLOCK - 1) / KNN_BLOCK));
    switch (dim) {
        case 1: launch_knn_k<1>(kt, g, c->stream, dref, n_ref, dquery, n_query, dim, k, didx, ddist); break;
        case 2: launch_knn_k<2>(kt, g, c->stream, dref, n_ref, dquery, n_query, dim, k, didx, ddist); break;
        case 3: launch_knn_k<3>(kt, g, c->stream, dref, n_ref, dquery, n_query, dim, k, didx, ddist); break;
        case 6: launch_knn_k<6>(kt, g, c->stream, dref, n_ref, dquery, n_query, dim, k, didx, ddist); break;
        case 10: launch_knn_k<10>(kt, g, c->stream, dref, n_ref, dquery, n_query, dim, k, didx, ddist); break;
        default: launch_knn_k<0>(kt, g, c->stream, dref, n_ref, dquery, n_query, dim, k, didx, ddist); break;
    }
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipMemcpyAsync(idx_out, didx, idx_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipMemcpyAsync(dist_out, ddist, dist_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return wa.release();
}

extern "C" int mvs_marker_descriptors(int device, const double* points, int32_t points_mem, int64_t n_points, int32_t ndim,
                                      const int32_t* neighbors, int32_t num_neighbors, int32_t redundancy, double* out, int32_t out_mem) {
    MvsContext* c0 = mvs_ctx(device);
    if (!points || !neighbors || !out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_marker_descriptors: NULL argument");
    if (bad_mem(points_mem) || bad_mem(out_mem)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_marker_descriptors: bad mem");
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_marker_descriptors: ndim must be 2 or 3");
    if (num_neighbors < 1 || redundancy < 0 || n_points < 1)
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_marker_descriptors: num_neighbors and n_points must be positive, redundancy non-negative");
    if (num_neighbors > MVS_MARKER_MAX_NEIGHBORS)
        return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_marker_descriptors: num_neighbors %d above MVS_MARKER_MAX_NEIGHBORS (%d)", (int)num_neighbors,
                        MVS_MARKER_MAX_NEIGHBORS);
    if (redundancy > MVS_KNN_MAX_K || num_neighbors + redundancy > MVS_KNN_MAX_K - 2)
        return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_marker_descriptors: num_neighbors + redundancy above %d", MVS_KNN_MAX_K - 2);
    const int required = num_neighbors + redundancy;
    long long n_sub = 1;
    for (int j = 1; j <= num_neighbors; ++j) n_sub = n_sub * (required - num_neighbors + j) / j;      // C(required, num_neighbors) <= 2002
    if (n_points > kMaxRows || n_points * n_sub > kMaxRows) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_marker_descriptors: more than 2^30 rows");
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    const int len = (num_neighbors + 1) * num_neighbors / 2;
    const long long rows = n_points * n_sub;
    const size_t pts_bytes = (size_t)n_points * ndim * sizeof(double), nbr_bytes = (size_t)n_points * required * sizeof(int32_t);
    const size_t out_bytes = (size_t)rows * len * sizeof(double);
    const size_t pts_stage = points_mem == MVS_MEM_HOST ? align_up(pts_bytes) : 0;
    const size_t out_stage = out_mem == MVS_MEM_HOST ? align_up(out_bytes) : 0;
    MvsWorkArea wa(c);
    rc = wa.alloc(pts_stage + align_up(nbr_bytes) + out_stage);
    if (rc) return rc;
    char* p = (char*)wa.ptr;
    const double* dpts = points;
    if (points_mem == MVS_MEM_HOST) {
        MVS_HIP_TRY(c, hipMemcpyAsync(p, points, pts_bytes, hipMemcpyHostToDevice, c->stream));
        dpts = (const double*)p;
    }
    int32_t* dnbr = (int32_t*)(p + pts_stage);
    MVS_HIP_TRY(c, hipMemcpyAsync(dnbr, neighbors, nbr_bytes, hipMemcpyHostToDevice, c->stream));
    double* dout = out_mem == MVS_MEM_HOST ? (double*)(p + pts_stage + align_up(nbr_bytes)) : out;
    const dim3 g((unsigned)((rows + 255) / 256)), b(256);
    switch (num_neighbors) {
        case 1: hipLaunchKernelGGL((descriptor_kernel<1>), g, b, 0, c->stream, dpts, (long long)n_points, (int)ndim, dnbr, required, (int)n_sub, dout); break;
        case 2: hipLaunchKernelGGL((descriptor_kernel<2>), g, b, 0, c->stream, dpts, (long long)n_points, (int)ndim, dnbr, required, (int)n_sub, dout); break;
        case 3: hipLaunchKernelGGL((descriptor_kernel<3>), g, b, 0, c->stream, dpts, (long long)n_points, (int)ndim, dnbr, required, (int)n_sub, dout); break;
        case 4: hipLaunchKernelGGL((descriptor_kernel<4>), g, b, 0, c->stream, dpts, (long long)n_points, (int)ndim, dnbr, required, (int)n_sub, dout); break;
        default: hipLaunchKernelGGL((descriptor_kernel<5>), g, b, 0, c->stream, dpts, (long long)n_points, (int)ndim, dnbr, required, (int)n_sub, dout); break;
    }
    MVS_HIP_TRY(c, hipGetLastError());
    if (out_mem == MVS_MEM_HOST) MVS_HIP_TRY(c, hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the staged neighbour table goes back to the pool: waited for either way)
    return wa.release();
}

extern "C" int mvs_marker_score(int device, const double* affines, int32_t n_hypotheses, const double* fixed, const double* moving,
                                int64_t n_corr, int32_t ndim, double max_error, int32_t* count_out, double* sum_out) {
    MvsContext* c0 = mvs_ctx(device);
    if (!affines || !fixed || !moving || !count_out || !sum_out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_marker_score: NULL argument");
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_marker_score: ndim must be 2 or 3");
    if (n_hypotheses < 1 || n_corr < 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_marker_score: n_hypotheses and n_corr must be positive");
    if (n_hypotheses > (1 << 24) || n_corr > kMaxRows) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_marker_score: more than 2^24 hypotheses or 2^30 correspondences");
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    const int w = ndim + 1;
    const size_t aff_bytes = (size_t)n_hypotheses * w * w * sizeof(double), pts_bytes = (size_t)n_corr * ndim * sizeof(double);
    const size_t cnt_bytes = (size_t)n_hypotheses * sizeof(int32_t), sum_bytes = (size_t)n_hypotheses * sizeof(double);
    MvsWorkArea wa(c);
    rc = wa.alloc(align_up(aff_bytes) + 2 * align_up(pts_bytes) + align_up(cnt_bytes) + align_up(sum_bytes));
    if (rc) return rc;
    char* p = (char*)wa.ptr;
    double* daff = (double*)p;
    double* dfx = (double*)(p + align_up(aff_bytes));
    double* dmv = (double*)(p + align_up(aff_bytes) + align_up(pts_bytes));
    int32_t* dcnt = (int32_t*)(p + align_up(aff_bytes) + 2 * align_up(pts_bytes));
    double* dsum = (double*)(p + align_up(aff_bytes) + 2 * align_up(pts_bytes) + align_up(cnt_bytes));
    MVS_HIP_TRY(c, hipMemcpyAsync(daff, affines, aff_bytes, hipMemcpyHostToDevice, c->stream));
    MVS_HIP_TRY(c, hipMemcpyAsync(dfx, fixed, pts_bytes, hipMemcpyHostToDevice, c->stream));
    MVS_HIP_TRY(c, hipMemcpyAsync(dmv, moving, pts_bytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)((n_hypotheses + 3) / 4)), dim3(256), 0, c->stream, (const double*)daff, (int)n_hypotheses,
                       (const double*)dfx, (const double*)dmv, (long long)n_corr, (int)ndim, max_error, dcnt, dsum);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipMemcpyAsync(count_out, dcnt, cnt_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipMemcpyAsync(sum_out, dsum, sum_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return wa.release();
}
