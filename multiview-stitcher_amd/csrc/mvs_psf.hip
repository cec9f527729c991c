// mvs_psf.hip -- PSF extraction from beads for the multi-view deconvolution (gfx950): mvs_psf_extract (include/mvs_hip.h).
//
// The reference has no such function; its model (BigStitcher / multiview-reconstruction) measures every view's PSF from the beads
// that drive the registration.  Per bead a window of output-grid voxels around the bead's centre is gathered from the view with the
// library's linear sampler, its background (the mean of the window's shell) subtracted, the centre refined by the centroid of what
// is left, and the windows, each scaled to unit sum, are averaged.  Three kernels, all deterministic:
//   A  psf_window_kernel      one workgroup per bead: gather into the bead's scratch row, shell mean, energy and first moments,
//                             centre update, gather again; the last pass leaves the bead's normalised window u_b in its row
//   B  psf_accumulate_kernel  one thread per window offset: a float64 sum over the used beads in ascending index order
//   C  psf_ncc_kernel         one workgroup per used bead: the five sums of the Pearson correlation of u_b with the PSF
// No floating-point atomics: a thread sums its strided samples in order, lanes fold by shuffles, the four waves through LDS in wave
// order.  Beads pass through in batches sized to a scratch budget; B carries its accumulator from batch to batch, so the sum visits
// the beads in the same order whatever the batch size, and equal inputs give equal bits.
#include "mvs_internal.h"
#include "mvs_fold_dev.h"
#include "mvs_fuse_dev.h"
#include "mvs_sample_dev.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr size_t kRowBudget = (size_t)256 << 20;      // bytes of per-bead rows of one batch when option "psf_batch" is 0

struct PsfArgs {
    DevView view;                // data, shape and strides are used
    double m[9];                 // window offset (output-grid voxels) -> view pixels
    int r[3], w[3];              // radius and extent 2 r + 1 per axis (z, y, x; r[0] = 0 in 2D)
    int n_window, n_shell;
    int first_axis;              // 3 - ndim: the axes from here on span the window
    int refine;
    int b0;                      // index of the batch's first bead
    const double* centers_in;    // [bead][3]
    double* centers_out;
    int32_t* status;
    float* stats;                // [bead][3]: background, energy sum, ncc
    float* rows;                 // [bead - b0][offset]
};

// Sums of K doubles over the workgroup, the same value in every thread (mvs_fold_dev.h).  Every thread of the workgroup calls it.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K]) {
    mvs_fold::Sums<double, K> s;
#pragma unroll
    for (int k = 0; k < K; ++k) s.v[k] = v[k];
    s = mvs_fold::block_fold_all<kWaves>(s);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = s.v[k];
}

// window offset of flat index i (x fastest)
__device__ __forceinline__ void window_offset(const PsfArgs& P, int i, int& oz, int& oy, int& ox) {
    ox = i % P.w[2] - P.r[2];
    const int t = i / P.w[2];
    oy = t % P.w[1] - P.r[1];
    oz = t / P.w[1] - P.r[0];
}

// Stage A.  grid = beads of the batch.  Loop exits are taken by the whole workgroup (they depend on block sums only).
template <typename T>
__global__ __launch_bounds__(kThreads) void psf_window_kernel(PsfArgs P) {
    const long long b = (long long)P.b0 + blockIdx.x;
    float* row = P.rows + (long long)blockIdx.x * P.n_window;
    double cz = P.centers_in[3 * b], cy = P.centers_in[3 * b + 1], cx = P.centers_in[3 * b + 2];
    int status = 0;
    double bg = NAN, esum = NAN;
    for (int it = 0;; ++it) {
        // gather: the samples go to the bead's row; shell sum; number of samples that are out of bounds or NaN
        double a[2] = {0.0, 0.0};
        for (int i = threadIdx.x; i < P.n_window; i += kThreads) {
            int oz, oy, ox;
            window_offset(P, i, oz, oy, ox);
            const double dz = (double)oz, dy = (double)oy, dx = (double)ox;
            const double pz = ((P.m[0] * dz + P.m[1] * dy) + P.m[2] * dx) + cz;
            const double py = ((P.m[3] * dz + P.m[4] * dy) + P.m[5] * dx) + cy;
            const double px = ((P.m[6] * dz + P.m[7] * dy) + P.m[8] * dx) + cx;
            // (a NaN coordinate fails no comparison of view_in_bounds: it is refused here, before any address is formed)
            const bool in = pz == pz && py == py && px == px && view_in_bounds(P.view, pz, py, px);
            float s = 0.f;
            if (in) s = sample_view<T, 1>(P.view, pz, py, px);
            if (!in || s != s) a[1] += 1.0;
            row[i] = s;
            const bool shell = (P.first_axis == 0 && abs(oz) == P.r[0]) || abs(oy) == P.r[1] || abs(ox) == P.r[2];
            if (shell) a[0] += (double)s;
        }
        block_sum<2>(a);
        if (a[1] > 0.0) {
            status = 1;
            bg = esum = NAN;
            break;
        }
        bg = a[0] / (double)P.n_shell;
        // energy and first moments (each thread reads back the samples it wrote itself)
        double mo[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = threadIdx.x; i < P.n_window; i += kThreads) {
            int oz, oy, ox;
            window_offset(P, i, oz, oy, ox);
            const double e = fmax((double)row[i] - bg, 0.0);
            mo[0] += e;
            mo[1] += (double)oz * e;
            mo[2] += (double)oy * e;
            mo[3] += (double)ox * e;
        }
        block_sum<4>(mo);
        esum = mo[0];
        if (!(esum > 0.0 && esum < INFINITY)) {
            status = 2;
            break;
        }
        if (it >= P.refine) {
            for (int i = threadIdx.x; i < P.n_window; i += kThreads) row[i] = (float)(fmax((double)row[i] - bg, 0.0) / esum);
            break;
        }
        const double tz = mo[1] / esum, ty = mo[2] / esum, tx = mo[3] / esum;
        cz += (P.m[0] * tz + P.m[1] * ty) + P.m[2] * tx;
        cy += (P.m[3] * tz + P.m[4] * ty) + P.m[5] * tx;
        cx += (P.m[6] * tz + P.m[7] * ty) + P.m[8] * tx;
    }
    if (threadIdx.x == 0) {
        P.centers_out[3 * b] = cz;
        P.centers_out[3 * b + 1] = cy;
        P.centers_out[3 * b + 2] = cx;
        P.status[b] = status;
        P.stats[3 * b] = (float)bg;
        P.stats[3 * b + 1] = (float)esum;
        P.stats[3 * b + 2] = NAN;
    }
}

// Stage B.  grid = ceil(n_window / 256).  acc[i] += the rows of the batch's used beads at offset i, in bead order.
__global__ __launch_bounds__(kThreads) void psf_accumulate_kernel(const float* __restrict__ rows, const int32_t* __restrict__ status, int b0,
                                                                  int n_batch, int n_window, double* __restrict__ acc) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_window) return;
    double a = acc[i];
    for (int j = 0; j < n_batch; ++j)
        if (status[b0 + j] == 0) a += (double)rows[(long long)j * n_window + i];
    acc[i] = a;
}

__global__ __launch_bounds__(kThreads) void psf_finish_kernel(const double* __restrict__ acc, int n_window, double n_used, float* __restrict__ psf) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n_window) psf[i] = (float)(acc[i] / n_used);
}

// Stage C.  grid = beads of the batch; a bead that is not used leaves at once (the whole workgroup).
__global__ __launch_bounds__(kThreads) void psf_ncc_kernel(const float* __restrict__ rows, const float* __restrict__ psf, const int32_t* __restrict__ status,
                                                           int b0, int n_window, float* __restrict__ stats) {
    const long long b = (long long)b0 + blockIdx.x;
    if (status[b] != 0) return;
    const float* row = rows + (long long)blockIdx.x * n_window;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};      // sum u, sum p, sum u u, sum p p, sum u p
    for (int i = threadIdx.x; i < n_window; i += kThreads) {
        const double u = (double)row[i], p = (double)psf[i];
        s[0] += u;
        s[1] += p;
        s[2] += u * u;
        s[3] += p * p;
        s[4] += u * p;
    }
    block_sum<5>(s);
    if (threadIdx.x == 0) {
        const double n = (double)n_window;
        const double vu = s[2] - s[0] * s[0] / n, vp = s[3] - s[1] * s[1] / n, cov = s[4] - s[0] * s[1] / n;
        stats[3 * b + 2] = (float)(cov / sqrt(vu * vp));
    }
}

}  // namespace

extern "C" int mvs_psf_extract(int device, const mvs_view_t* view, int32_t ndim, const double* centers, int64_t n_beads,
                               const double window_matrix[9], const int32_t radius[3], int32_t refine_iterations, double* centers_out,
                               int32_t* status_out, float* stats_out, float* psf_out) {
    MvsContext* c0 = mvs_ctx(device);
    if (!view || !centers || !window_matrix || !radius || !centers_out || !status_out || !stats_out || !psf_out)
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_psf_extract: NULL argument");
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_psf_extract: ndim must be 2 or 3");
    int rc = mvs_check_tile_view(c0, "mvs_psf_extract", view, ndim);
    if (rc) return rc;
    for (int k = 3 - ndim; k < 3; ++k)
        if (radius[k] < 1 || radius[k] > MVS_PSF_MAX_RADIUS)
            return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_psf_extract: radius[%d] = %d, must be 1..%d", k, (int)radius[k], MVS_PSF_MAX_RADIUS);
    if (n_beads < 1 || n_beads > ((int64_t)1 << 24)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_psf_extract: n_beads must be 1..2^24");
    if (refine_iterations < 0 || refine_iterations > 64) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_psf_extract: refine_iterations must be 0..64");
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(window_matrix[k])) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_psf_extract: window_matrix is not finite");
    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    PsfArgs P;
    DevView* dv = &P.view;
    rc = mvs_stage_tile_views(c, &view, 1, ndim, nullptr, &dv);
    if (rc) return rc;

    memcpy(P.m, window_matrix, sizeof(P.m));
    P.first_axis = 3 - ndim;
    long long n_window = 1, n_core = 1;
    for (int k = 0; k < 3; ++k) {
        P.r[k] = k < P.first_axis ? 0 : (int)radius[k];
        P.w[k] = 2 * P.r[k] + 1;
        n_window *= P.w[k];
        if (k >= P.first_axis) n_core *= P.w[k] - 2;
    }
    P.n_window = (int)n_window;                    // <= 63^3
    P.n_shell = (int)(n_window - n_core);          // >= 8: every used axis has r >= 1
    P.refine = refine_iterations;

    const size_t row_bytes = (size_t)n_window * sizeof(float);
    int64_t batch = c->psf_batch > 0 ? c->psf_batch : (int64_t)std::max<size_t>(kRowBudget / row_bytes, 1);
    batch = std::min<int64_t>(std::min<int64_t>(batch, n_beads), 1 << 20);
    const int64_t n_batches = (n_beads + batch - 1) / batch;
    P.rows = (float*)mvs_scratch(c, 1, (size_t)batch * row_bytes);
    if (!P.rows) return mvs_alloc_failed(c);
    const size_t ctr_bytes = (size_t)n_beads * 3 * sizeof(double), st_bytes = (size_t)n_beads * sizeof(int32_t);
    const size_t stat_bytes = (size_t)n_beads * 3 * sizeof(float), acc_bytes = (size_t)n_window * sizeof(double);
    char* rec = (char*)mvs_scratch(c, 2, 2 * align_up(ctr_bytes) + align_up(st_bytes) + align_up(stat_bytes) + align_up(acc_bytes) + align_up(row_bytes));
    if (!rec) return mvs_alloc_failed(c);
    double* d_in = (double*)rec;
    P.centers_in = d_in;
    P.centers_out = (double*)(rec + align_up(ctr_bytes));
    P.status = (int32_t*)(rec + 2 * align_up(ctr_bytes));
    P.stats = (float*)(rec + 2 * align_up(ctr_bytes) + align_up(st_bytes));
    double* acc = (double*)(rec + 2 * align_up(ctr_bytes) + align_up(st_bytes) + align_up(stat_bytes));
    float* psf = (float*)((char*)acc + align_up(acc_bytes));

    MVS_HIP_TRY(c, hipMemcpyAsync(d_in, centers, ctr_bytes, hipMemcpyHostToDevice, c->stream));
    MVS_HIP_TRY(c, hipMemsetAsync(acc, 0, acc_bytes, c->stream));
    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    const int offset_blocks = (int)((n_window + kThreads - 1) / kThreads);
    auto launch_windows = [&](int64_t b0, int nb) {
        P.b0 = (int)b0;
        mvs_dispatch_dtype(view->dtype, [&](auto tag) {
            hipLaunchKernelGGL((psf_window_kernel<decltype(tag)>), dim3(nb), dim3(kThreads), 0, c->stream, P);
        });
    };
    for (int64_t b0 = 0; b0 < n_beads; b0 += batch) {
        const int nb = (int)std::min<int64_t>(batch, n_beads - b0);
        launch_windows(b0, nb);
        MVS_HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(psf_accumulate_kernel, dim3(offset_blocks), dim3(kThreads), 0, c->stream, (const float*)P.rows, (const int32_t*)P.status,
                           (int)b0, nb, P.n_window, acc);
        MVS_HIP_TRY(c, hipGetLastError());
    }
    MVS_HIP_TRY(c, hipMemcpyAsync(status_out, P.status, st_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    int64_t n_used = 0;
    for (int64_t b = 0; b < n_beads; ++b) n_used += status_out[b] == 0;

    if (n_used > 0) {
        hipLaunchKernelGGL(psf_finish_kernel, dim3(offset_blocks), dim3(kThreads), 0, c->stream, (const double*)acc, P.n_window, (double)n_used, psf);
        MVS_HIP_TRY(c, hipGetLastError());
        for (int64_t b0 = 0; b0 < n_beads; b0 += batch) {
            const int nb = (int)std::min<int64_t>(batch, n_beads - b0);
            if (n_batches > 1) {      // the rows of this batch are gone: the same launch writes the same rows again
                launch_windows(b0, nb);
                MVS_HIP_TRY(c, hipGetLastError());
            }
            hipLaunchKernelGGL(psf_ncc_kernel, dim3(nb), dim3(kThreads), 0, c->stream, (const float*)P.rows, (const float*)psf, (const int32_t*)P.status,
                               (int)b0, P.n_window, P.stats);
            MVS_HIP_TRY(c, hipGetLastError());
        }
        MVS_HIP_TRY(c, hipMemcpyAsync(psf_out, psf, row_bytes, hipMemcpyDeviceToHost, c->stream));
    } else {
        memset(psf_out, 0, row_bytes);
    }
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    MVS_HIP_TRY(c, hipMemcpyAsync(centers_out, P.centers_out, ctr_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipMemcpyAsync(stats_out, P.stats, stat_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MVS_OK;
}
