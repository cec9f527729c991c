// mvs_detect.hip -- bead detection on the GPU (gfx950): mvs_log_response and mvs_local_maxima (include/mvs_hip.h).
//
// The reference's detection.log_detect (src/multiview_stitcher/detection.py) is, per voxel,
//   response = -scipy.ndimage.gaussian_laplace(image as float32, sigma, mode="reflect") * mean(sigma)^2
//   detections = (response == maximum_filter(response, size, mode="reflect")) & (response > threshold) & (response > 0)
//                [& (minimum_filter(sample, size_2, mode="reflect") < max_neigh_intensity)]
// followed by a connected-component labelling and a centre of mass.  Here the first line is mvs_log_response, the second
// mvs_local_maxima, and what leaves the device is the list of detected voxels (labelling a few thousand coordinates is host work).
//
// mvs_log_response: scipy forms the Laplacian as ndim separable filters of ndim line passes each (order 2 along one axis, order 0
// along the others).  The same sum comes out of ndim line passes that carry two volumes:
//   along x:  A = G I,  B = G'' I          along y:  C = G A,  D = G'' A + G B          along z:  L = G D + G'' C
// (2D: the y pass is the last one, L = G B + G'' A).  Every pass accumulates in float64 over float64 taps -- centre tap, then the
// pairs from the farthest to the nearest, scipy's order for a symmetric kernel -- and stores float32, like scipy after each axis.
// A workgroup stages its lines, reflected ends included, in LDS once; the reflection is worked out per staged sample, so a radius
// above the axis length (several reflections) and an axis of one sample need nothing special.  The last pass also leaves the
// maximum of each workgroup; a second small launch reduces those (no atomics: a maximum does not depend on the order).
//
// mvs_local_maxima: the box maximum is separable, so it is a running maximum along x, one along y, and a last pass along the
// first axis which only looks at voxels above the threshold, compares, applies the neighbourhood-minimum rule at the remaining
// candidates and appends them to the list with one integer atomicAdd per wave.
#include "mvs_detect_dev.h"
#include "mvs_fold_dev.h"
#include "mvs_internal.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int DT_COLS = 64;       // x columns of a tile: one per lane
constexpr int DT_SEG = 32;        // outputs along y / z a workgroup produces per column
constexpr int DT_XROWS = 16;      // rows a workgroup of the x pass takes

struct Dims { int n[3]; };        // z, y, x

// ---- line passes of the Gaussian / Laplacian-of-Gaussian ------------------------------------------------------------------------
// along x: grid = ceil(rows / DT_XROWS) * ceil(nx / 64); LDS [DT_XROWS][64 + 2 r]
template <typename T, bool LOG>
__global__ __launch_bounds__(256) void log_x_kernel(const T* __restrict__ src, float* __restrict__ A, float* __restrict__ B, Dims S, int r,
                                                    const double* __restrict__ w0, const double* __restrict__ w2) {
    extern __shared__ float sl[];
    const int nx = S.n[2], pitch = DT_COLS + 2 * r;
    const long long nrows = (long long)S.n[0] * S.n[1];
    const int nxb = (nx + DT_COLS - 1) / DT_COLS;
    const long long row0 = (long long)(blockIdx.x / nxb) * DT_XROWS;
    const int x0 = (int)(blockIdx.x % nxb) * DT_COLS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int rr = wave; rr < DT_XROWS; rr += 4) {      // a wave stages the rows it filters (and its neighbours')
        const long long row = row0 + rr;
        for (int k = lane; k < pitch; k += 64)
            sl[rr * pitch + k] = row < nrows ? (float)src[row * nx + mvs_det::reflect(x0 + k - r, nx)] : 0.f;
    }
    __syncthreads();
    const int x = x0 + lane;
    if (x >= nx) return;
    for (int rr = wave; rr < DT_XROWS; rr += 4) {
        const long long row = row0 + rr;
        if (row >= nrows) break;
        const float* c = sl + rr * pitch + lane + r;
        double a = (double)c[0] * w0[r], b = LOG ? (double)c[0] * w2[r] : 0.0;
        for (int j = r; j >= 1; --j) {
            const double s = (double)c[-j] + (double)c[j];
            a += s * w0[r - j];
            if (LOG) b += s * w2[r - j];
        }
        A[row * nx + x] = (float)a;
        if (LOG) B[row * nx + x] = (float)b;
    }
}

// along y (axis 1) or z (axis 0): a tile is 64 x columns times DT_SEG positions of one plane (fixed z, or fixed y);
// grid = ceil(nx / 64) * ceil(len / DT_SEG) * (extent of the other axis); LDS [DT_SEG + 2 r][64] per staged volume.
//   not LAST:  O1 = G P,  O2 = G'' P + G Q            LAST:  O1 = (G'' P + G Q) * factor   (smoothing: O1 = G P, both times)
// LAST also writes the maximum of the workgroup's outputs whose position along the axis lies in [mlo, mhi) to partial[blockIdx.x]
// (-inf when there is none; NaN never wins a comparison).
template <bool LOG, bool LAST>
__global__ __launch_bounds__(256) void log_s_kernel(const float* __restrict__ P, const float* __restrict__ Q, float* __restrict__ O1,
                                                    float* __restrict__ O2, Dims S, int axis, int r, const double* __restrict__ w0,
                                                    const double* __restrict__ w2, double factor, float* __restrict__ partial, int mlo, int mhi) {
    extern __shared__ float sl[];
    const int nx = S.n[2], len = S.n[axis];
    const long long st = axis == 0 ? (long long)S.n[1] * nx : nx;            // stride along the axis
    const long long ost = axis == 0 ? nx : (long long)S.n[1] * nx;           // stride of the other outer axis
    const int nxb = (nx + DT_COLS - 1) / DT_COLS, nseg = (len + DT_SEG - 1) / DT_SEG;
    long long b = blockIdx.x;
    const int x0 = (int)(b % nxb) * DT_COLS;
    b /= nxb;
    const int p0 = (int)(b % nseg) * DT_SEG;
    const long long base = (b / nseg) * ost;
    const int rows = DT_SEG + 2 * r;
    float* sp = sl;
    float* sq = sl + rows * DT_COLS;
    for (int idx = threadIdx.x; idx < rows * DT_COLS; idx += blockDim.x) {
        const int k = idx >> 6, x = x0 + (idx & 63);
        const long long i = base + (long long)mvs_det::reflect(p0 + k - r, len) * st + x;
        sp[idx] = x < nx ? P[i] : 0.f;
        if (LOG) sq[idx] = x < nx ? Q[i] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = x0 + lane;
    float best = -INFINITY;
    if (x < nx) {
        for (int k = wave; k < DT_SEG; k += 4) {
            const int pos = p0 + k;
            if (pos >= len) break;
            const float* cp = sp + (k + r) * DT_COLS + lane;
            const float* cq = sq + (k + r) * DT_COLS + lane;
            double g1 = (double)cp[0] * w0[r], h = 0.0;
            if (LOG) h = (double)cp[0] * w2[r] + (double)cq[0] * w0[r];
            for (int j = r; j >= 1; --j) {
                const double s1 = (double)cp[-j * DT_COLS] + (double)cp[j * DT_COLS];
                g1 += s1 * w0[r - j];
                if (LOG) {
                    const double s2 = (double)cq[-j * DT_COLS] + (double)cq[j * DT_COLS];
                    h += s1 * w2[r - j] + s2 * w0[r - j];
                }
            }
            const long long o = base + (long long)pos * st + x;
            if (LAST) {
                const float v = LOG ? (float)(h * factor) : (float)g1;
                O1[o] = v;
                if (pos >= mlo && pos < mhi && v > best) best = v;
            } else {
                O1[o] = (float)g1;
                if (LOG) O2[o] = (float)h;
            }
        }
    }
    if (LAST) {
        best = mvs_fold::block_fold<4>(mvs_fold::Max<float>{best}).v;
        if (threadIdx.x == 0) partial[blockIdx.x] = best;
    }
}

// the maximum of the workgroups' maxima: one workgroup, result in out[0] (NaN when no workgroup had a value)
__global__ __launch_bounds__(256) void max_partials_kernel(const float* __restrict__ partial, long long n, float* __restrict__ out) {
    __shared__ float s[256];
    float best = -INFINITY;
    for (long long i = threadIdx.x; i < n; i += 256) best = fmaxf(best, partial[i]);
    s[threadIdx.x] = best;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s[threadIdx.x] = fmaxf(s[threadIdx.x], s[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = s[0] == -INFINITY ? NAN : s[0];
}

// ---- local maxima -------------------------------------------------------------------------------------------------------------
// running maximum over the window along `axis`.  A workgroup takes tiles of 256 x positions of one row, so a row's (z, y) is
// worked out once per tile on the scalar unit; the window's reads are the neighbours' reads (L1 / L2 hits).
struct Tiles { long long count; int per_row; };      // tiles of 256 x positions; per_row = ceil(nx / 256)

__global__ __launch_bounds__(256) void max_line_kernel(const float* __restrict__ R, float* __restrict__ M, Dims S, Tiles T, int axis, int win) {
    const int nx = S.n[2], ny = S.n[1], len = S.n[axis];
    const long long st = axis == 0 ? (long long)ny * nx : (axis == 1 ? nx : 1);
    for (long long tile = blockIdx.x; tile < T.count; tile += gridDim.x) {
        const long long row = tile / T.per_row;
        const int x = (int)(tile % T.per_row) * 256 + (int)threadIdx.x;
        if (x >= nx) continue;
        const int y = (int)(row % ny), z = (int)(row / ny);
        const int pos = axis == 2 ? x : (axis == 1 ? y : z);
        const long long i = row * nx + x;
        const long long base = i - (long long)pos * st;
        int lo, hi;
        mvs_det::window(pos, win, &lo, &hi);
        float m = -INFINITY;
        for (int p = lo; p <= hi; ++p) m = fmaxf(m, R[base + (long long)mvs_det::reflect(p, len) * st]);
        M[i] = m;
    }
}

template <typename TS> __device__ __forceinline__ bool below_bound(TS mn, double bound) { return (double)mn < bound; }
// (numpy compares a float32 array with a Python number in float32)
template <> __device__ __forceinline__ bool below_bound<float>(float mn, double bound) { return mn < (float)bound; }

struct MinRule { const void* sample; int win[3]; double bound; };

// The last pass: M holds the running maxima of the other axes; a voxel above the threshold takes the maximum of M over the window
// along `axis`, and is a detection when it equals it (and the minimum of the sample volume over its box is below the bound).
// Detections are appended in no particular order; *count ends as their exact number, coords holds the first `cap` that arrived.
template <typename TS>
__global__ __launch_bounds__(256) void maxima_last_kernel(const float* __restrict__ R, const float* __restrict__ M, Dims S, int axis, int win,
                                                          float threshold, MinRule mr, Tiles T, int32_t* __restrict__ coords, long long cap,
                                                          unsigned long long* __restrict__ count) {
    const int nx = S.n[2], ny = S.n[1], len = S.n[axis];
    const long long st = axis == 0 ? (long long)ny * nx : nx;
    const int lane = threadIdx.x & 63;
    // (the loop is the same for every thread of a workgroup: the wave-wide votes below see whole waves)
    for (long long tile = blockIdx.x; tile < T.count; tile += gridDim.x) {
        const long long row = tile / T.per_row;
        const int x = (int)(tile % T.per_row) * 256 + (int)threadIdx.x;
        const int y = (int)(row % ny), z = (int)(row / ny);
        const long long i = row * nx + x;
        bool cand = false;
        if (x < nx) {
            const float r = R[i];
            if (r > threshold && r > 0.f) {
                const int pos = axis == 0 ? z : y;
                const long long base = i - (long long)pos * st;
                int lo, hi;
                mvs_det::window(pos, win, &lo, &hi);
                float m = -INFINITY;
                for (int p = lo; p <= hi; ++p) m = fmaxf(m, M[base + (long long)mvs_det::reflect(p, len) * st]);
                cand = (r == m);
                if (cand && mr.sample) {
                    const TS* sm = (const TS*)mr.sample;
                    int l0, h0, l1, h1, l2, h2;
                    mvs_det::window(z, mr.win[0], &l0, &h0);
                    mvs_det::window(y, mr.win[1], &l1, &h1);
                    mvs_det::window(x, mr.win[2], &l2, &h2);
                    TS mn = sm[i];
                    for (int a = l0; a <= h0; ++a)
                        for (int bq = l1; bq <= h1; ++bq) {
                            const long long srow = ((long long)mvs_det::reflect(a, S.n[0]) * ny + mvs_det::reflect(bq, ny)) * nx;
                            for (int cq = l2; cq <= h2; ++cq) {
                                const TS v = sm[srow + mvs_det::reflect(cq, nx)];
                                if (v < mn) mn = v;
                            }
                        }
                    cand = below_bound<TS>(mn, mr.bound);
                }
            }
        }
        const unsigned long long votes = __ballot(cand);
        if (votes) {
            const int leader = __ffsll((long long)votes) - 1;
            unsigned long long slot = 0;
            if (lane == leader) slot = atomicAdd(count, (unsigned long long)__popcll(votes));
            slot = __shfl(slot, leader) + (unsigned long long)__popcll(votes & ((1ull << lane) - 1ull));
            if (cand && slot < (unsigned long long)cap) {
                coords[3 * slot + 0] = z;
                coords[3 * slot + 1] = y;
                coords[3 * slot + 2] = x;
            }
        }
    }
}

__global__ void count_out_kernel(const unsigned long long* __restrict__ count, unsigned long long* __restrict__ out) { out[0] = count[0]; }

int check_shape(MvsContext* c, const char* who, int32_t ndim, const int64_t* shape, Dims* S) {
    if (ndim != 2 && ndim != 3) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", who);
    if (!shape) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: NULL argument", who);
    for (int k = 0; k < 3; ++k) {
        if (shape[k] < 1 || (k < 3 - ndim && shape[k] != 1))
            return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: shape must be positive (and 1 along z in 2D)", who);
        if (shape[k] > (1 << 24)) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: axis longer than 2^24", who);
        S->n[k] = (int)shape[k];
    }
    // (the product of three admitted axes can pass 2^63: compare before multiplying)
    if (shape[0] * shape[1] > MVS_DETECT_MAX_VOXELS / shape[2])
        return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: more than MVS_DETECT_MAX_VOXELS (2^34) voxels", who);
    return MVS_OK;
}

// a launch holds fewer than 2^32 threads: with workgroups of 256 that is the limit on a grid
constexpr long long kMaxWorkgroups = (1ll << 24) - 1;

}  // namespace

extern "C" int mvs_log_response(int device, const void* image, int32_t dtype, int32_t mem, int32_t ndim, const int64_t shape[3],
                                const int32_t radius[3], const double* taps0, const double* taps2, double scale,
                                const int64_t* max_range, float* response, float* max_out) {
    MvsContext* c0 = mvs_ctx(device);
    Dims S;
    int rc = check_shape(c0, "mvs_log_response", ndim, shape, &S);
    if (rc) return rc;
    if (!image || !radius || !taps0 || !response) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_log_response: NULL argument");
    if (mem != MVS_MEM_HOST && mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_log_response: bad mem");
    const size_t es = mvs_dtype_size(dtype);
    if (!es) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_log_response: dtype must be uint8, uint16 or float32");
    const int a0 = 3 - ndim;                       // the image's first axis
    size_t ntaps = 0, tap_off[3] = {0, 0, 0};
    for (int k = a0; k < 3; ++k) {
        if (radius[k] < 0) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_log_response: negative radius");
        if (radius[k] > MVS_LOG_MAX_RADIUS)
            return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_log_response: radius %d above MVS_LOG_MAX_RADIUS (%d)", (int)radius[k], MVS_LOG_MAX_RADIUS);
        tap_off[k] = ntaps;
        ntaps += (size_t)(2 * radius[k] + 1);
    }
    int mlo = 0, mhi = S.n[a0];
    if (max_range) {
        if (max_range[0] < 0 || max_range[1] > S.n[a0] || max_range[0] > max_range[1])
            return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_log_response: max_range outside the first axis");
        mlo = (int)max_range[0];
        mhi = (int)max_range[1];
    }
    const bool lg = taps2 != nullptr;
    const int nxb = (S.n[2] + DT_COLS - 1) / DT_COLS;
    const long long nrows = (long long)S.n[0] * S.n[1];
    const long long grid_x = (nrows + DT_XROWS - 1) / DT_XROWS * nxb;
    long long grid_s[2];                           // axis 0 (z), axis 1 (y)
    for (int axis = 0; axis < 2; ++axis)
        grid_s[axis] = (long long)nxb * ((S.n[axis] + DT_SEG - 1) / DT_SEG) * S.n[1 - axis];
    if (grid_x > kMaxWorkgroups || grid_s[0] > kMaxWorkgroups || grid_s[1] > kMaxWorkgroups)
        return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_log_response: volume too large (more than 2^24 workgroups in a pass)");

    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    const long long n = nrows * S.n[2];
    const int n_work = lg ? ndim : 1;              // float volumes besides the result (see the pass plan below)
    const size_t tap_bytes = align_up(ntaps * sizeof(double));
    const size_t partial_bytes = align_up((size_t)grid_s[a0] * sizeof(float));
    const size_t stage_bytes = mem == MVS_MEM_HOST ? align_up((size_t)n * es) : 0;
    const size_t vol_bytes = align_up((size_t)n * sizeof(float));
    MvsWorkArea wa(c);
    rc = wa.alloc(2 * tap_bytes + partial_bytes + stage_bytes + (size_t)n_work * vol_bytes);
    if (rc) return rc;
    char* p = (char*)wa.ptr;
    double* d0 = (double*)p;
    double* d2 = (double*)(p + tap_bytes);
    float* partial = (float*)(p + 2 * tap_bytes);
    char* staged = p + 2 * tap_bytes + partial_bytes;
    float* W[3];
    for (int k = 0; k < 3; ++k) W[k] = (float*)(staged + stage_bytes + (size_t)(k < n_work ? k : 0) * vol_bytes);
    void *mb_host = nullptr, *mb_dev = nullptr;
    rc = mvs_mailbox(c, sizeof(float), &mb_host, &mb_dev);
    if (rc) return rc;

    MVS_HIP_TRY(c, hipMemcpyAsync(d0, taps0, ntaps * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (lg) MVS_HIP_TRY(c, hipMemcpyAsync(d2, taps2, ntaps * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const void* src = image;
    if (mem == MVS_MEM_HOST) {
        MVS_HIP_TRY(c, hipMemcpyAsync(staged, image, (size_t)n * es, hipMemcpyHostToDevice, c->stream));
        src = staged;
    }

    // pass plan (R = the caller's volume):  3D LoG  x: I -> R, W0   y: R, W0 -> W1, W2   z: W1, W2 -> R
    //                                       2D LoG  x: I -> W0, W1  y: W0, W1 -> R
    //                                       smoothing  3D: I -> R -> W0 -> R      2D: I -> W0 -> R
    float* xa = ndim == 3 ? response : W[0];
    float* xb = ndim == 3 ? W[0] : W[1];
    {
        const int r = radius[2];
        const size_t lds = (size_t)DT_XROWS * (DT_COLS + 2 * r) * sizeof(float);
        mvs_dispatch_dtype(dtype, [&](auto tag) {
            using T = decltype(tag);
            if (lg) hipLaunchKernelGGL((log_x_kernel<T, true>), dim3((unsigned)grid_x), dim3(256), lds, c->stream, (const T*)src, xa, xb, S, r, d0 + tap_off[2], d2 + tap_off[2]);
            else hipLaunchKernelGGL((log_x_kernel<T, false>), dim3((unsigned)grid_x), dim3(256), lds, c->stream, (const T*)src, xa, xb, S, r, d0 + tap_off[2], d0 + tap_off[2]);
        });
        MVS_HIP_TRY(c, hipGetLastError());
    }
    const double factor = -scale;
    auto strided = [&](int axis, bool last, const float* P, const float* Q, float* O1, float* O2) {
        const int r = radius[axis];
        const size_t lds = (size_t)(DT_SEG + 2 * r) * DT_COLS * sizeof(float) * (lg ? 2 : 1);
        const dim3 g((unsigned)grid_s[axis]), b(256);
        const double *t0 = d0 + tap_off[axis], *t2 = (lg ? d2 : d0) + tap_off[axis];
        if (lg && last) hipLaunchKernelGGL((log_s_kernel<true, true>), g, b, lds, c->stream, P, Q, O1, O2, S, axis, r, t0, t2, factor, partial, mlo, mhi);
        else if (lg) hipLaunchKernelGGL((log_s_kernel<true, false>), g, b, lds, c->stream, P, Q, O1, O2, S, axis, r, t0, t2, factor, partial, mlo, mhi);
        else if (last) hipLaunchKernelGGL((log_s_kernel<false, true>), g, b, lds, c->stream, P, Q, O1, O2, S, axis, r, t0, t2, factor, partial, mlo, mhi);
        else hipLaunchKernelGGL((log_s_kernel<false, false>), g, b, lds, c->stream, P, Q, O1, O2, S, axis, r, t0, t2, factor, partial, mlo, mhi);
    };
    if (ndim == 3) {
        if (lg) {
            strided(1, false, xa, xb, W[1], W[2]);
            MVS_HIP_TRY(c, hipGetLastError());
            strided(0, true, W[1], W[2], response, nullptr);
        } else {
            strided(1, false, xa, xa, W[0], nullptr);
            MVS_HIP_TRY(c, hipGetLastError());
            strided(0, true, W[0], W[0], response, nullptr);
        }
    } else {
        strided(1, true, xa, lg ? xb : xa, response, nullptr);
    }
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(max_partials_kernel, dim3(1), dim3(256), 0, c->stream, partial, grid_s[a0], (float*)mb_dev);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (max_out) *max_out = *(const float*)mb_host;
    return wa.release();
}

extern "C" int mvs_local_maxima(int device, const float* response, int32_t ndim, const int64_t shape[3], const int32_t window[3],
                                float threshold, const void* sample, int32_t sample_dtype, const int32_t sample_window[3], double bound,
                                int32_t* coords_out, int64_t capacity, int64_t* count_out) {
    MvsContext* c0 = mvs_ctx(device);
    Dims S;
    int rc = check_shape(c0, "mvs_local_maxima", ndim, shape, &S);
    if (rc) return rc;
    if (!response || !window || !count_out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_local_maxima: NULL argument");
    if (capacity < 0 || (capacity > 0 && !coords_out)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_local_maxima: capacity without a buffer");
    if (capacity > (int64_t)1 << 40) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_local_maxima: capacity above 2^40");
    const int a0 = 3 - ndim;
    for (int k = a0; k < 3; ++k)
        if (window[k] < 1 || window[k] % 2 == 0 || window[k] > MVS_MAXIMA_MAX_WINDOW)
            return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_local_maxima: windows must be odd, in 1 .. %d", MVS_MAXIMA_MAX_WINDOW);
    MinRule mr;
    mr.sample = sample;
    mr.bound = bound;
    mr.win[0] = mr.win[1] = mr.win[2] = 1;
    if (sample) {
        if (!sample_window) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_local_maxima: sample without a window");
        if (!mvs_dtype_size(sample_dtype)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_local_maxima: sample dtype must be uint8, uint16 or float32");
        for (int k = a0; k < 3; ++k) {
            if (sample_window[k] < 1 || sample_window[k] > MVS_MAXIMA_MAX_WINDOW)
                return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_local_maxima: sample windows must be in 1 .. %d", MVS_MAXIMA_MAX_WINDOW);
            mr.win[k] = sample_window[k];
        }
    }
    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    const long long n = (long long)S.n[0] * S.n[1] * S.n[2];
    const size_t vol_bytes = align_up((size_t)n * sizeof(float));
    const size_t coord_bytes = align_up((size_t)capacity * 3 * sizeof(int32_t));
    const int n_vol = ndim - 1;                    // running maxima along x (and y)
    MvsWorkArea wa(c);
    rc = wa.alloc(256 + coord_bytes + (size_t)n_vol * vol_bytes);
    if (rc) return rc;
    char* p = (char*)wa.ptr;
    unsigned long long* count = (unsigned long long*)p;
    int32_t* coords = (int32_t*)(p + 256);
    float* M1 = (float*)(p + 256 + coord_bytes);
    float* M2 = (float*)(p + 256 + coord_bytes + vol_bytes);
    void *mb_host = nullptr, *mb_dev = nullptr;
    rc = mvs_mailbox(c, sizeof(unsigned long long), &mb_host, &mb_dev);
    if (rc) return rc;

    MVS_HIP_TRY(c, hipMemsetAsync(count, 0, sizeof(unsigned long long), c->stream));
    Tiles T;
    T.per_row = (S.n[2] + 255) / 256;
    T.count = (long long)S.n[0] * S.n[1] * T.per_row;
    const dim3 g((unsigned)std::min<long long>(T.count, 256 * 32)), b(256);
    hipLaunchKernelGGL(max_line_kernel, g, b, 0, c->stream, response, M1, S, T, 2, (int)window[2]);
    MVS_HIP_TRY(c, hipGetLastError());
    const float* M = M1;
    if (ndim == 3) {
        hipLaunchKernelGGL(max_line_kernel, g, b, 0, c->stream, (const float*)M1, M2, S, T, 1, (int)window[1]);
        MVS_HIP_TRY(c, hipGetLastError());
        M = M2;
    }
    mvs_dispatch_dtype(sample ? sample_dtype : MVS_F32, [&](auto tag) {
        using TS = decltype(tag);
        hipLaunchKernelGGL((maxima_last_kernel<TS>), g, b, 0, c->stream, response, M, S, a0, (int)window[a0], threshold, mr, T, coords,
                           (long long)capacity, count);
    });
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(count_out_kernel, dim3(1), dim3(1), 0, c->stream, (const unsigned long long*)count, (unsigned long long*)mb_dev);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned long long found = *(const unsigned long long*)mb_host;
    *count_out = (int64_t)found;
    const size_t stored = (size_t)std::min<unsigned long long>(found, (unsigned long long)capacity);
    if (stored) {
        MVS_HIP_TRY(c, hipMemcpyAsync(coords_out, coords, stored * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return wa.release();
}
