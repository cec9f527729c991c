// mvs_affine_mi.hip -- the Mattes mutual-information metric of affine_registration: the joint histogram of a warped crop pair
// (mvs_affine_joint_hist), the gradient reduction over the same samples (mvs_affine_mi_gradient) and the finite range of a crop
// (mvs_finite_range).  Contracts: include/mvs_hip.h.  Per-sample arithmetic: mvs_affine_reg_dev.h (warp, validity) and
// mvs_affine_mi_dev.h (bins, windows, weights).
//
// Both kernels take the walk of mvs_affine_walk_dev.h, shared with affine_neq_kernel (mvs_affine_reg.hip): a block is 4 waves
// over 64 consecutive x columns, a thread keeps its x (and the block its z) and walks mvs_aw::RUN rows.
//
// Histogram.  The weights are integers (2^20 per sample, spread over four moving bins), so a sum is the same in every order
// and atomics keep the result bit-reproducible.  A block adds into LDS copies of the B x B table with 64-bit LDS atomics and
// then adds each non-zero entry into the global table with one 64-bit global atomic.  Neighbouring lanes of a smooth crop hit
// the same bin: lane l uses copy l % copies (16 copies up to B = 16, 4 up to B = 32, 1 above: at most 32 KB), and a copy
// starts one entry after a multiple of B * B so that equal bins of different copies lie in different banks.
//
// Gradient.  A thread carries sum w g_j and sum w g_j y for its run in float32 (w from the table in LDS), multiplies by the
// powers of its x in double at the end of the run, the block reduces in double (shuffles, then LDS, fixed order), expands by its
// z and writes one row of partials; a second launch adds the rows in a fixed order.  No floating-point atomics.
#include <algorithm>

#include "mvs_affine_mi_dev.h"
#include "mvs_affine_walk.h"

namespace {

using mvs_aw::WAVES;
using mvs_aw::wave_sum;

struct MiParams : mvs_aw::Walk {
    float f_lo, f_scale, m_lo, m_scale;
    int B;               // bins per axis
    int copies, stride;  // histogram only: LDS copies and the distance between them in entries
};

// hist: B * B entries [a][b], then the valid count; zeroed before the launch
template <int ND>
__global__ __launch_bounds__(WAVES * 64) void mi_hist_kernel(MiParams P, unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned long long lds[];      // copies * stride entries
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int B = P.B, nb2 = B * B;
    for (int i = threadIdx.x; i < P.copies * P.stride; i += WAVES * 64) lds[i] = 0ull;
    __syncthreads();

    const mvs_aw::BlockPos bp = mvs_aw::block_pos(P, blockIdx.x);
    const long long x = (long long)bp.xb * 64 + lane;
    const double dxd = (double)x - P.c[2];
    const double dzd = ND == 3 ? (double)bp.z - P.c[0] : 0.0;
    unsigned long long* mine = lds + (lane & (P.copies - 1)) * P.stride;
    int n = 0;
    mvs_aw::walk_run<ND>(P, bp.z, bp.yc, wave, x, dzd, dxd, [&](float fv, float v, const float*, float) {
        const int a = mvs_mi::fixed_bin(fv, P.f_lo, P.f_scale, B);
        long long q[4];
        const int b0 = mvs_mi::hist_weights(mvs_mi::moving_coord(v, P.m_lo, P.m_scale, B), q);
        unsigned long long* row = mine + a * B + b0;      // a in 0..B-1 and b0 in 0..B-4 for every input: see the header
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (q[k] != 0) atomicAdd(&row[k], (unsigned long long)q[k]);
        ++n;
    });
    __syncthreads();

    for (int i = threadIdx.x; i < nb2; i += WAVES * 64) {
        unsigned long long s = 0ull;
        for (int cpy = 0; cpy < P.copies; ++cpy) s += lds[cpy * P.stride + i];
        if (s != 0ull) atomicAdd(&hist[i], s);
    }
    n = mvs_fold::wave_fold(mvs_fold::Sums<int>{{n}}).v[0];
    if (lane == 0 && n != 0) atomicAdd(&hist[nb2], (unsigned long long)n);
}

template <int ND>
struct GradLayout {
    static constexpr int NV = ND * 3 + 1;             // values a thread hands to the block reduction
    static constexpr int NOUT = ND * (ND + 1) + 1;    // sums of one block: w g_k (x - c)_m and w g_k in the order of the rows of [A | t], the count
};

template <int ND>
__global__ __launch_bounds__(WAVES * 64) void mi_grad_kernel(MiParams P, const float* __restrict__ table, double* __restrict__ partials) {
    using L = GradLayout<ND>;
    __shared__ float tab[mvs_mi::MAX_BINS * mvs_mi::MAX_BINS];
    __shared__ double red[WAVES][L::NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int B = P.B;
    for (int i = threadIdx.x; i < B * B; i += WAVES * 64) tab[i] = table[i];
    __syncthreads();

    const mvs_aw::BlockPos bp = mvs_aw::block_pos(P, blockIdx.x);
    const long long x = (long long)bp.xb * 64 + lane;
    const double dxd = (double)x - P.c[2];
    const double dzd = ND == 3 ? (double)bp.z - P.c[0] : 0.0;
    float R0[ND], R1[ND], s_n = 0.f;
#pragma unroll
    for (int k = 0; k < ND; ++k) R0[k] = R1[k] = 0.f;
    mvs_aw::walk_run<ND>(P, bp.z, bp.yc, wave, x, dzd, dxd, [&](float fv, float v, const float* g, float dy) {
        const int a = mvs_mi::fixed_bin(fv, P.f_lo, P.f_scale, B);
        const float w = mvs_mi::gradient_weight(mvs_mi::moving_coord(v, P.m_lo, P.m_scale, B), tab + a * B);
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            const float wg = w * g[k];
            R0[k] += wg;
            R1[k] = fmaf(wg, dy, R1[k]);
        }
        s_n += 1.f;
    });

    // per thread: the moments times the powers of its x, in the order (y, x, 1) per gradient component
    int iv = 0;
    auto put = [&](double val) {
        val = wave_sum(val);
        if (lane == 0) red[wave][iv] = val;
        ++iv;
    };
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        put((double)R1[k]);
        put(dxd * (double)R0[k]);
        put((double)R0[k]);
    }
    put((double)s_n);
    __syncthreads();

    const int j = threadIdx.x;
    if (j < L::NOUT) {
        auto tot = [&](int i) { return ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i]; };
        double val;
        if (j < ND * (ND + 1)) {
            const int k = j / (ND + 1), m = j % (ND + 1), base = k * 3;
            if (ND == 2) val = tot(base + m);
            else val = m == 0 ? dzd * tot(base + 2) : tot(base + m - 1);
        } else {
            val = tot(ND * 3);
        }
        partials[(size_t)blockIdx.x * L::NOUT + j] = val;
    }
}

// minimum, maximum and count of the finite values, per block: part[b] = (min, max), cnt[b]
__global__ __launch_bounds__(256) void finite_range_kernel(const float* __restrict__ a, long long n, float2* __restrict__ part,
                                                           long long* __restrict__ cnt) {
    mvs_fold::Range<long long> r = {INFINITY, -INFINITY, 0};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float v = a[i];
        if (mvs_ar::finite_f(v)) r.merge({v, v, 1});
    }
    r = mvs_fold::block_fold<4>(r);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = make_float2(r.mn, r.mx);
        cnt[blockIdx.x] = r.n;
    }
}

// The checks and the parameter block the two metric entries share.  mi_setup: *c is the locked context's.
int mi_check_args(MvsContext* c0, const char* who, const void* fixed, const void* moving, int32_t mem, int32_t ndim, const int64_t* shape,
                  const double* matrix, const double* offset, int32_t n_bins, const void* out0, const void* out1) {
    if (n_bins < mvs_mi::MIN_BINS || n_bins > mvs_mi::MAX_BINS) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: n_bins must be in 8..64", who);
    return affine_check_args(c0, who, fixed, moving, mem, ndim, shape, matrix, offset, out0, out1);
}

int mi_setup(MvsContext* c, const char* who, const float* fixed, const float* moving, int32_t mem, const int64_t shape[3], const double matrix[9],
             const double offset[3], int32_t n_bins, float f_lo, float f_scale, float m_lo, float m_scale, MiParams* P, long long* nblocks) {
    P->f_lo = f_lo;
    P->f_scale = f_scale;
    P->m_lo = m_lo;
    P->m_scale = m_scale;
    P->B = n_bins;
    P->copies = n_bins <= 16 ? 16 : (n_bins <= 32 ? 4 : 1);
    P->stride = n_bins * n_bins + (P->copies > 1 ? 1 : 0);
    return affine_walk_setup(c, who, fixed, moving, mem, shape, matrix, offset, P, nblocks);
}

}  // namespace

extern "C" int mvs_affine_joint_hist(int device, const float* fixed, const float* moving, int32_t mem, int32_t ndim, const int64_t shape[3],
                                     const double matrix[9], const double offset[3], int32_t n_bins, float f_lo, float f_scale, float m_lo,
                                     float m_scale, int64_t* hist_out, int64_t* n_valid_out) {
    const char* who = "mvs_affine_joint_hist";
    int rc = mi_check_args(mvs_ctx(device), who, fixed, moving, mem, ndim, shape, matrix, offset, n_bins, hist_out, n_valid_out);
    if (rc) return rc;
    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));
    MiParams P;
    long long nblocks;
    rc = mi_setup(c, who, fixed, moving, mem, shape, matrix, offset, n_bins, f_lo, f_scale, m_lo, m_scale, &P, &nblocks);
    if (rc) return rc;

    const size_t nent = (size_t)n_bins * n_bins + 1;
    unsigned long long* dhist = (unsigned long long*)mvs_scratch(c, 3, nent * 8);
    if (!dhist) return mvs_alloc_failed(c);
    void *mb_host = nullptr, *mb_dev = nullptr;
    rc = mvs_mailbox(c, nent * 8, &mb_host, &mb_dev);
    if (rc) return rc;
    MVS_HIP_TRY(c, hipMemsetAsync(dhist, 0, nent * 8, c->stream));
    const size_t lds_bytes = (size_t)P.copies * P.stride * 8;
    if (ndim == 3) hipLaunchKernelGGL(mi_hist_kernel<3>, dim3((unsigned)nblocks), dim3(WAVES * 64), lds_bytes, c->stream, P, dhist);
    else hipLaunchKernelGGL(mi_hist_kernel<2>, dim3((unsigned)nblocks), dim3(WAVES * 64), lds_bytes, c->stream, P, dhist);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipMemcpyAsync(mb_host, dhist, nent * 8, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int64_t* h = (const int64_t*)mb_host;
    for (size_t i = 0; i + 1 < nent; ++i) hist_out[i] = h[i];
    *n_valid_out = h[nent - 1];
    return MVS_OK;
}

extern "C" int mvs_affine_mi_gradient(int device, const float* fixed, const float* moving, int32_t mem, int32_t ndim, const int64_t shape[3],
                                      const double matrix[9], const double offset[3], int32_t n_bins, float f_lo, float f_scale, float m_lo,
                                      float m_scale, const float* table, double* out) {
    const char* who = "mvs_affine_mi_gradient";
    int rc = mi_check_args(mvs_ctx(device), who, fixed, moving, mem, ndim, shape, matrix, offset, n_bins, table, out);
    if (rc) return rc;
    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));
    MiParams P;
    long long nblocks;
    rc = mi_setup(c, who, fixed, moving, mem, shape, matrix, offset, n_bins, f_lo, f_scale, m_lo, m_scale, &P, &nblocks);
    if (rc) return rc;

    const int nout = ndim == 3 ? GradLayout<3>::NOUT : GradLayout<2>::NOUT;
    const size_t tab_bytes = align_up((size_t)n_bins * n_bins * sizeof(float));
    char* work = (char*)mvs_scratch(c, 3, tab_bytes + (size_t)nblocks * nout * sizeof(double));
    if (!work) return mvs_alloc_failed(c);
    float* dtab = (float*)work;
    double* partials = (double*)(work + tab_bytes);
    void *mb_host = nullptr, *mb_dev = nullptr;
    rc = mvs_mailbox(c, (size_t)nout * sizeof(double), &mb_host, &mb_dev);
    if (rc) return rc;
    MVS_HIP_TRY(c, hipMemcpyAsync(dtab, table, (size_t)n_bins * n_bins * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (ndim == 3) hipLaunchKernelGGL(mi_grad_kernel<3>, dim3((unsigned)nblocks), dim3(WAVES * 64), 0, c->stream, P, dtab, partials);
    else hipLaunchKernelGGL(mi_grad_kernel<2>, dim3((unsigned)nblocks), dim3(WAVES * 64), 0, c->stream, P, dtab, partials);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(mvs_aw::rows_sum_kernel, dim3(nout), dim3(256), 0, c->stream, partials, nblocks, nout, (double*)mb_dev);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < MVS_AFFINE_MI_GRAD_LEN; ++i) out[i] = i < nout ? ((const double*)mb_host)[i] : 0.0;
    return MVS_OK;
}

extern "C" int mvs_finite_range(int device, const float* data, int32_t mem, int64_t n, float* min_out, float* max_out, int64_t* n_finite_out) {
    MvsContext* c0 = mvs_ctx(device);
    if (!data || !min_out || !max_out || !n_finite_out || n < 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_finite_range: bad argument");
    if (mem != MVS_MEM_HOST && mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_finite_range: bad mem");
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));
    float* d;
    rc = mvs_stage_float_volume(c, data, mem, n, 4, &d);
    if (rc) return rc;
    const int nb = (int)std::min<long long>((n + 256 * 8 - 1) / (256 * 8), 512);
    void *mb_host = nullptr, *mb_dev = nullptr;
    rc = mvs_mailbox(c, (size_t)nb * 16, &mb_host, &mb_dev);
    if (rc) return rc;
    hipLaunchKernelGGL(finite_range_kernel, dim3(nb), dim3(256), 0, c->stream, d, (long long)n, (float2*)mb_dev,
                       (long long*)((char*)mb_dev + (size_t)nb * 8));
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const float2* part = (const float2*)mb_host;
    const long long* cnt = (const long long*)((const char*)mb_host + (size_t)nb * 8);
    float mn = INFINITY, mx = -INFINITY;
    long long nv = 0;
    for (int i = 0; i < nb; ++i) {
        mn = std::min(mn, part[i].x);
        mx = std::max(mx, part[i].y);
        nv += cnt[i];
    }
    if (nv == 0) mn = mx = NAN;
    *min_out = mn;
    *max_out = mx;
    *n_finite_out = nv;
    return MVS_OK;
}
