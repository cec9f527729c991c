// mvs_affine_mi.hip -- the Mattes mutual-information metric of affine_registration: the joint histogram of a warped crop pair
// (mvs_affine_joint_hist), the gradient reduction over the same samples (mvs_affine_mi_gradient) and the finite range of a crop
// (mvs_finite_range).  Contracts: include/mvs_hip.h.  Per-sample arithmetic: mvs_affine_reg_dev.h (warp, validity) and
// mvs_affine_mi_dev.h (bins, windows, weights).
//
// Both walks have the geometry of affine_neq_kernel (mvs_affine_reg.hip): a block is 4 waves over 64 consecutive x columns, a
// thread keeps its x (and the block its z) and walks MI_RUN rows.
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
#include "mvs_affine_reg_dev.h"
#include "mvs_internal.h"

int mvs_stage_float_volume(MvsContext* c, const float* src, int32_t mem, long long n, int slot, float** dptr);   // mvs_reg.hip

namespace {

constexpr int MI_WAVES = 4;      // waves of a block: wave w takes rows y0 + w, y0 + w + 4, ...
constexpr int MI_RUN = 32;       // rows per thread: the length of a float32 run sum

struct MiParams {
    const float* fixed;
    const float* moving;
    long long n[3];      // z, y, x (z = 1 in 2D)
    double A[9];         // 3x3, row-major (z, y, x); 2D uses the lower right 2x2
    double o[3];         // c + t
    double c[3];
    float f_lo, f_scale, m_lo, m_scale;
    int B;               // bins per axis
    int copies, stride;  // histogram only: LDS copies and the distance between them in entries
    int nxb, nyc;        // blocks along x and y
};

// The samples of one thread's run: f(fixed value, moving value, gradient, y - c_y as float) for every valid one.
template <int ND, typename F>
__device__ __forceinline__ void walk_run(const MiParams& P, long long z, int yc, int wave, long long x, double dzd, double dxd, F&& f) {
    const long long ny = P.n[1], nx = P.n[2];
    if (x >= nx) return;
    // the products of the coordinate that do not change along the run (each rounds on its own, as in coord2 / coord3)
    double az[3], ax[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        az[k] = P.A[k * 3 + 0] * dzd;
        ax[k] = P.A[k * 3 + 2] * dxd;
    }
    const long long y0 = (long long)yc * (MI_WAVES * MI_RUN) + wave;
    const float* __restrict__ frow = P.fixed + (z * ny + y0) * nx + x;
    for (int i = 0; i < MI_RUN; ++i, frow += MI_WAVES * nx) {
        const long long y = y0 + (long long)i * MI_WAVES;
        if (y >= ny) break;
        const float fv = *frow;
        if (!mvs_ar::finite_f(fv)) continue;
        const double dyd = (double)y - P.c[1];
        float v, g[ND];
        if constexpr (ND == 3) {
            long long iz, iy, ix;
            float fz, fy, fx;
            if (!mvs_ar::split(((az[0] + P.A[1] * dyd) + ax[0]) + P.o[0], P.n[0], &iz, &fz)) continue;
            if (!mvs_ar::split(((az[1] + P.A[4] * dyd) + ax[1]) + P.o[1], ny, &iy, &fy)) continue;
            if (!mvs_ar::split(((az[2] + P.A[7] * dyd) + ax[2]) + P.o[2], nx, &ix, &fx)) continue;
            const float* __restrict__ m = P.moving + (iz * ny + iy) * nx + ix;
            const long long sz = ny * nx;
            const float taps[8] = {m[0], m[1], m[nx], m[nx + 1], m[sz], m[sz + 1], m[sz + nx], m[sz + nx + 1]};
            if (!mvs_ar::sample3(taps, fz, fy, fx, &v, g)) continue;
        } else {
            long long iy, ix;
            float fy, fx;
            if (!mvs_ar::split((P.A[4] * dyd + ax[1]) + P.o[1], ny, &iy, &fy)) continue;
            if (!mvs_ar::split((P.A[7] * dyd + ax[2]) + P.o[2], nx, &ix, &fx)) continue;
            const float* __restrict__ m = P.moving + iy * nx + ix;
            const float taps[4] = {m[0], m[1], m[nx], m[nx + 1]};
            if (!mvs_ar::sample2(taps, fy, fx, &v, g)) continue;
        }
        f(fv, v, g, (float)dyd);
    }
}

struct BlockPos {
    int xb, yc;
    long long z;
};
__device__ __forceinline__ BlockPos block_pos(const MiParams& P) {
    long long b = blockIdx.x;
    BlockPos r;
    r.xb = (int)(b % P.nxb);
    b /= P.nxb;
    r.yc = (int)(b % P.nyc);
    r.z = b / P.nyc;
    return r;
}

// hist: B * B entries [a][b], then the valid count; zeroed before the launch
template <int ND>
__global__ __launch_bounds__(MI_WAVES * 64) void mi_hist_kernel(MiParams P, unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned long long lds[];      // copies * stride entries
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int B = P.B, nb2 = B * B;
    for (int i = threadIdx.x; i < P.copies * P.stride; i += MI_WAVES * 64) lds[i] = 0ull;
    __syncthreads();

    const BlockPos bp = block_pos(P);
    const long long x = (long long)bp.xb * 64 + lane;
    const double dxd = (double)x - P.c[2];
    const double dzd = ND == 3 ? (double)bp.z - P.c[0] : 0.0;
    unsigned long long* mine = lds + (lane & (P.copies - 1)) * P.stride;
    int n = 0;
    walk_run<ND>(P, bp.z, bp.yc, wave, x, dzd, dxd, [&](float fv, float v, const float*, float) {
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

    for (int i = threadIdx.x; i < nb2; i += MI_WAVES * 64) {
        unsigned long long s = 0ull;
        for (int cpy = 0; cpy < P.copies; ++cpy) s += lds[cpy * P.stride + i];
        if (s != 0ull) atomicAdd(&hist[i], s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
    if (lane == 0 && n != 0) atomicAdd(&hist[nb2], (unsigned long long)n);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

template <int ND>
struct GradLayout {
    static constexpr int NV = ND * 3 + 1;             // values a thread hands to the block reduction
    static constexpr int NOUT = ND * (ND + 1) + 1;    // sums of one block: w g_k (x - c)_m and w g_k in the order of the rows of [A | t], the count
};

template <int ND>
__global__ __launch_bounds__(MI_WAVES * 64) void mi_grad_kernel(MiParams P, const float* __restrict__ table, double* __restrict__ partials) {
    using L = GradLayout<ND>;
    __shared__ float tab[mvs_mi::MAX_BINS * mvs_mi::MAX_BINS];
    __shared__ double red[MI_WAVES][L::NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int B = P.B;
    for (int i = threadIdx.x; i < B * B; i += MI_WAVES * 64) tab[i] = table[i];
    __syncthreads();

    const BlockPos bp = block_pos(P);
    const long long x = (long long)bp.xb * 64 + lane;
    const double dxd = (double)x - P.c[2];
    const double dzd = ND == 3 ? (double)bp.z - P.c[0] : 0.0;
    float R0[ND], R1[ND], s_n = 0.f;
#pragma unroll
    for (int k = 0; k < ND; ++k) R0[k] = R1[k] = 0.f;
    walk_run<ND>(P, bp.z, bp.yc, wave, x, dzd, dxd, [&](float fv, float v, const float* g, float dy) {
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

// out[j] = sum over the blocks of partials[b][j]: thread t takes b = t, t + 256, ... in order, then a fixed tree in LDS
// (the scheme of affine_neq_sum_kernel)
__global__ __launch_bounds__(256) void mi_grad_sum_kernel(const double* __restrict__ partials, long long nblocks, int nout, double* __restrict__ out) {
    __shared__ double s[256];
    const int j = blockIdx.x;
    double acc = 0.0;
    for (long long b = threadIdx.x; b < nblocks; b += 256) acc += partials[(size_t)b * nout + j];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[j] = s[0];
}

// minimum, maximum and count of the finite values, per block: part[b] = (min, max), cnt[b]
__global__ __launch_bounds__(256) void finite_range_kernel(const float* __restrict__ a, long long n, float2* __restrict__ part,
                                                           long long* __restrict__ cnt) {
    float mn = INFINITY, mx = -INFINITY;
    long long nv = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float v = a[i];
        if (mvs_ar::finite_f(v)) {
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
            ++nv;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_down(mn, off));
        mx = fmaxf(mx, __shfl_down(mx, off));
        nv += __shfl_down(nv, off);
    }
    __shared__ float smn[4], smx[4];
    __shared__ long long snv[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        smn[wave] = mn;
        smx[wave] = mx;
        snv[wave] = nv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            mn = fminf(mn, smn[w]);
            mx = fmaxf(mx, smx[w]);
            nv += snv[w];
        }
        part[blockIdx.x] = make_float2(mn, mx);
        cnt[blockIdx.x] = nv;
    }
}

// Argument checks and the launch geometry the two metric entries share.  *c is the locked context's; the caller holds its lock.
int mi_setup(MvsContext* c, const char* who, const float* fixed, const float* moving, int32_t mem, int32_t ndim, const int64_t shape[3],
             const double matrix[9], const double offset[3], int32_t n_bins, float f_lo, float f_scale, float m_lo, float m_scale, MiParams* P,
             long long* nblocks) {
    for (int k = 0; k < 3; ++k) {
        P->n[k] = shape[k];
        P->c[k] = (double)(shape[k] - 1) / 2.0;
        P->o[k] = P->c[k] + offset[k];
    }
    for (int k = 0; k < 9; ++k) P->A[k] = matrix[k];
    P->f_lo = f_lo;
    P->f_scale = f_scale;
    P->m_lo = m_lo;
    P->m_scale = m_scale;
    P->B = n_bins;
    P->copies = n_bins <= 16 ? 16 : (n_bins <= 32 ? 4 : 1);
    P->stride = n_bins * n_bins + (P->copies > 1 ? 1 : 0);
    P->nxb = (int)((shape[2] + 63) / 64);
    P->nyc = (int)((shape[1] + MI_WAVES * MI_RUN - 1) / (MI_WAVES * MI_RUN));
    *nblocks = (long long)P->nxb * P->nyc * shape[0];
    if (*nblocks > 0x7fffffffll) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: crop too large", who);
    const long long n = (long long)shape[0] * shape[1] * shape[2];
    float *dF, *dM;
    int rc = mvs_stage_float_volume(c, fixed, mem, n, 4, &dF);
    if (rc) return rc;
    rc = mvs_stage_float_volume(c, moving, mem, n, 5, &dM);
    if (rc) return rc;
    P->fixed = dF;
    P->moving = dM;
    return MVS_OK;
}

int mi_check_args(MvsContext* c0, const char* who, const void* fixed, const void* moving, int32_t mem, int32_t ndim, const int64_t* shape,
                  const double* matrix, const double* offset, int32_t n_bins, const void* out0, const void* out1) {
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", who);
    if (!fixed || !moving || !shape || !matrix || !offset || !out0 || !out1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (mem != MVS_MEM_HOST && mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: bad mem", who);
    if (n_bins < mvs_mi::MIN_BINS || n_bins > mvs_mi::MAX_BINS) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: n_bins must be in 8..64", who);
    for (int k = 0; k < 3; ++k)
        if (shape[k] < 1 || (k < 3 - ndim && shape[k] != 1))
            return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: shape must be positive (and 1 along z in 2D)", who);
    for (int k = 0; k < 3; ++k)
        if (shape[k] > (1 << 24)) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: axis longer than 2^24", who);
    return MVS_OK;
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
    rc = mi_setup(c, who, fixed, moving, mem, ndim, shape, matrix, offset, n_bins, f_lo, f_scale, m_lo, m_scale, &P, &nblocks);
    if (rc) return rc;

    const size_t nent = (size_t)n_bins * n_bins + 1;
    unsigned long long* dhist = (unsigned long long*)mvs_scratch(c, 3, nent * 8);
    if (!dhist) return mvs_alloc_failed(c);
    void *mb_host = nullptr, *mb_dev = nullptr;
    rc = mvs_mailbox(c, nent * 8, &mb_host, &mb_dev);
    if (rc) return rc;
    MVS_HIP_TRY(c, hipMemsetAsync(dhist, 0, nent * 8, c->stream));
    const size_t lds_bytes = (size_t)P.copies * P.stride * 8;
    if (ndim == 3) hipLaunchKernelGGL(mi_hist_kernel<3>, dim3((unsigned)nblocks), dim3(MI_WAVES * 64), lds_bytes, c->stream, P, dhist);
    else hipLaunchKernelGGL(mi_hist_kernel<2>, dim3((unsigned)nblocks), dim3(MI_WAVES * 64), lds_bytes, c->stream, P, dhist);
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
    rc = mi_setup(c, who, fixed, moving, mem, ndim, shape, matrix, offset, n_bins, f_lo, f_scale, m_lo, m_scale, &P, &nblocks);
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
    if (ndim == 3) hipLaunchKernelGGL(mi_grad_kernel<3>, dim3((unsigned)nblocks), dim3(MI_WAVES * 64), 0, c->stream, P, dtab, partials);
    else hipLaunchKernelGGL(mi_grad_kernel<2>, dim3((unsigned)nblocks), dim3(MI_WAVES * 64), 0, c->stream, P, dtab, partials);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(mi_grad_sum_kernel, dim3(nout), dim3(256), 0, c->stream, partials, nblocks, nout, (double*)mb_dev);
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
