// mvs_affine_reg.hip -- normal equations of the Gauss-Newton intensity registration (mvs_affine_normal_eq, include/mvs_hip.h).
//
// One launch walks every voxel of the fixed crop, warps it into the moving crop by the centred pose and sums J^T J, J^T r, the
// squared residual, the valid count and the intensity moments.  The per-sample arithmetic is mvs_affine_reg_dev.h.
//
// Accumulator layout.  J = gain * g (x) [x - c, 1], so J^T J = sum (g g^T) (x) (x~ x~^T): ndim (ndim + 1) / 2 gradient pairs times
// (ndim + 1)(ndim + 2) / 2 coordinate monomials (60 distinct sums in 3D, 18 in 2D).  A block is 4 waves over 64 consecutive x
// columns; a thread keeps its x (and the block its z) and walks AR_RUN rows, so only y changes along its run and it carries the
// moments  sum g_a g_b y^k (k = 0..2),  sum r g_a y^k (k = 0..1)  and the 7 scalar sums in float32: 31 accumulators in 3D, 18 in
// 2D.  At the end of the run they are multiplied by the powers of the thread's x in double, summed over the wave by shuffles and
// over the block through LDS in double, expanded by the block's z, and written as one row of per-block partials.  A second
// launch adds the rows in a fixed order (no atomics): the same input gives the same bits.
#include "mvs_affine_reg_dev.h"
#include "mvs_internal.h"

int mvs_stage_float_volume(MvsContext* c, const float* src, int32_t mem, long long n, int slot, float** dptr);   // mvs_reg.hip

namespace {

constexpr int AR_WAVES = 4;      // waves of a block: wave w takes rows y0 + w, y0 + w + 4, ...
constexpr int AR_RUN = 32;       // rows per thread: the length of a float32 run sum

template <int ND>
struct ArLayout {
    static constexpr int NP = ND * (ND + 1) / 2;            // gradient pairs (a <= b)
    static constexpr int NM = (ND + 1) * (ND + 2) / 2;      // monomials x~_j x~_m (j <= m), x~ = (x - c, 1)
    static constexpr int NV = NP * 6 + ND * 3 + 7;          // values a thread hands to the block reduction
    static constexpr int NOUT = NP * NM + ND * (ND + 1) + 7;   // distinct sums of one block
};

struct ArParams {
    const float* fixed;
    const float* moving;
    long long n[3];      // z, y, x (z = 1 in 2D)
    double A[9];         // 3x3, row-major (z, y, x); 2D uses the lower right 2x2
    double o[3];         // c + t
    double c[3];
    float gain, bias;
    int nxb, nyc;        // blocks along x and y
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

template <int ND>
__global__ __launch_bounds__(AR_WAVES * 64) void affine_neq_kernel(ArParams P, double* __restrict__ partials) {
    using L = ArLayout<ND>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long b = blockIdx.x;
    const int xb = (int)(b % P.nxb);
    b /= P.nxb;
    const int yc = (int)(b % P.nyc);
    const long long z = b / P.nyc;
    const long long ny = P.n[1], nx = P.n[2];
    const long long x = (long long)xb * 64 + lane;
    const double dxd = (double)x - P.c[2];
    const double dzd = ND == 3 ? (double)z - P.c[0] : 0.0;

    float S0[L::NP], S1[L::NP], S2[L::NP], R0[ND], R1[ND];
#pragma unroll
    for (int p = 0; p < L::NP; ++p) S0[p] = S1[p] = S2[p] = 0.f;
#pragma unroll
    for (int k = 0; k < ND; ++k) R0[k] = R1[k] = 0.f;
    float s_r2 = 0.f, s_n = 0.f, s_v = 0.f, s_f = 0.f, s_vf = 0.f, s_v2 = 0.f, s_f2 = 0.f;

    if (x < nx) {
        // the products of the coordinate that do not change along the run (each rounds on its own, as in coord2 / coord3)
        double az[3], ax[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            az[k] = P.A[k * 3 + 0] * dzd;
            ax[k] = P.A[k * 3 + 2] * dxd;
        }
        const long long y0 = (long long)yc * (AR_WAVES * AR_RUN) + wave;
        const float* __restrict__ frow = P.fixed + (z * ny + y0) * nx + x;
        for (int i = 0; i < AR_RUN; ++i, frow += AR_WAVES * nx) {
            const long long y = y0 + (long long)i * AR_WAVES;
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
            const float r = mvs_ar::residual(P.gain, P.bias, v, fv);
            const float dy = (float)dyd;
            float gg[ND];
#pragma unroll
            for (int k = 0; k < ND; ++k) gg[k] = P.gain * g[k];
            int p = 0;
#pragma unroll
            for (int a = 0; a < ND; ++a) {
#pragma unroll
                for (int bb = a; bb < ND; ++bb, ++p) {
                    const float q = gg[a] * gg[bb];
                    const float qy = q * dy;
                    S0[p] += q;
                    S1[p] += qy;
                    S2[p] = fmaf(qy, dy, S2[p]);
                }
                const float rg = r * gg[a];
                R0[a] += rg;
                R1[a] = fmaf(rg, dy, R1[a]);
            }
            s_r2 = fmaf(r, r, s_r2);
            s_n += 1.f;
            s_v += v;
            s_f += fv;
            s_vf = fmaf(v, fv, s_vf);
            s_v2 = fmaf(v, v, s_v2);
            s_f2 = fmaf(fv, fv, s_f2);
        }
    }

    // per thread: the moments times the powers of its x, in the order (yy, yx, y1, xx, x1, 11) per pair and (y, x, 1) per gradient
    __shared__ double red[AR_WAVES][L::NV];
    const double dx2 = dxd * dxd;
    int iv = 0;
    auto put = [&](double val) {
        val = wave_sum(val);
        if (lane == 0) red[wave][iv] = val;
        ++iv;
    };
#pragma unroll
    for (int p = 0; p < L::NP; ++p) {
        put((double)S2[p]);
        put(dxd * (double)S1[p]);
        put((double)S1[p]);
        put(dx2 * (double)S0[p]);
        put(dxd * (double)S0[p]);
        put((double)S0[p]);
    }
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        put((double)R1[k]);
        put(dxd * (double)R0[k]);
        put((double)R0[k]);
    }
    put((double)s_r2);
    put((double)s_n);
    put((double)s_v);
    put((double)s_f);
    put((double)s_vf);
    put((double)s_v2);
    put((double)s_f2);
    __syncthreads();

    const int j = threadIdx.x;
    if (j < L::NOUT) {
        auto tot = [&](int i) { return ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i]; };
        double val;
        if (j < L::NP * L::NM) {
            const int p = j / L::NM, m = j % L::NM;
            if (ND == 2) val = tot(p * 6 + m);
            else if (m == 0) val = (dzd * dzd) * tot(p * 6 + 5);       // zz
            else if (m == 1) val = dzd * tot(p * 6 + 2);               // zy
            else if (m == 2) val = dzd * tot(p * 6 + 4);               // zx
            else if (m == 3) val = dzd * tot(p * 6 + 5);               // z1
            else val = tot(p * 6 + m - 4);
        } else if (j < L::NP * L::NM + ND * (ND + 1)) {
            const int q = j - L::NP * L::NM, k = q / (ND + 1), m = q % (ND + 1);
            const int base = L::NP * 6 + k * 3;
            if (ND == 2) val = tot(base + m);
            else val = m == 0 ? dzd * tot(base + 2) : tot(base + m - 1);
        } else {
            val = tot(L::NP * 6 + ND * 3 + (j - L::NP * L::NM - ND * (ND + 1)));
        }
        partials[(size_t)blockIdx.x * L::NOUT + j] = val;
    }
}

// out[j] = sum over the blocks of partials[b][j]: thread t takes b = t, t + 256, ... in order, then a fixed tree in LDS
__global__ __launch_bounds__(256) void affine_neq_sum_kernel(const double* __restrict__ partials, long long nblocks, int nout,
                                                             double* __restrict__ out) {
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

inline int tri_index(int a, int b, int n) {      // index of (a <= b) in the row-major upper triangle of an n x n matrix
    return a * n - a * (a - 1) / 2 + (b - a);
}

template <int ND>
void scatter_result(const double* sums, double* out) {
    using L = ArLayout<ND>;
    constexpr int NPAR = ND * (ND + 1);
    for (int i = 0; i < MVS_AFFINE_NEQ_LEN; ++i) out[i] = 0.0;
    for (int k = 0; k < ND; ++k)
        for (int j = 0; j <= ND; ++j)
            for (int l = 0; l < ND; ++l)
                for (int m = 0; m <= ND; ++m) {
                    const int p = tri_index(k < l ? k : l, k < l ? l : k, ND);
                    const int mono = tri_index(j < m ? j : m, j < m ? m : j, ND + 1);
                    out[(k * (ND + 1) + j) * NPAR + l * (ND + 1) + m] = sums[p * L::NM + mono];
                }
    for (int i = 0; i < NPAR + 7; ++i) out[NPAR * NPAR + i] = sums[L::NP * L::NM + i];
}

}  // namespace

extern "C" int mvs_affine_normal_eq(int device, const float* fixed, const float* moving, int32_t mem, int32_t ndim, const int64_t shape[3],
                                    const double matrix[9], const double offset[3], double gain, double bias, double* out) {
    MvsContext* c0 = mvs_ctx(device);
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_affine_normal_eq: ndim must be 2 or 3");
    if (!fixed || !moving || !shape || !matrix || !offset || !out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_affine_normal_eq: NULL argument");
    if (mem != MVS_MEM_HOST && mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_affine_normal_eq: bad mem");
    for (int k = 0; k < 3; ++k)
        if (shape[k] < 1 || (k < 3 - ndim && shape[k] != 1))
            return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_affine_normal_eq: shape must be positive (and 1 along z in 2D)");
    for (int k = 0; k < 3; ++k)
        if (shape[k] > (1 << 24)) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_affine_normal_eq: axis longer than 2^24");
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    ArParams P;
    for (int k = 0; k < 3; ++k) {
        P.n[k] = shape[k];
        P.c[k] = (double)(shape[k] - 1) / 2.0;
        P.o[k] = P.c[k] + offset[k];
    }
    for (int k = 0; k < 9; ++k) P.A[k] = matrix[k];
    P.gain = (float)gain;
    P.bias = (float)bias;
    P.nxb = (int)((shape[2] + 63) / 64);
    P.nyc = (int)((shape[1] + AR_WAVES * AR_RUN - 1) / (AR_WAVES * AR_RUN));
    const long long nblocks = (long long)P.nxb * P.nyc * shape[0];
    if (nblocks > 0x7fffffffll) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "mvs_affine_normal_eq: crop too large");
    const int nout = ndim == 3 ? ArLayout<3>::NOUT : ArLayout<2>::NOUT;

    const long long n = (long long)shape[0] * shape[1] * shape[2];
    float *dF, *dM;
    rc = mvs_stage_float_volume(c, fixed, mem, n, 4, &dF);
    if (rc) return rc;
    rc = mvs_stage_float_volume(c, moving, mem, n, 5, &dM);
    if (rc) return rc;
    P.fixed = dF;
    P.moving = dM;
    double* partials = (double*)mvs_scratch(c, 3, (size_t)nblocks * nout * sizeof(double));
    if (!partials) return mvs_alloc_failed(c);
    void *mb_host = nullptr, *mb_dev = nullptr;
    rc = mvs_mailbox(c, (size_t)nout * sizeof(double), &mb_host, &mb_dev);
    if (rc) return rc;

    if (ndim == 3) hipLaunchKernelGGL(affine_neq_kernel<3>, dim3((unsigned)nblocks), dim3(AR_WAVES * 64), 0, c->stream, P, partials);
    else hipLaunchKernelGGL(affine_neq_kernel<2>, dim3((unsigned)nblocks), dim3(AR_WAVES * 64), 0, c->stream, P, partials);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(affine_neq_sum_kernel, dim3(nout), dim3(256), 0, c->stream, partials, nblocks, nout, (double*)mb_dev);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (ndim == 3) scatter_result<3>((const double*)mb_host, out);
    else scatter_result<2>((const double*)mb_host, out);
    return MVS_OK;
}
