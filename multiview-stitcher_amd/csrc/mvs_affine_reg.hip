// mvs_affine_reg.hip -- normal equations of the Gauss-Newton intensity registration (mvs_affine_normal_eq, include/mvs_hip.h).
//
// One launch walks every voxel of the fixed crop, warps it into the moving crop by the centred pose and sums J^T J, J^T r, the
// squared residual, the valid count and the intensity moments.  The walk (block geometry, warp, taps, validity) is
// mvs_affine_walk_dev.h, shared with the kernels of mvs_affine_mi.hip; the per-sample arithmetic is mvs_affine_reg_dev.h.
//
// Accumulator layout.  J = gain * g (x) [x - c, 1], so J^T J = sum (g g^T) (x) (x~ x~^T): ndim (ndim + 1) / 2 gradient pairs times
// (ndim + 1)(ndim + 2) / 2 coordinate monomials (60 distinct sums in 3D, 18 in 2D).  A block is 4 waves over 64 consecutive x
// columns; a thread keeps its x (and the block its z) and walks mvs_aw::RUN rows, so only y changes along its run and it carries the
// moments  sum g_a g_b y^k (k = 0..2),  sum r g_a y^k (k = 0..1)  and the 7 scalar sums in float32: 31 accumulators in 3D, 18 in
// 2D.  At the end of the run they are multiplied by the powers of the thread's x in double, summed over the wave by shuffles and
// over the block through LDS in double, expanded by the block's z, and written as one row of per-block partials.  A second
// launch adds the rows in a fixed order (no atomics): the same input gives the same bits.
#include "mvs_affine_walk.h"

namespace {

using mvs_aw::WAVES;
using mvs_aw::wave_sum;

template <int ND>
struct ArLayout {
    static constexpr int NP = ND * (ND + 1) / 2;            // gradient pairs (a <= b)
    static constexpr int NM = (ND + 1) * (ND + 2) / 2;      // monomials x~_j x~_m (j <= m), x~ = (x - c, 1)
    static constexpr int NV = NP * 6 + ND * 3 + 7;          // values a thread hands to the block reduction
    static constexpr int NOUT = NP * NM + ND * (ND + 1) + 7;   // distinct sums of one block
};

struct ArParams : mvs_aw::Walk {
    float gain, bias;
};

template <int ND>
__global__ __launch_bounds__(WAVES * 64) void affine_neq_kernel(ArParams P, double* __restrict__ partials) {
    using L = ArLayout<ND>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const mvs_aw::BlockPos bp = mvs_aw::block_pos(P, blockIdx.x);
    const long long x = (long long)bp.xb * 64 + lane;
    const double dxd = (double)x - P.c[2];
    const double dzd = ND == 3 ? (double)bp.z - P.c[0] : 0.0;

    float S0[L::NP], S1[L::NP], S2[L::NP], R0[ND], R1[ND];
#pragma unroll
    for (int p = 0; p < L::NP; ++p) S0[p] = S1[p] = S2[p] = 0.f;
#pragma unroll
    for (int k = 0; k < ND; ++k) R0[k] = R1[k] = 0.f;
    float s_r2 = 0.f, s_n = 0.f, s_v = 0.f, s_f = 0.f, s_vf = 0.f, s_v2 = 0.f, s_f2 = 0.f;

    mvs_aw::walk_run<ND>(P, bp.z, bp.yc, wave, x, dzd, dxd, [&](float fv, float v, const float* g, float dy) {
        const float r = mvs_ar::residual(P.gain, P.bias, v, fv);
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
    });

    // per thread: the moments times the powers of its x, in the order (yy, yx, y1, xx, x1, 11) per pair and (y, x, 1) per gradient
    __shared__ double red[WAVES][L::NV];
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
    const char* who = "mvs_affine_normal_eq";
    int rc = affine_check_args(mvs_ctx(device), who, fixed, moving, mem, ndim, shape, matrix, offset, out, out);
    if (rc) return rc;
    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    ArParams P;
    long long nblocks;
    rc = affine_walk_setup(c, who, fixed, moving, mem, shape, matrix, offset, &P, &nblocks);
    if (rc) return rc;
    P.gain = (float)gain;
    P.bias = (float)bias;
    const int nout = ndim == 3 ? ArLayout<3>::NOUT : ArLayout<2>::NOUT;
    double* partials = (double*)mvs_scratch(c, 3, (size_t)nblocks * nout * sizeof(double));
    if (!partials) return mvs_alloc_failed(c);
    void *mb_host = nullptr, *mb_dev = nullptr;
    rc = mvs_mailbox(c, (size_t)nout * sizeof(double), &mb_host, &mb_dev);
    if (rc) return rc;

    if (ndim == 3) hipLaunchKernelGGL(affine_neq_kernel<3>, dim3((unsigned)nblocks), dim3(WAVES * 64), 0, c->stream, P, partials);
    else hipLaunchKernelGGL(affine_neq_kernel<2>, dim3((unsigned)nblocks), dim3(WAVES * 64), 0, c->stream, P, partials);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(mvs_aw::rows_sum_kernel, dim3(nout), dim3(256), 0, c->stream, partials, nblocks, nout, (double*)mb_dev);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (ndim == 3) scatter_result<3>((const double*)mb_host, out);
    else scatter_result<2>((const double*)mb_host, out);
    return MVS_OK;
}
