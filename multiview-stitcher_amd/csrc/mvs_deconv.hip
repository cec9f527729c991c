// mvs_deconv.hip -- multi-view deconvolution (fusion/mv_deconv.py:251-501 of the reference): Richardson-Lucy with
// per-view compound back-projection kernels, sequential per-view updates, every step on the context's stream.
//
// One iteration, for each view v in order (mv_deconv.py:428-483):
//   forward  blurred = convolve(psi, k1_v, mode="mirror")                     } conv kernel, epilogue writes wr only
//            ratio   = covered ? img / max(blurred, min_value) : 1            }
//            wr      = 1 + w * (ratio - 1)                                     }
//   back     integral = convolve(wr, k2_v, mode="constant", cval=1)           } conv kernel, epilogue updates psi in place
//            psi = clamp(psi * integral [Tikhonov])                            } (it reads psi at its own voxel only)
// Two convolution paths: a general direct one (LDS tile of one input plane per kernel z offset, register-blocked
// outputs, any kernel up to 63 per axis) and a separable one (three 1-D passes) for rank-1 kernels, which the host
// detects.  Boundary rules are scipy.ndimage's: "mirror" reflects about the edge sample (d c b | a b c d | c b a),
// periodically when the kernel reaches further than the axis, a length-1 axis is constant; "constant" reads cval.
// Kernel origin as scipy.ndimage.convolve: out[i] = sum_j k[j] in[i + K//2 - j], even sizes included.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mvs_deconv_plan.h"
#include "mvs_internal.h"
#include "mvs_stack_frame.h"

namespace {

namespace dp = mvs_deconv_plan;
using dp::GX, dp::GY, dp::RX, dp::RY, dp::TX, dp::TY;      // the tile constants the kernels read
static_assert(dp::kOk == MVS_OK && dp::kInvalidArg == MVS_ERR_INVALID_ARG && dp::kUnsupported == MVS_ERR_UNSUPPORTED, "make_plan returns MVS_* codes");

__device__ __forceinline__ int mirror_index(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

// np.nan_to_num of a float32
__device__ __forceinline__ float nan_to_num(float v) {
    if (isnan(v)) return 0.f;
    if (isinf(v)) return v > 0.f ? 3.402823466e38f : -3.402823466e38f;
    return v;
}

struct Epi {
    const float* img;       // view v (NaN = outside)
    const float* w;         // its normalised blending weight
    float* psi;             // the estimate (updated in place by the back epilogue)
    const float* peak;      // max_intensity (device scalar), read when lambda_on
    float minv, l2, lf;     // float32(min_value), float32(2 lambda), float32(lambda)
    int lambda_on;
};

// forward epilogue (mv_deconv.py:442-462): the weighted ratio that the back-projection convolves
__device__ __forceinline__ float epi_forward(const Epi& e, long long i, float blurred) {
    const float img = e.img[i];
    float ratio = 1.f;
    if (!isnan(img)) ratio = nan_to_num(img) / (blurred < e.minv ? e.minv : blurred);
    const float t = e.w[i] * (ratio - 1.f);
    return 1.f + t;
}

// back epilogue (mv_deconv.py:464-483): multiplicative update, optional Tikhonov step, clamp
__device__ __forceinline__ void epi_back(const Epi& e, long long i, float integral) {
    float v = e.psi[i] * integral;
    if (e.lambda_on) {
        const float pk = *e.peak;
        const float x = (v < 0.f ? 0.f : v) / pk;
        const float s = sqrtf(1.f + e.l2 * x) - 1.f;
        v = (s / e.lf) * pk;
    }
    e.psi[i] = isnan(v) ? e.minv : (v < e.minv ? e.minv : v);
}

// psi = max(nansum(nan_to_num(img) * w), min_value) (mv_deconv.py:409-410) + per-block maxima for max_intensity
__global__ void deconv_init_kernel(const float* __restrict__ views, const float* __restrict__ w, int n_views, long long S, float minv,
                                   float* __restrict__ psi, float* __restrict__ block_max) {
    __shared__ float red[256];
    float m = -INFINITY;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (long long)gridDim.x * blockDim.x) {
        float acc = 0.f;
        for (int v = 0; v < n_views; ++v) {
            const float p = nan_to_num(views[v * S + i]) * w[v * S + i];
            if (!isnan(p)) acc = acc + p;
        }
        acc = acc < minv ? minv : acc;
        psi[i] = acc;
        m = fmaxf(m, acc);
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) block_max[blockIdx.x] = red[0];
}

// max_intensity = float(psi.max()), 1 when not positive (mv_deconv.py:412-414)
__global__ void deconv_peak_kernel(const float* __restrict__ block_max, int n, float* __restrict__ peak) {
    __shared__ float red[256];
    float m = -INFINITY;
    for (int i = threadIdx.x; i < n; i += blockDim.x) m = fmaxf(m, block_max[i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *peak = red[0] > 0.f ? red[0] : 1.f;
}

// General direct convolution.  Workgroup = one wave, output tile TX x TY of one z plane.  For each kernel z offset the
// input plane's window (tile + halo, boundary remapped at fill time, so the tap loop has no branches on data) goes to
// LDS; each thread accumulates RY x RX outputs, reading 12 consecutive floats per window row and kernel-x block of 4
// (three ds_read_b128) for up to 4 x 32 FMAs.  `taps` are in correlation order (flipped), x padded with zeros to kxp
// (a multiple of 4); `a*` = K - 1 - K//2 (scipy's origin for odd and even sizes).
// MODE 0: mirror boundary, forward epilogue (writes wr to `out`); MODE 1: constant boundary (cval), back epilogue.
template <int MODE>
__global__ __launch_bounds__(64) void deconv_conv_general(const float* __restrict__ in, float* __restrict__ out,
                                                          const float* __restrict__ taps, int nz, int ny, int nx, int kz, int ky,
                                                          int kxp, int az, int ay, int ax, float cval, Epi e) {
    extern __shared__ float4 lds4[];
    float* tile = reinterpret_cast<float*>(lds4);
    const int LW = TX + kxp;               // window row: TX + kx - 1 needed, padded to a multiple of 4 (values past it meet zero taps)
    const int LH = TY + ky - 1;
    const int t = threadIdx.x, tx = t % GX, ty = t / GX;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, z0 = blockIdx.z;
    // the (at most two) window columns this thread fills, remapped once
    int cx[2];
    bool cin[2];
    for (int k = 0; k < 2; ++k) {
        const int ix = x0 + t + 64 * k - ax;
        cin[k] = ix >= 0 && ix < nx;
        cx[k] = MODE == 0 ? mirror_index(ix, nx) : ix;
    }
    float acc[RY][RX];
#pragma unroll
    for (int r = 0; r < RY; ++r)
#pragma unroll
        for (int c = 0; c < RX; ++c) acc[r][c] = 0.f;

    for (int dz = 0; dz < kz; ++dz) {
        const int iz0 = z0 + dz - az;
        const bool zin = iz0 >= 0 && iz0 < nz;
        const int iz = MODE == 0 ? mirror_index(iz0, nz) : iz0;
        __syncthreads();
        for (int r = 0; r < LH; ++r) {
            const int iy0 = y0 + r - ay;
            const bool yin = zin && iy0 >= 0 && iy0 < ny;
            const int iy = MODE == 0 ? mirror_index(iy0, ny) : iy0;
            const float* row = in + ((long long)iz * ny + iy) * nx;
            for (int k = 0; k < 2; ++k) {
                const int c = t + 64 * k;
                if (c < LW) {
                    float v;
                    if (MODE == 0) v = row[cx[k]];
                    else v = (yin && cin[k]) ? row[cx[k]] : cval;
                    tile[r * LW + c] = v;
                }
            }
        }
        __syncthreads();
        const float* tz = taps + (long long)dz * ky * kxp;
        for (int iy = 0; iy < RY + ky - 1; ++iy) {
            const float* trow = tile + (ty * RY + iy) * LW + tx * RX;
            for (int dx0 = 0; dx0 < kxp; dx0 += 4) {
                const float4 p0 = *reinterpret_cast<const float4*>(trow + dx0);
                const float4 p1 = *reinterpret_cast<const float4*>(trow + dx0 + 4);
                const float4 p2 = *reinterpret_cast<const float4*>(trow + dx0 + 8);
                const float win[12] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w};
#pragma unroll
                for (int ry = 0; ry < RY; ++ry) {
                    const int dy = iy - ry;
                    if (dy < 0 || dy >= ky) continue;
                    const float* w = tz + dy * kxp + dx0;
                    const float w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
#pragma unroll
                    for (int c = 0; c < RX; ++c) {
                        float a = acc[ry][c];
                        a = fmaf(w0, win[c], a);
                        a = fmaf(w1, win[c + 1], a);
                        a = fmaf(w2, win[c + 2], a);
                        a = fmaf(w3, win[c + 3], a);
                        acc[ry][c] = a;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int ry = 0; ry < RY; ++ry) {
        const int y = y0 + ty * RY + ry;
        if (y >= ny) continue;
#pragma unroll
        for (int c = 0; c < RX; ++c) {
            const int x = x0 + tx * RX + c;
            if (x >= nx) continue;
            const long long i = ((long long)z0 * ny + y) * nx + x;
            if (MODE == 0) out[i] = epi_forward(e, i, acc[ry][c]);
            else epi_back(e, i, acc[ry][c]);
        }
    }
}

// One 1-D pass of the separable path along AXIS (0 z, 1 y, 2 x).  MODE 0 mirror, 1 constant (cval: the value the
// extended array has out there after the previous passes).  EPI 0 writes `out`, 1 the forward epilogue, 2 the back one.
template <int AXIS, int MODE, int EPI>
__global__ __launch_bounds__(256) void deconv_pass(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ taps,
                                                   int nz, int ny, int nx, int k, int a, float cval, Epi e) {
    const long long S = (long long)nz * ny * nx;
    const long long step = AXIS == 0 ? (long long)ny * nx : AXIS == 1 ? nx : 1;
    const int n = AXIS == 0 ? nz : AXIS == 1 ? ny : nx;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (long long)gridDim.x * blockDim.x) {
        const int c = AXIS == 0 ? (int)(i / step) : AXIS == 1 ? (int)((i / nx) % ny) : (int)(i % nx);
        const float* base = in + (i - (long long)c * step);
        float acc = 0.f;
        const int lo = c - a;
        if (lo >= 0 && lo + k <= n) {
            const float* p = base + (long long)lo * step;
            for (int j = 0; j < k; ++j) acc = fmaf(taps[j], p[(long long)j * step], acc);
        } else {
            for (int j = 0; j < k; ++j) {
                const int q = lo + j;
                float v;
                if (MODE == 0) v = base[(long long)mirror_index(q, n) * step];
                else v = (q >= 0 && q < n) ? base[(long long)q * step] : cval;
                acc = fmaf(taps[j], v, acc);
            }
        }
        if (EPI == 0) out[i] = acc;
        else if (EPI == 1) out[i] = epi_forward(e, i, acc);
        else epi_back(e, i, acc);
    }
}

// blending weights * ~isnan(view), then normalised by their nansum over the views (0 -> 1), in place
// (fusion/_core.py:1648-1649, weights.py:325-345)
__global__ void deconv_weights_kernel(const float* __restrict__ views, float* __restrict__ w, int n_views, long long S) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (long long)gridDim.x * blockDim.x) {
        float sum = 0.f;
        for (int v = 0; v < n_views; ++v) {
            const float x = w[v * S + i] * (isnan(views[v * S + i]) ? 0.f : 1.f);
            w[v * S + i] = x;
            if (!isnan(x)) sum = sum + x;
        }
        if (sum == 0.f) sum = 1.f;
        for (int v = 0; v < n_views; ++v) w[v * S + i] = w[v * S + i] / sum;
    }
}

// union coverage (any view not NaN) as bytes
__global__ void deconv_coverage_kernel(const float* __restrict__ views, int n_views, long long S, unsigned char* __restrict__ m) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (long long)gridDim.x * blockDim.x) {
        unsigned char any = 0;
        for (int v = 0; v < n_views; ++v) any |= !isnan(views[v * S + i]);
        m[i] = any;
    }
}

// one iteration of scipy's binary_erosion with the cross structure (rank 1 connectivity), border_value=1
__global__ void deconv_erode_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int nz, int ny, int nx, int ndim) {
    const long long S = (long long)nz * ny * nx;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / ((long long)nx * ny));
        unsigned char v = src[i];
        if (v) {
            if (x > 0) v &= src[i - 1];
            if (x + 1 < nx) v &= src[i + 1];
            if (y > 0) v &= src[i - nx];
            if (y + 1 < ny) v &= src[i + nx];
            if (ndim == 3) {
                if (z > 0) v &= src[i - (long long)nx * ny];
                if (z + 1 < nz) v &= src[i + (long long)nx * ny];
            }
        }
        dst[i] = v;
    }
}

// result: psi (0 outside the eroded coverage), trimmed, nan_to_num, cast to the output dtype (C truncation as numpy's astype)
template <typename T>
__global__ void deconv_out_kernel(const float* __restrict__ psi, const unsigned char* __restrict__ mask, int ny, int nx, int oz, int oy, int ox,
                                  int tz, int ty, int tx, T* __restrict__ out) {
    const long long So = (long long)oz * oy * ox;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < So; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % ox), y = (int)((i / ox) % oy), z = (int)(i / ((long long)ox * oy));
        const long long j = ((long long)(z + tz) * ny + (y + ty)) * nx + (x + tx);
        float v = psi[j];
        if (mask && !mask[j]) v = 0.f;
        v = nan_to_num(v);
        if (sizeof(T) == 4) out[i] = (T)v;
        else out[i] = (T)(int)v;
    }
}

const char* const NAME = "mvs_mv_deconv";

// One mvs_mv_deconv call: its arguments, the frame, the plan, the host tables and the carved work area.  The steps below run in the
// order of the entry point.
struct DeconvCall {
    const float* views;
    float* weights;
    int V;
    const int64_t* shape;
    int ndim;
    const float *kernels1, *kernels2;
    const int64_t* ksize;
    const float *sep1, *sep2;
    const mvs_deconv_opts_t* opts;
    void* out;
    int32_t out_mem;
    MvsStackFrame F;
    dp::Plan plan;
    std::vector<float> htaps;
    std::vector<float> sep_cval;        // per view: cval of the y and z passes of the back projection
    float *psi, *wr, *pa, *pb, *bmax, *peak, *dtaps;
    unsigned char *m0, *m1;
    const unsigned char* mask = nullptr;   // the eroded coverage, when there is an erosion
    int pgrid;                          // workgroups of the element-wise kernels over a view
    Epi e{};
};

// argument checks: they need no device
int dc_check(MvsContext* c0, const DeconvCall& K) {
    const mvs_deconv_opts_t* opts = K.opts;
    if (!K.views || !K.weights || !K.shape || !K.kernels1 || !K.kernels2 || !K.ksize || !opts || !K.out)
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: NULL argument");
    if (K.V < 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: n_views must be >= 1");
    if (K.ndim != 2 && K.ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: ndim must be 2 or 3");
    if (int rc = mvs_stack_check_out(c0, NAME, K.out_mem, opts->out_dtype)) return rc;
    if (opts->n_iterations < 0 || opts->erosion_px < 0) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: negative n_iterations / erosion");
    for (int k = 0; k < 3; ++k) {
        if (K.shape[k] < 1 || K.shape[k] > 0x7fffffffLL || K.ksize[k] < 1)
            return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: bad shape / kernel size on axis %d", k);
        if (int rc = mvs_stack_check_trim(c0, NAME, K.shape, opts->trim, k)) return rc;
        if (K.ksize[k] > dp::KMAX)
            return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_mv_deconv: kernel extent %lld on axis %d exceeds the limit of %d", (long long)K.ksize[k], k, dp::KMAX);
    }
    if (K.ndim == 2 && (K.shape[0] != 1 || K.ksize[0] != 1))
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: 2D data has shape[0] == ksize[0] == 1");
    return mvs_stack_check_size(c0, NAME, (long long)K.shape[0] * K.shape[1] * K.shape[2], K.V);
}

// the plan (mvs_deconv_plan.h) and the host tap tables
int dc_plan_and_taps(DeconvCall& K) {
    MvsContext* c = K.F.c;
    const bool separable = K.sep1 && K.sep2 && !c->deconv_general;
    const int rc = dp::make_plan(K.shape, K.ksize, K.V, separable, K.opts->erosion_px > 0, K.opts->trim, K.opts->out_dtype, K.out_mem == MVS_MEM_HOST, &K.plan);
    if (rc) return mvs_fail(c, rc, "mvs_mv_deconv: bad shape / kernel size");      // (dc_check has refused these already)
    dp::make_taps(K.plan, K.V, K.kernels1, K.kernels2, K.sep1, K.sep2, &K.htaps, &K.sep_cval);
    K.pgrid = dp::grid_for(K.plan.S);
    return MVS_OK;
}

// the work area, carved as the plan lays it out
int dc_reserve(DeconvCall& K) {
    const dp::Plan& p = K.plan;
    int rc = K.F.reserve(p.total, p.off_out, K.out, K.out_mem, p.box.out_bytes);
    if (rc) return rc;
    char* W = K.F.W;
    K.psi = (float*)(W + p.off_psi);
    K.wr = (float*)(W + p.off_wr);
    K.pa = (float*)(W + p.off_a);
    K.pb = (float*)(W + p.off_b);
    K.m0 = (unsigned char*)(W + p.off_m0);
    K.m1 = (unsigned char*)(W + p.off_m1);
    K.bmax = (float*)(W + p.off_bm);
    K.peak = (float*)(W + p.off_pk);
    K.dtaps = (float*)(W + p.off_tp);
    return MVS_OK;
}

int dc_upload_taps(DeconvCall& K) {
    MvsContext* c = K.F.c;
    MVS_HIP_TRY(c, hipMemcpyAsync(K.dtaps, K.htaps.data(), K.htaps.size() * 4, hipMemcpyHostToDevice, c->stream));
    return MVS_OK;
}

// the weights (when the caller passed raw ones), the first estimate, its peak (for the Tikhonov step), and the epilogues' constants
int dc_prepare(DeconvCall& K) {
    MvsContext* c = K.F.c;
    const mvs_deconv_opts_t* opts = K.opts;
    const long long S = K.plan.S;
    if (opts->flags & MVS_DECONV_PREPARE_WEIGHTS) {
        hipLaunchKernelGGL(deconv_weights_kernel, dim3(K.pgrid), dim3(256), 0, c->stream, K.views, K.weights, K.V, S);
        MVS_HIP_TRY(c, hipGetLastError());
    }
    const float minv = (float)opts->min_value;
    const int lambda_on = opts->lambda_reg > 0.0;
    hipLaunchKernelGGL(deconv_init_kernel, dim3(dp::kInitBlocks), dim3(256), 0, c->stream, K.views, (const float*)K.weights, K.V, S, minv, K.psi, K.bmax);
    MVS_HIP_TRY(c, hipGetLastError());
    if (lambda_on) {
        hipLaunchKernelGGL(deconv_peak_kernel, dim3(1), dim3(256), 0, c->stream, (const float*)K.bmax, dp::kInitBlocks, K.peak);
        MVS_HIP_TRY(c, hipGetLastError());
    }
    K.e.psi = K.psi;
    K.e.peak = K.peak;
    K.e.minv = minv;
    K.e.l2 = (float)(2.0 * opts->lambda_reg);
    K.e.lf = (float)opts->lambda_reg;
    K.e.lambda_on = lambda_on;
    return MVS_OK;
}

// forward and back projection of view v, general direct path
int dc_view_general(DeconvCall& K, int v) {
    MvsContext* c = K.F.c;
    const dp::Plan& p = K.plan;
    const dim3 ggrid(p.grid_x, p.grid_y, p.grid_z);
    const float* t1 = K.dtaps + (long long)v * p.kvolp;
    const float* t2 = K.dtaps + (long long)(K.V + v) * p.kvolp;
    hipLaunchKernelGGL(deconv_conv_general<0>, ggrid, dim3(64), p.lds_bytes, c->stream, (const float*)K.psi, K.wr, t1, p.nz, p.ny, p.nx, p.kz, p.ky, p.kxp,
                       p.az, p.ay, p.ax, 0.f, K.e);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(deconv_conv_general<1>, ggrid, dim3(64), p.lds_bytes, c->stream, (const float*)K.wr, (float*)nullptr, t2, p.nz, p.ny, p.nx, p.kz,
                       p.ky, p.kxp, p.az, p.ay, p.ax, 1.f, K.e);
    MVS_HIP_TRY(c, hipGetLastError());
    return MVS_OK;
}

// forward and back projection of view v, separable path: x, y, z passes with the epilogue in the z pass
int dc_view_separable(DeconvCall& K, int v) {
    MvsContext* c = K.F.c;
    const dp::Plan& p = K.plan;
    const dim3 grid(K.pgrid), block(256);
    const float* t1 = K.dtaps + (long long)v * p.ksep;
    const float* t2 = K.dtaps + (long long)(K.V + v) * p.ksep;
    const int nz = p.nz, ny = p.ny, nx = p.nx, kz = p.kz, ky = p.ky, kx = p.kx;
    hipLaunchKernelGGL((deconv_pass<2, 0, 0>), grid, block, 0, c->stream, (const float*)K.psi, K.pa, t1 + kz + ky, nz, ny, nx, kx, p.ax, 0.f, K.e);
    hipLaunchKernelGGL((deconv_pass<1, 0, 0>), grid, block, 0, c->stream, (const float*)K.pa, K.pb, t1 + kz, nz, ny, nx, ky, p.ay, 0.f, K.e);
    hipLaunchKernelGGL((deconv_pass<0, 0, 1>), grid, block, 0, c->stream, (const float*)K.pb, K.wr, t1, nz, ny, nx, kz, p.az, 0.f, K.e);
    hipLaunchKernelGGL((deconv_pass<2, 1, 0>), grid, block, 0, c->stream, (const float*)K.wr, K.pa, t2 + kz + ky, nz, ny, nx, kx, p.ax, 1.f, K.e);
    hipLaunchKernelGGL((deconv_pass<1, 1, 0>), grid, block, 0, c->stream, (const float*)K.pa, K.pb, t2 + kz, nz, ny, nx, ky, p.ay, K.sep_cval[2 * v], K.e);
    hipLaunchKernelGGL((deconv_pass<0, 1, 2>), grid, block, 0, c->stream, (const float*)K.pb, (float*)nullptr, t2, nz, ny, nx, kz, p.az,
                       K.sep_cval[2 * v + 1], K.e);
    MVS_HIP_TRY(c, hipGetLastError());
    return MVS_OK;
}

// one view's update of the estimate: the epilogues read this view and its weights
int dc_view(DeconvCall& K, int v) {
    K.e.img = K.views + v * K.plan.S;
    K.e.w = K.weights + v * K.plan.S;
    return K.plan.separable ? dc_view_separable(K, v) : dc_view_general(K, v);
}

// the union coverage eroded erosion_px times (mv_deconv.py:485-499)
int dc_erosion_mask(DeconvCall& K) {
    MvsContext* c = K.F.c;
    const dp::Plan& p = K.plan;
    if (K.opts->erosion_px <= 0) return MVS_OK;
    hipLaunchKernelGGL(deconv_coverage_kernel, dim3(K.pgrid), dim3(256), 0, c->stream, K.views, K.V, p.S, K.m0);
    unsigned char *src = K.m0, *dst = K.m1;
    for (int k = 0; k < K.opts->erosion_px; ++k) {
        hipLaunchKernelGGL(deconv_erode_kernel, dim3(K.pgrid), dim3(256), 0, c->stream, (const unsigned char*)src, dst, p.nz, p.ny, p.nx, K.ndim);
        std::swap(src, dst);
    }
    MVS_HIP_TRY(c, hipGetLastError());
    K.mask = src;
    return MVS_OK;
}

// the estimate, masked, trimmed and cast, where the frame wants the result
int dc_write_result(DeconvCall& K) {
    MvsContext* c = K.F.c;
    const dp::Plan& p = K.plan;
    const int oz = (int)p.box.oz, oy = (int)p.box.oy, ox = (int)p.box.ox;
    const int ogrid = dp::grid_for(p.box.oz * p.box.oy * p.box.ox);
    const int t0 = (int)K.opts->trim[0], t1 = (int)K.opts->trim[1], t2 = (int)K.opts->trim[2];
    mvs_dispatch_dtype(K.opts->out_dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(deconv_out_kernel<T>, dim3(ogrid), dim3(256), 0, c->stream, (const float*)K.psi, K.mask, p.ny, p.nx, oz, oy, ox, t0, t1, t2,
                           (T*)K.F.dout);
    });
    MVS_HIP_TRY(c, hipGetLastError());
    return MVS_OK;
}

}  // namespace

extern "C" int mvs_mv_deconv(int device, const float* views, float* weights, int32_t n_views, const int64_t shape[3], int32_t ndim,
                             const float* kernels1, const float* kernels2, const int64_t ksize[3], const float* sep1, const float* sep2,
                             const mvs_deconv_opts_t* opts, void* out, int32_t out_mem) {
    DeconvCall K{views, weights, n_views, shape, ndim, kernels1, kernels2, ksize, sep1, sep2, opts, out, out_mem};
    int rc = dc_check(mvs_ctx(device), K);
    if (!rc) rc = K.F.begin(device);
    if (!rc) rc = dc_plan_and_taps(K);
    if (!rc) rc = dc_reserve(K);
    if (!rc) rc = dc_upload_taps(K);
    if (!rc) rc = dc_prepare(K);
    for (int it = 0; !rc && it < opts->n_iterations; ++it)
        for (int v = 0; !rc && v < n_views; ++v) rc = dc_view(K, v);
    if (!rc) rc = dc_erosion_mask(K);
    if (!rc) rc = dc_write_result(K);
    return rc ? rc : K.F.finish();
}
