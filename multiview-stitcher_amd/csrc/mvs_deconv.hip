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

#include "mvs_internal.h"

namespace {

constexpr int GX = 8, GY = 8;       // threads of a general-path workgroup (one wave)
constexpr int RX = 8, RY = 4;       // outputs per thread along x / y
constexpr int TX = GX * RX, TY = GY * RY;   // output tile 64 x 32
constexpr int KMAX = 63;            // largest kernel extent per axis of the general path

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

int grid_for(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 256 * 32)); }

}  // namespace

extern "C" int mvs_mv_deconv(int device, const float* views, float* weights, int32_t n_views, const int64_t shape[3], int32_t ndim,
                             const float* kernels1, const float* kernels2, const int64_t ksize[3], const float* sep1, const float* sep2,
                             const mvs_deconv_opts_t* opts, void* out, int32_t out_mem) {
    MvsContext* c0 = mvs_ctx(device);
    // argument checks first: they need no device
    if (!views || !weights || !shape || !kernels1 || !kernels2 || !ksize || !opts || !out)
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: NULL argument");
    if (n_views < 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: n_views must be >= 1");
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: ndim must be 2 or 3");
    if (out_mem != MVS_MEM_HOST && out_mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: bad out_mem");
    if (opts->out_dtype != MVS_U8 && opts->out_dtype != MVS_U16 && opts->out_dtype != MVS_F32)
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: bad out_dtype");
    if (opts->n_iterations < 0 || opts->erosion_px < 0) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: negative n_iterations / erosion");
    for (int k = 0; k < 3; ++k) {
        if (shape[k] < 1 || shape[k] > 0x7fffffffLL || ksize[k] < 1)
            return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: bad shape / kernel size on axis %d", k);
        if (opts->trim[k] < 0 || 2 * opts->trim[k] >= shape[k])
            return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: trim on axis %d leaves nothing", k);
        if (ksize[k] > KMAX)
            return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_mv_deconv: kernel extent %lld on axis %d exceeds the limit of %d", (long long)ksize[k], k, KMAX);
    }
    if (ndim == 2 && (shape[0] != 1 || ksize[0] != 1)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: 2D data has shape[0] == ksize[0] == 1");
    if ((long long)shape[0] * shape[1] * shape[2] * n_views > (1LL << 40)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_mv_deconv: too large");

    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));
    const int nz = (int)shape[0], ny = (int)shape[1], nx = (int)shape[2];
    const int kz = (int)ksize[0], ky = (int)ksize[1], kx = (int)ksize[2];
    const long long S = (long long)nz * ny * nx;
    const int V = n_views;
    const bool separable = sep1 && sep2 && !c->deconv_general;
    const int kxp = (kx + 3) & ~3;
    const int az = kz - 1 - kz / 2, ay = ky - 1 - ky / 2, ax = kx - 1 - kx / 2;

    // host tap tables in correlation order: general [set][v][kz][ky][kxp] (x zero-padded), separable [set][v][kz + ky + kx]
    const long long kvol = (long long)kz * ky * kx, kvolp = (long long)kz * ky * kxp, ksep = kz + ky + kx;
    std::vector<float> htaps;
    std::vector<float> sep_cval;          // per view: cval of the y and z passes of the back projection
    if (separable) {
        htaps.resize(2 * V * ksep);
        sep_cval.resize(2 * (size_t)V);
        for (int s = 0; s < 2; ++s)
            for (int v = 0; v < V; ++v) {
                const float* src = (s ? sep2 : sep1) + v * ksep;
                float* dst = htaps.data() + (s * V + v) * ksep;
                const int len[3] = {kz, ky, kx};
                int off = 0;
                for (int ax_ = 0; ax_ < 3; ++ax_) {
                    for (int j = 0; j < len[ax_]; ++j) dst[off + j] = src[off + len[ax_] - 1 - j];
                    off += len[ax_];
                }
                if (s == 1) {
                    double sx = 0.0, sy = 0.0;
                    for (int j = 0; j < kx; ++j) sx += src[kz + ky + j];
                    for (int j = 0; j < ky; ++j) sy += src[kz + j];
                    sep_cval[2 * v] = (float)sx;
                    sep_cval[2 * v + 1] = (float)(sx * sy);
                }
            }
    } else {
        htaps.assign(2 * V * kvolp, 0.f);
        for (int s = 0; s < 2; ++s)
            for (int v = 0; v < V; ++v) {
                const float* src = (s ? kernels2 : kernels1) + v * kvol;
                float* dst = htaps.data() + (s * V + v) * kvolp;
                for (int z = 0; z < kz; ++z)
                    for (int y = 0; y < ky; ++y)
                        for (int x = 0; x < kx; ++x)
                            dst[((long long)z * ky + y) * kxp + x] = src[((long long)(kz - 1 - z) * ky + (ky - 1 - y)) * kx + (kx - 1 - x)];
            }
    }

    // device work area: psi | wr | two pass buffers (separable) | two masks (erosion) | block maxima | peak | taps
    const int init_blocks = 1024;
    const size_t fS = (size_t)S * 4;
    size_t off_psi = 0, off_wr = off_psi + fS, off_a = off_wr + fS, off_b = off_a + (separable ? fS : 0);
    size_t off_m0 = off_b + (separable ? fS : 0);
    size_t off_m1 = off_m0 + (opts->erosion_px > 0 ? align_up((size_t)S) : 0);
    size_t off_bm = off_m1 + (opts->erosion_px > 0 ? align_up((size_t)S) : 0);
    size_t off_pk = off_bm + init_blocks * 4;
    size_t off_tp = off_pk + 256;
    size_t off_out = off_tp + align_up(htaps.size() * 4);
    const size_t out_elem = mvs_dtype_size(opts->out_dtype);
    const long long oz = nz - 2 * opts->trim[0], oy = ny - 2 * opts->trim[1], ox = nx - 2 * opts->trim[2];
    const size_t out_bytes = (size_t)(oz * oy * ox) * out_elem;
    size_t total = off_out + (out_mem == MVS_MEM_HOST ? out_bytes : 0);
    MvsWorkArea work(c);
    rc = work.alloc(total);
    if (rc) return rc;
    char* W = (char*)work.ptr;
    float* psi = (float*)(W + off_psi);
    float* wr = (float*)(W + off_wr);
    float* pa = (float*)(W + off_a);
    float* pb = (float*)(W + off_b);
    unsigned char* m0 = (unsigned char*)(W + off_m0);
    unsigned char* m1 = (unsigned char*)(W + off_m1);
    float* bmax = (float*)(W + off_bm);
    float* peak = (float*)(W + off_pk);
    float* dtaps = (float*)(W + off_tp);
    void* dout = out_mem == MVS_MEM_HOST ? (void*)(W + off_out) : out;

    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    MVS_HIP_TRY(c, hipMemcpyAsync(dtaps, htaps.data(), htaps.size() * 4, hipMemcpyHostToDevice, c->stream));
    const int pgrid = grid_for(S);
    if (opts->flags & MVS_DECONV_PREPARE_WEIGHTS) {
        hipLaunchKernelGGL(deconv_weights_kernel, dim3(pgrid), dim3(256), 0, c->stream, views, (float*)weights, V, S);
        MVS_HIP_TRY(c, hipGetLastError());
    }
    const float minv = (float)opts->min_value;
    const int lambda_on = opts->lambda_reg > 0.0;
    hipLaunchKernelGGL(deconv_init_kernel, dim3(init_blocks), dim3(256), 0, c->stream, views, weights, V, S, minv, psi, bmax);
    MVS_HIP_TRY(c, hipGetLastError());
    if (lambda_on) {
        hipLaunchKernelGGL(deconv_peak_kernel, dim3(1), dim3(256), 0, c->stream, (const float*)bmax, init_blocks, peak);
        MVS_HIP_TRY(c, hipGetLastError());
    }
    Epi e{};
    e.psi = psi;
    e.peak = peak;
    e.minv = minv;
    e.l2 = (float)(2.0 * opts->lambda_reg);
    e.lf = (float)opts->lambda_reg;
    e.lambda_on = lambda_on;
    const dim3 ggrid((nx + TX - 1) / TX, (ny + TY - 1) / TY, nz);
    const size_t glds = (size_t)(TY + ky - 1) * (TX + kxp) * 4;
    for (int it = 0; it < opts->n_iterations; ++it) {
        for (int v = 0; v < V; ++v) {
            e.img = views + v * S;
            e.w = weights + v * S;
            if (!separable) {
                const float* t1 = dtaps + (long long)v * kvolp;
                const float* t2 = dtaps + (long long)(V + v) * kvolp;
                hipLaunchKernelGGL(deconv_conv_general<0>, ggrid, dim3(64), glds, c->stream, (const float*)psi, wr, t1, nz, ny, nx, kz, ky, kxp,
                                   az, ay, ax, 0.f, e);
                MVS_HIP_TRY(c, hipGetLastError());
                hipLaunchKernelGGL(deconv_conv_general<1>, ggrid, dim3(64), glds, c->stream, (const float*)wr, (float*)nullptr, t2, nz, ny, nx,
                                   kz, ky, kxp, az, ay, ax, 1.f, e);
                MVS_HIP_TRY(c, hipGetLastError());
            } else {
                const float* t1 = dtaps + (long long)v * ksep;
                const float* t2 = dtaps + (long long)(V + v) * ksep;
                hipLaunchKernelGGL((deconv_pass<2, 0, 0>), dim3(pgrid), dim3(256), 0, c->stream, (const float*)psi, pa, t1 + kz + ky, nz, ny, nx, kx, ax, 0.f, e);
                hipLaunchKernelGGL((deconv_pass<1, 0, 0>), dim3(pgrid), dim3(256), 0, c->stream, (const float*)pa, pb, t1 + kz, nz, ny, nx, ky, ay, 0.f, e);
                hipLaunchKernelGGL((deconv_pass<0, 0, 1>), dim3(pgrid), dim3(256), 0, c->stream, (const float*)pb, wr, t1, nz, ny, nx, kz, az, 0.f, e);
                hipLaunchKernelGGL((deconv_pass<2, 1, 0>), dim3(pgrid), dim3(256), 0, c->stream, (const float*)wr, pa, t2 + kz + ky, nz, ny, nx, kx, ax, 1.f, e);
                hipLaunchKernelGGL((deconv_pass<1, 1, 0>), dim3(pgrid), dim3(256), 0, c->stream, (const float*)pa, pb, t2 + kz, nz, ny, nx, ky, ay, sep_cval[2 * v], e);
                hipLaunchKernelGGL((deconv_pass<0, 1, 2>), dim3(pgrid), dim3(256), 0, c->stream, (const float*)pb, (float*)nullptr, t2, nz, ny, nx, kz, az,
                                   sep_cval[2 * v + 1], e);
                MVS_HIP_TRY(c, hipGetLastError());
            }
        }
    }
    const unsigned char* mask = nullptr;
    if (opts->erosion_px > 0) {     // mv_deconv.py:485-499
        hipLaunchKernelGGL(deconv_coverage_kernel, dim3(pgrid), dim3(256), 0, c->stream, views, V, S, m0);
        unsigned char *src = m0, *dst = m1;
        for (int k = 0; k < opts->erosion_px; ++k) {
            hipLaunchKernelGGL(deconv_erode_kernel, dim3(pgrid), dim3(256), 0, c->stream, (const unsigned char*)src, dst, nz, ny, nx, (int)ndim);
            std::swap(src, dst);
        }
        MVS_HIP_TRY(c, hipGetLastError());
        mask = src;
    }
    const int ogrid = grid_for(oz * oy * ox);
    const int t0 = (int)opts->trim[0], t1 = (int)opts->trim[1], t2 = (int)opts->trim[2];
    if (opts->out_dtype == MVS_F32)
        hipLaunchKernelGGL(deconv_out_kernel<float>, dim3(ogrid), dim3(256), 0, c->stream, (const float*)psi, mask, ny, nx, (int)oz, (int)oy, (int)ox,
                           t0, t1, t2, (float*)dout);
    else if (opts->out_dtype == MVS_U16)
        hipLaunchKernelGGL(deconv_out_kernel<unsigned short>, dim3(ogrid), dim3(256), 0, c->stream, (const float*)psi, mask, ny, nx, (int)oz, (int)oy,
                           (int)ox, t0, t1, t2, (unsigned short*)dout);
    else
        hipLaunchKernelGGL(deconv_out_kernel<unsigned char>, dim3(ogrid), dim3(256), 0, c->stream, (const float*)psi, mask, ny, nx, (int)oz, (int)oy,
                           (int)ox, t0, t1, t2, (unsigned char*)dout);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    if (out_mem == MVS_MEM_HOST) {
        MVS_HIP_TRY(c, hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, c->stream));
        MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    // the work area goes back to the pool; the pool hands it out again only to work later on this stream
    return work.release();
}
