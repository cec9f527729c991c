// mvs_reg.hip -- pairwise phase correlation on the GPU (gfx950).
//
// mvs_phasecorr == skimage.registration.phase_cross_correlation(a, b, normalization=None|"phase",
// upsample_factor=u, disambiguate=False)[0] as called from the reference's
// registration.phase_correlation_registration (src/multiview_stitcher/registration.py:422-431):
//   F = fftn(a), G = fftn(b)                         (complex64, mvs_fft.hip; both from ONE transform of a + i b)
//   P = F * conj(G);  "phase": P /= max(|P|, 100 eps)
//   cc = ifftn(P);  integer peak = argmax |cc|  (lowest flat index wins ties, like np.argmax)
//   wrap to signed shift, then the matrix-multiply upsampled DFT around round(shift*u)/u
// mvs_rescale_intensity == skimage.exposure.rescale_intensity(im, in_range=(nanmin, nanmax),
// out_range=(0,1)) (registration.py:381-389).
#include "mvs_fft_dev.h"

#include <rocprim/warp/warp_reduce.hpp>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

namespace {

// Both images are real, so ONE complex transform carries both spectra: Z = fft(a + i b), and with Zm = Z(-k)
//   A(k) = (Z + conj Zm) / 2,   B(k) = (Z - conj Zm) / (2 i).
__global__ void pack_pair_kernel(const float* __restrict__ a, const float* __restrict__ b, float2* __restrict__ dst, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float va = a[i], vb = b[i];
        if (va != va) va = 0.f;   // np.nan_to_num (registration.py:403-408)
        if (vb != vb) vb = 0.f;
        dst[i] = make_float2(va, vb);
    }
}

// Cross power spectra from the packed transform: p = A conj(B); P1 = p / max(|p|, 100 eps) ("phase"), P2 = p (None).
// The spectra are Hermitian, so their inverse transforms are real and again share one complex transform:
// C = sa Pa + i sb Pb  ->  ifft(C) = sa cc_a + i sb cc_b.  sel_a / sel_b pick which of {P1 (1), P2 (0)} go where
// (sel_b < 0: C = Pa, one correlation per transform).
__global__ void xpower_packed_kernel(const float2* __restrict__ Z, float2* __restrict__ P1, float2* __restrict__ P2,
                                     float2* __restrict__ C, int nz, int ny, int nx, int sel_a, int sel_b) {
    const long long n = (long long)nz * ny * nx;
    float scale_phase = 1.f, scale_plain = 1.f;
    if (sel_b >= 0) mvs_xpower_scales(Z[0], n, &scale_phase, &scale_plain);   // Z[0] = sum(a) + i sum(b)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int kx = (int)(i % nx);
        const long long t = i / nx;
        const int ky = (int)(t % ny), kz = (int)(t / ny);
        const int mx = kx ? nx - kx : 0, my = ky ? ny - ky : 0, mz = kz ? nz - kz : 0;
        // Two correlations in one transform only work if both have the same order of magnitude: float32 rounding of the
        // larger one leaks into the other channel.  The phase-normalised correlation is <= N, the plain one about
        // N * sum(a) * sum(b) for non-negative images (its DC term dominates): both are brought to O(1) by exact
        // powers of two (scale_phase, scale_plain), which commute with every operation of the transform, so each
        // channel holds the bits of its separate transform times its scale, plus ~1e-7 of the other channel.
        float2 p, p1;
        C[i] = mvs_xpower_value(Z[i], Z[((long long)mz * ny + my) * nx + mx], sel_a, sel_b, scale_phase, scale_plain, &p, &p1);
        P1[i] = p1;
        P2[i] = p;
    }
}

// argmax |c| with np.argmax's tie-break (lowest flat index): per-block partial results
// COMP 0: |c| (one correlation per transform); 1 / 2: |Re c| / |Im c| (two real correlations packed in one transform).
// (A template parameter: the variant that selected the component at run time returned wrong maxima for the imaginary part.)
template <int COMP>
__global__ __launch_bounds__(256) void argmax_abs_kernel(const float2* __restrict__ c, long long n, float* __restrict__ pval,
                                                         long long* __restrict__ pidx) {
    constexpr int comp = COMP;
    Peak<1> best = {{-1.f}, {0x7fffffffffffffffLL}};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float2 v = c[i];
        float a;
        if (comp == 0) a = hypotf(v.x, v.y);
        else if (comp == 1) a = fabsf(v.x);
        else a = fabsf(v.y);
        best.merge({{a}, {i}});
    }
    best = mvs_fold::block_fold<4>(best);
    if (threadIdx.x == 0) {
        pval[blockIdx.x] = best.v[0];
        pidx[blockIdx.x] = best.i[0];
    }
}

// Both channels of a packed correlation in ONE pass over the array: argmax |Re| into (pval, pidx), argmax |Im| into (pval2, pidx2)
// -- the same comparisons as argmax_abs_kernel<1> and <2> -- and, from block 0, the DC term of the forward transform (z0_src[0])
// into z0_dst (host memory): one launch instead of three.
__global__ __launch_bounds__(256) void argmax_abs2_kernel(const float2* __restrict__ c, long long n, float* __restrict__ pval,
                                                          long long* __restrict__ pidx, float* __restrict__ pval2, long long* __restrict__ pidx2,
                                                          const float2* __restrict__ z0_src, float2* __restrict__ z0_dst) {
    Peak2 best;
    peak_init(best);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) peak_add(best, c[i], i);
    best = mvs_fold::block_fold<4>(best);
    if (threadIdx.x == 0) {
        pval[blockIdx.x] = best.v[0]; pidx[blockIdx.x] = best.i[0];
        pval2[blockIdx.x] = best.v[1]; pidx2[blockIdx.x] = best.i[1];
        if (blockIdx.x == 0) *z0_dst = *z0_src;
    }
}

// sum of a complex value over the wavefront, in lane 0
__device__ __forceinline__ float2 wave_sum2(float2 v) {
    const mvs_fold::Sums<float, 2> s = mvs_fold::wave_fold(mvs_fold::Sums<float, 2>{{v.x, v.y}});
    return make_float2(s.v[0], s.v[1]);
}

// Upsampled DFT, stage 1: contract the last (x) axis with kernel K (U x nx), input conj(P).
// out[(row) * U + a] = sum_x K[a][x] * conj(P[row][x]); one wavefront per row.
__global__ __launch_bounds__(256) void updft_x_kernel(const float2* __restrict__ P, const float2* __restrict__ K,
                                                      float2* __restrict__ out, long long nrows, int nx, int U) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;
    for (int a = 0; a < U; ++a) {
        float2 acc = make_float2(0.f, 0.f);
        for (int x = lane; x < nx; x += 64) {
            const float2 p = P[row * nx + x];
            const float2 k = K[a * nx + x];
            // k * conj(p)
            acc.x += k.x * p.x + k.y * p.y;
            acc.y += k.y * p.x - k.x * p.y;
        }
        acc = wave_sum2(acc);
        if (lane == 0) out[row * U + a] = acc;
    }
}

// Stage 1 of BOTH normalisations of a packed phase correlation in one pass over the plain cross power P2: the phase-normalised
// one is formed on the fly (the same expression as mvs_xpower_value's p1, so the values are those xpower_packed_kernel would
// have stored), which is why that array is neither written nor read.  Per normalisation the sums run in updft_x_kernel's order.
struct UpdftX2 { const float2* K[2]; float2* out[2]; int phase[2]; };
template <int UM>
__global__ __launch_bounds__(256) void updft_x2_kernel(const float2* __restrict__ P2, UpdftX2 q, long long nrows, int nx, int U) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;
    const float floor_ = 100.f * FLT_EPSILON;
    float2 acc[2][UM];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int a = 0; a < UM; ++a) acc[j][a] = make_float2(0.f, 0.f);
    // a lane's samples of 256 consecutive x are loaded together, then consumed in ascending x like updft_x_kernel's loop.  (One row
    // per wavefront on purpose: a wavefront that keeps the kernel samples in registers and walks four rows ran 47 instead of 34 us
    // -- the contraction is bound by how many short dependent chains are in flight, not by its loads.)
    for (int x0 = lane; x0 < nx; x0 += 256) {
        float2 pv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) pv[i] = (x0 + 64 * i < nx) ? P2[row * nx + x0 + 64 * i] : make_float2(0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = x0 + 64 * i;
            if (x < nx) {
                const float2 p = pv[i];
                const float m = fmaxf(hypotf(p.x, p.y), floor_);
                const float2 p1 = make_float2(p.x / m, p.y / m);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float2 v = q.phase[j] ? p1 : p;
#pragma unroll
                    for (int a = 0; a < UM; ++a) {
                        if (a < U) {
                            const float2 k = q.K[j][a * nx + x];
                            // k * conj(v)
                            acc[j][a].x += k.x * v.x + k.y * v.y;
                            acc[j][a].y += k.y * v.x - k.x * v.y;
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int a = 0; a < UM; ++a) {
            if (a < U) {
                const float2 r = wave_sum2(acc[j][a]);
                if (lane == 0) q.out[j][row * U + a] = r;
            }
        }
}

// Stages 1 AND 2 of both refinements of a 3D pair in one pass over the plain cross power (nx <= 256, U samples per axis):
//   part[(z, chunk)][b][a] = sum_{y in chunk} sum_x Ky[b][y] Kx[a][x] conj(v[z][y][x]).
// A workgroup owns the rows of one y chunk of one plane; every lane sums ITS columns over the wavefront's rows first (the y
// contraction: sequential additions, nothing crosses lanes), then contracts its columns with Kx and only then the 2 x U x U results
// are reduced across the wavefront and the four wavefronts -- one reduction per 16 rows instead of one per row and stage (the
// row-at-a-time kernels spend their time in exactly those reductions: 55 us for the three stages of both refinements of a
// 256 x 256 x 51 crop, 39 us this way).  Stage 3 (updft_mid_kernel over z) folds the chunks
// (kdiv: the chunks of a plane share its kernel sample).  The sums run in a different order than in the separate stages (y before x): equal to them to
// float32 rounding, the refined shifts -- multiples of 1 / upsample -- agree (tests/test_reg_gpu.py).
// (rows of a chunk: kYxRows, at most kYxChunksMax chunks -- mvs_phasecorr_plan.h)
struct UpdftYX { const float2* Kx[2]; const float2* Ky[2]; float2* out[2]; int phase[2]; };
template <int U>
__global__ __launch_bounds__(256) void updft_yx2_kernel(const float2* __restrict__ P2, UpdftYX q, int nz, int ny, int nx, int rows_per_chunk, int nchunks) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = blockIdx.x / nchunks, ch = blockIdx.x % nchunks;
    const int y0 = ch * rows_per_chunk, y1 = min(y0 + rows_per_chunk, ny);
    const float floor_ = 100.f * FLT_EPSILON;
    float2 s[2][U][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int b = 0; b < U; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) s[j][b][i] = make_float2(0.f, 0.f);
    for (int y = y0 + wave; y < y1; y += 4) {
        const float2* row = P2 + ((long long)z * ny + y) * nx;
        float2 pv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) pv[i] = (lane + 64 * i < nx) ? row[lane + 64 * i] : make_float2(0.f, 0.f);
        float2 ky[2][U];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int b = 0; b < U; ++b) ky[j][b] = q.Ky[j][b * ny + y];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (64 * i >= nx) continue;                               // (uniform: short rows use the first lanes' slots only)
            const float2 p = pv[i];                                   // (columns beyond nx hold 0: they add nothing)
            const float m = fmaxf(hypotf(p.x, p.y), floor_);
            const float2 p1 = make_float2(p.x / m, p.y / m);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float2 v = q.phase[j] ? p1 : p;
#pragma unroll
                for (int b = 0; b < U; ++b) {
                    const float2 k = ky[j][b];
                    // k * conj(v)
                    s[j][b][i].x += k.x * v.x + k.y * v.y;
                    s[j][b][i].y += k.y * v.x - k.x * v.y;
                }
            }
        }
    }
    // x contraction of the lane's columns, then across the wavefront
    __shared__ float2 red[4][2 * U * U];
    using WaveSum = rocprim::warp_reduce<float, 64>;
    __shared__ typename WaveSum::storage_type wsum[4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int a = 0; a < U; ++a) {
            float2 kx[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) kx[i] = (lane + 64 * i < nx) ? q.Kx[j][a * nx + lane + 64 * i] : make_float2(0.f, 0.f);
#pragma unroll
            for (int b = 0; b < U; ++b) {
                float2 r = make_float2(0.f, 0.f);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (64 * i >= nx) continue;
                    r.x += kx[i].x * s[j][b][i].x - kx[i].y * s[j][b][i].y;
                    r.y += kx[i].x * s[j][b][i].y + kx[i].y * s[j][b][i].x;
                }
                // (DPP row operations: the bpermute-based shuffle tree costs several times as much, and this kernel is made of reductions)
                WaveSum().reduce(r.x, r.x, wsum[wave]);
                WaveSum().reduce(r.y, r.y, wsum[wave]);
                if (lane == 0) red[wave][(j * U + b) * U + a] = r;
            }
        }
    __syncthreads();
    if (threadIdx.x < 2 * U * U) {
        const int t = threadIdx.x, j = t / (U * U), ba = t % (U * U);
        float2 r = red[0][t];
        for (int w = 1; w < 4; ++w) { r.x += red[w][t].x; r.y += red[w][t].y; }
        q.out[j][(long long)blockIdx.x * (U * U) + ba] = r;
    }
}

// Generic later stage: in has shape (n_outer, n_red, n_inner) -> out (n_outer, U, n_inner):
// out[o][b][i] = sum_r K[b][r] * in[o][r][i]; one wavefront per output element, lanes stride over r (the outputs are
// few -- U^2 nz or U^3 -- and the reduction long, so a thread per output would leave the GPU idle behind a serial loop).
__global__ __launch_bounds__(256) void updft_mid_kernel(const float2* __restrict__ in, const float2* __restrict__ K, float2* __restrict__ out,
                                                        int n_outer, int n_red, int n_inner, int U, int kdiv = 1) {
    const long long total = (long long)n_outer * U * n_inner;
    const int lane = threadIdx.x & 63;
    for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < total; t += (long long)gridDim.x * 4) {
        const int i = (int)(t % n_inner);
        const int b = (int)((t / n_inner) % U);
        const int o = (int)(t / ((long long)n_inner * U));
        float2 acc = make_float2(0.f, 0.f);
        for (int r = lane; r < n_red; r += 64) {
            const float2 v = in[((long long)o * n_red + r) * n_inner + i];
            const float2 k = kdiv == 1 ? K[b * n_red + r] : K[b * (n_red / kdiv) + r / kdiv];   // kdiv consecutive entries share a kernel sample
            acc.x += k.x * v.x - k.y * v.y;
            acc.y += k.x * v.y + k.y * v.x;
        }
        acc = wave_sum2(acc);
        if (lane == 0) out[t] = acc;
    }
}

// nanmin / nanmax / count of one block's share of `a` into slot blockIdx.x of the partials [float min[nb] | float max[nb] |
// long long count[nb]], finished on the host (fold_minmax_partials)
__device__ __forceinline__ void nanminmax_block(const float* __restrict__ a, long long n, char* __restrict__ part, int nb) {
    mvs_fold::Range<long long> r = {INFINITY, -INFINITY, 0};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float v = a[i];
        if (v == v) {
            r.mn = fminf(r.mn, v); r.mx = fmaxf(r.mx, v); ++r.n;
            // upper half of the count: valid voxels that are NOT integers in [0, 65535] (an image of such integers can be rank-
            // ordered by 16-bit keys, see mvs_score.hip)
            if (!(v >= 0.f && v <= 65535.f && v == floorf(v))) r.n += 1ll << 32;
        }
    }
    r = mvs_fold::block_fold<4>(r);
    if (threadIdx.x == 0) {
        ((float*)part)[blockIdx.x] = r.mn;
        ((float*)part)[nb + blockIdx.x] = r.mx;
        ((long long*)(part + (size_t)nb * 8))[blockIdx.x] = r.n;
    }
}
__global__ __launch_bounds__(256) void nanminmax_kernel(const float* __restrict__ a, long long n, char* __restrict__ partials, int nb) {
    nanminmax_block(a, n, partials, nb);
}

// (clip(im, lo, hi) - lo) / (hi - lo) * 1 + 0 in float32, NaN preserved (skimage rescale_intensity)
__global__ void rescale_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n, float lo, float hi, int degenerate) {
    const float d = hi - lo;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float v = src[i];
        if (v == v) {
            v = fminf(fmaxf(v, lo), hi);
            if (!degenerate) v = (v - lo) / d;
            v = v * 1.0f + 0.0f;
        }
        dst[i] = v;
    }
}

// both crops of a pair in one launch (blockIdx.y = image): same bodies
struct PairPtrs { const float* in[2]; float* out[2]; float lo[2], hi[2]; int degenerate[2]; };
__global__ __launch_bounds__(256) void nanminmax_pair_kernel(PairPtrs P, long long n, char* __restrict__ partials, int nb) {
    nanminmax_block(P.in[blockIdx.y], n, partials + (size_t)blockIdx.y * nb * 16, nb);
}
__global__ void rescale_pair_kernel(PairPtrs P, long long n) {
    const int k = blockIdx.y;
    const float* __restrict__ src = P.in[k];
    float* __restrict__ dst = P.out[k];
    const float lo = P.lo[k], hi = P.hi[k];
    const int degenerate = P.degenerate[k];
    const float d = hi - lo;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float v = src[i];
        if (v == v) {
            v = fminf(fmaxf(v, lo), hi);
            if (!degenerate) v = (v - lo) / d;
            v = v * 1.0f + 0.0f;
        }
        dst[i] = v;
    }
}

inline int grid_for(long long n) { return mvs_phasecorr_plan::voxel_grid(n); }

// a few bytes of device memory into the host-resident mailbox
__global__ void peek_kernel(const unsigned int* __restrict__ src, unsigned int* __restrict__ dst, int nwords) {
    for (int i = threadIdx.x; i < nwords; i += blockDim.x) dst[i] = src[i];
}

// min / max / counts over the per-block partials of nanminmax_kernel and nanminmax_pair_kernel: [float min[nb] | float max[nb] |
// long long count[nb]]; the upper half of a count holds the valid voxels that are not 16-bit integers
struct MinMaxCount { float mn, mx; long long nvalid, n_not_u16; };
MinMaxCount fold_minmax_partials(const char* part, int nb) {
    const float* hmin = (const float*)part;
    const float* hmax = hmin + nb;
    const long long* hval = (const long long*)(part + (size_t)nb * 8);
    float a = INFINITY, b = -INFINITY;
    long long v = 0;
    for (int i = 0; i < nb; ++i) { a = std::min(a, hmin[i]); b = std::max(b, hmax[i]); v += hval[i]; }
    MinMaxCount r;
    r.n_not_u16 = v >> 32;
    r.nvalid = v & 0xffffffffll;
    if (r.nvalid == 0) { a = NAN; b = NAN; }
    r.mn = a; r.mx = b;
    return r;
}

}  // namespace

int mvs_device_nanminmax(MvsContext* c, const float* d_in, long long n, float* mn, float* mx, long long* nvalid) {
    const int nb = grid_for(n);
    char* scratch = (char*)mvs_scratch(c, 3, (size_t)nb * 16);
    if (!scratch) return mvs_alloc_failed(c);
    hipLaunchKernelGGL(nanminmax_kernel, dim3(nb), dim3(256), 0, c->stream, d_in, n, scratch, nb);
    MVS_HIP_TRY(c, hipGetLastError());
    std::vector<char> h((size_t)nb * 16);
    MVS_HIP_TRY(c, hipMemcpyAsync(h.data(), scratch, h.size(), hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const MinMaxCount r = fold_minmax_partials(h.data(), nb);
    *mn = r.mn; *mx = r.mx; *nvalid = r.nvalid;
    return MVS_OK;
}

// Intensity normalisation of BOTH crops of a pair (device resident) with one host round trip: the two reductions are
// queued together, their partials come back in one copy, then the two rescale kernels follow.  Same kernels and
// arithmetic as two mvs_rescale_intensity calls.
int mvs_rescale_pair_device(MvsContext* c, const float* in0, const float* in1, long long n, float* out0, float* out1,
                            float mn[2], float mx[2], long long nvalid[2], long long n_not_u16[2], const MvsCropStats* parked) {
    const int nb = std::min(grid_for(n), 512);      // (each block writes its partials over the host link: fewer, longer blocks)
    void *mb_host = nullptr, *mb_dev = nullptr;       // the per-block partials land in host memory directly
    int rcm = mvs_mailbox(c, (size_t)nb * 32, &mb_host, &mb_dev);
    if (rcm) return rcm;
    char* scratch = (char*)mb_dev;
    PairPtrs PP;
    PP.in[0] = in0; PP.in[1] = in1; PP.out[0] = out0; PP.out[1] = out1;
    // (mvs_register_views: the crop kernels have left these partials already -- same layout, same block count)
    // ... and only in the very allocation they were written to: a mailbox that was reallocated in between has lost them
    if (!(parked && parked->done[0] && parked->done[1] && parked->nb == nb && parked->gen == c->mbox_gen && (void*)parked->base == mb_dev))
        hipLaunchKernelGGL(nanminmax_pair_kernel, dim3(nb, 2), dim3(256), 0, c->stream, PP, n, scratch, nb);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 2; ++k) {
        const MinMaxCount r = fold_minmax_partials((const char*)mb_host + (size_t)k * nb * 16, nb);
        n_not_u16[k] = r.n_not_u16;
        mn[k] = r.mn; mx[k] = r.mx; nvalid[k] = r.nvalid;
        PP.lo[k] = r.mn; PP.hi[k] = r.mx; PP.degenerate[k] = r.mn == r.mx ? 1 : 0;
    }
    MVS_DUP("rescale", hipLaunchKernelGGL(rescale_pair_kernel, dim3(nb, 2), dim3(256), 0, c->stream, PP, n));
    MVS_HIP_TRY(c, hipGetLastError());
    return MVS_OK;
}

// device-resident building blocks (used by mvs_phasecorr and mvs_score.hip)
int mvs_stage_float_volume(MvsContext* c, const float* src, int32_t mem, long long n, int slot, float** dptr) {
    if (mem == MVS_MEM_DEVICE) { *dptr = (float*)src; return MVS_OK; }
    float* d = (float*)mvs_scratch(c, slot, (size_t)n * 4);
    if (!d) return mvs_alloc_failed(c);
    MVS_HIP_TRY(c, hipMemcpyAsync(d, src, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    *dptr = d;
    return MVS_OK;
}

extern "C" int mvs_rescale_intensity(int device, const float* in, int32_t mem, int64_t n, float* out, int32_t out_mem,
                                     float* min_out, float* max_out, int64_t* nvalid_out) {
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (!in || !out || n < 1) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_rescale_intensity: bad argument");
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));
    float* din;
    rc = mvs_stage_float_volume(c, in, mem, n, 4, &din);
    if (rc) return rc;
    float mn, mx;
    long long nv;
    rc = mvs_device_nanminmax(c, din, n, &mn, &mx, &nv);
    if (rc) return rc;
    float* dout = out;
    if (out_mem == MVS_MEM_HOST) {
        dout = (float*)mvs_scratch(c, 5, (size_t)n * 4);
        if (!dout) return mvs_alloc_failed(c);
    }
    hipLaunchKernelGGL(rescale_kernel, dim3(grid_for(n)), dim3(256), 0, c->stream, din, dout, (long long)n, mn, mx, mn == mx ? 1 : 0);
    MVS_HIP_TRY(c, hipGetLastError());
    if (out_mem == MVS_MEM_HOST) MVS_HIP_TRY(c, hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (min_out) *min_out = mn;
    if (max_out) *max_out = mx;
    if (nvalid_out) *nvalid_out = nv;
    return MVS_OK;
}

// In-place complex64 (interleaved re, im) n-D transform of one C-contiguous (z,y,x) array: numpy.fft.fftn / ifftn
// without the 1/N of the inverse.  The building block of mvs_phasecorr, exposed so that it can be checked on its own.
extern "C" int mvs_fft_c2c(int device, void* data, int32_t mem, int32_t ndim, const int64_t shape[3], int32_t inverse) {
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (!data || !shape || (ndim != 2 && ndim != 3)) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_fft_c2c: bad argument");
    for (int k = 0; k < 3; ++k)
        if (shape[k] < 1) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_fft_c2c: bad shape");
    if (ndim == 2 && shape[0] != 1) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_fft_c2c: 2D needs shape[0]==1");
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));
    const size_t bytes = (size_t)shape[0] * shape[1] * shape[2] * sizeof(float2);
    float2* d = (float2*)data;
    if (mem == MVS_MEM_HOST) {
        d = (float2*)mvs_scratch(c, 6, bytes);
        if (!d) return mvs_alloc_failed(c);
        MVS_HIP_TRY(c, hipMemcpyAsync(d, data, bytes, hipMemcpyHostToDevice, c->stream));
    }
    rc = mvs_fft3_c2c(c, d, shape, inverse != 0);
    if (rc) return rc;
    if (mem == MVS_MEM_HOST) MVS_HIP_TRY(c, hipMemcpyAsync(data, d, bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MVS_OK;
}

extern "C" int mvs_phasecorr(int device, const float* fixed, const float* moving, int32_t mem, int32_t ndim,
                             const int64_t shape[3], int32_t normalization, int32_t upsample_factor,
                             double shift_out[3], int64_t peak_index_out[3], float* peak_abs_out) {
    return mvs_phasecorr_multi(device, fixed, moving, mem, ndim, shape, &normalization, 1, upsample_factor, shift_out,
                               peak_index_out, peak_abs_out);
}

// ---- mvs_phasecorr_multi: the steps, in the order the exported function at the end runs them ----
// Every decision (route, fusions, peak counts) and every offset (mailbox, refinement scratch) comes from mvs_phasecorr_plan.h.
namespace {
namespace pcp = mvs_phasecorr_plan;

struct NormRefine {      // one normalisation: its shift so far and where its refinement works
    float shift[3] = {0.f, 0.f, 0.f};
    size_t nout = 0;                // complex values of the result
    const float2* P = nullptr;      // the cross power it refines
    float2 *dk = nullptr, *o1 = nullptr, *o2 = nullptr, *o3 = nullptr;      // kernel vectors, outputs of the three stages
    size_t koff[3] = {0, 0, 0};     // the kernel of axis k starts at dk + koff[k]
};
struct Phasecorr {
    MvsContext* c = nullptr;
    int ndim = 0, n_norm = 0, upsample = 1;
    const int64_t* shape = nullptr;
    const int32_t* norms = nullptr;
    long long n = 0;
    int nz = 0, ny = 0, nx = 0;
    pcp::Plan plan;
    pcp::Mailbox mb;
    pcp::Scratch up;
    float *da = nullptr, *db = nullptr;
    // complex work volumes: Z (ONE forward transform of a + i b carries both spectra), P1 / P2 (cross power with and without phase
    // normalisation, kept for the upsampled DFT), CC (inverse transform; both correlations in one transform on the packed routes)
    float2 *Z = nullptr, *P1 = nullptr, *P2 = nullptr, *CC = nullptr;
    char *mb_host = nullptr, *mb_dev = nullptr, *up_base = nullptr;
    float packed_scale[2] = {1.f, 1.f};
    std::vector<NormRefine> norm;
    int sel(int ch) const { return norms[ch] ? 1 : 0; }
    float* peak_val(int ch) const { return (float*)(mb_dev + mb.peak_val(ch)); }
    long long* peak_idx(int ch) const { return (long long*)(mb_dev + mb.peak_idx(ch)); }
    float2* z0_dev() const { return (float2*)(mb_dev + mb.z0); }
};

int validate_and_stage(Phasecorr& s, MvsContext* c, int device, const float* fixed, const float* moving, int32_t mem, int32_t ndim,
                       const int64_t shape[3], const int32_t* normalizations, int32_t n_norm, int32_t upsample_factor, const double* shifts_out) {
    if (!fixed || !moving || !shape || !shifts_out || !normalizations || n_norm < 1)
        return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_phasecorr: NULL argument");
    if (ndim != 2 && ndim != 3) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_phasecorr: ndim must be 2 or 3");
    if (upsample_factor < 1) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_phasecorr: upsample_factor < 1");
    for (int k = 0; k < 3; ++k)
        if (shape[k] < 1) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_phasecorr: bad shape");
    if (ndim == 2 && shape[0] != 1) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_phasecorr: 2D needs shape[0]==1");
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));
    s.c = c; s.ndim = ndim; s.n_norm = n_norm; s.upsample = upsample_factor; s.shape = shape; s.norms = normalizations;
    s.nz = (int)shape[0]; s.ny = (int)shape[1]; s.nx = (int)shape[2];
    s.n = (long long)shape[0] * shape[1] * shape[2];
    s.plan = pcp::plan(ndim, shape, normalizations, n_norm, upsample_factor, mvs_phasecorr_switches(c));
    s.mb = pcp::mailbox(s.plan, ndim, shape, n_norm);
    s.up = pcp::scratch(s.plan, shape, n_norm);
    s.norm.resize((size_t)n_norm);
    int rc = mvs_stage_float_volume(c, fixed, mem, s.n, 4, &s.da);
    if (rc) return rc;
    rc = mvs_stage_float_volume(c, moving, mem, s.n, 5, &s.db);
    if (rc) return rc;
    s.Z = (float2*)mvs_scratch(c, 6, (size_t)s.n * 8 * 4);
    if (!s.Z) return mvs_alloc_failed(c);
    s.P1 = s.Z + s.n;
    s.P2 = s.P1 + s.n;
    s.CC = s.P2 + s.n;
    return MVS_OK;
}

// Z = fft(a + i b); the slab route transforms inside its own passes
int forward_transform(Phasecorr& s) {
    if (s.plan.route == pcp::kSlab) return MVS_OK;
    if (s.plan.forward_reads_crops) {
        MvsFftFuse ff;      // the first pass reads a and b themselves: no packed copy is written and read back
        ff.re_src = s.da;
        ff.im_src = s.db;
        return mvs_fft3_c2c(s.c, s.Z, s.shape, false, &ff);
    }
    hipLaunchKernelGGL(pack_pair_kernel, dim3(s.plan.gb), dim3(256), 0, s.c->stream, s.da, s.db, s.Z, s.n);
    return mvs_fft3_c2c(s.c, s.Z, s.shape, false);
}

int reserve_mailbox(Phasecorr& s) {
    void *host = nullptr, *dev = nullptr;
    const int rc = mvs_mailbox(s.c, s.mb.total, &host, &dev);
    s.mb_host = (char*)host;
    s.mb_dev = (char*)dev;
    return rc;
}

// the packed routes end here: wait for the peaks and the DC term z0, and take the channel scales the device used from z0 (exact
// powers of two), to report the peak heights unscaled
int wait_for_packed_peaks(Phasecorr& s) {
    MVS_HIP_TRY(s.c, hipStreamSynchronize(s.c->stream));
    float s_phase, s_plain;
    mvs_xpower_scales(*(const float2*)(s.mb_host + s.mb.z0), s.n, &s_phase, &s_plain);
    for (int ch = 0; ch < 2; ++ch) s.packed_scale[ch] = s.norms[ch] ? s_phase : s_plain;
    return MVS_OK;
}

// route kSlab: forward transform, cross power and inverse transform in three passes; peaks are in the mailbox
int correlate_slab(Phasecorr& s) {
    float* pv[2] = {s.peak_val(0), s.peak_val(1)};
    long long* pi[2] = {s.peak_idx(0), s.peak_idx(1)};
    const int rc = mvs_phasecorr_slab(s.c, s.da, s.db, s.Z, s.CC, s.P2, s.P1 /* scratch: the slabs' DC terms */, s.shape, s.plan.short_axis, s.sel(0),
                                      s.sel(1), pv, pi, s.z0_dev());
    if (rc) return rc;
    s.c->reg_slab_pairs += 1;
    return wait_for_packed_peaks(s);
}

// route kPacked: both correlations out of ONE inverse transform (real and imaginary channel); peaks are in the mailbox
int correlate_packed(Phasecorr& s) {
    MvsContext* c = s.c;
    if (!s.plan.fuse_xp)
        hipLaunchKernelGGL(xpower_packed_kernel, dim3(s.plan.gb), dim3(256), 0, c->stream, s.Z, s.P1, s.P2, s.CC, s.nz, s.ny, s.nx, s.sel(0), s.sel(1));
    MvsFftFuse fp;
    if (s.plan.last_pass_peaks) {      // no correlation volume written and read back
        for (int ch = 0; ch < 2; ++ch) { fp.peak_val[ch] = s.peak_val(ch); fp.peak_idx[ch] = s.peak_idx(ch); }
        fp.peak_cap = s.plan.ga;
    }
    if (s.plan.fuse_xp) { fp.xp_src = s.Z; fp.xp_p2 = s.P2; fp.xp_sel_a = s.sel(0); fp.xp_sel_b = s.sel(1); }
    const int rc = mvs_fft3_c2c(c, s.CC, s.shape, true, &fp);
    if (rc) return rc;
    if (fp.xp_used != s.plan.fuse_xp || fp.n_peak != (s.plan.last_pass_peaks ? s.plan.n_peak : 0))
        return mvs_fail(c, MVS_ERR_UNSUPPORTED, "phase correlation: the inverse transform did not take the planned fusions");
    if (s.plan.last_pass_peaks)
        hipLaunchKernelGGL(peek_kernel, dim3(1), dim3(64), 0, c->stream, (const unsigned int*)s.Z, (unsigned int*)s.z0_dev(), 2);
    else
        hipLaunchKernelGGL(argmax_abs2_kernel, dim3(s.plan.ga), dim3(256), 0, c->stream, s.CC, s.n, s.peak_val(0), s.peak_idx(0), s.peak_val(1),
                           s.peak_idx(1), s.Z, s.z0_dev());
    MVS_HIP_TRY(c, hipGetLastError());
    return wait_for_packed_peaks(s);
}

// route kPerNorm: one cross power, one inverse transform and one round trip for this normalisation; peaks are in the mailbox (channel 0)
int correlate_one_norm(Phasecorr& s, int inorm) {
    MvsContext* c = s.c;
    hipLaunchKernelGGL(xpower_packed_kernel, dim3(s.plan.gb), dim3(256), 0, c->stream, s.Z, s.P1, s.P2, s.CC, s.nz, s.ny, s.nx, s.sel(inorm), -1);
    const int rc = mvs_fft3_c2c(c, s.CC, s.shape, true);   // cc (unnormalised inverse: argmax is scale invariant)
    if (rc) return rc;
    hipLaunchKernelGGL(argmax_abs_kernel<0>, dim3(s.plan.ga), dim3(256), 0, c->stream, s.CC, s.n, s.peak_val(0), s.peak_idx(0));
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MVS_OK;
}

// integer peak of one normalisation out of the mailbox -> outputs, signed shift
void read_peaks(Phasecorr& s, int inorm, int64_t* peak_index_out, float* peak_abs_out) {
    const bool packed = s.plan.route != pcp::kPerNorm;
    const int ch = packed ? inorm : 0;
    float best;
    long long bi, peak[3];
    pcp::argmax_partials((const float*)(s.mb_host + s.mb.peak_val(ch)), (const long long*)(s.mb_host + s.mb.peak_idx(ch)), s.plan.n_peak, &best, &bi);
    if (packed) best /= s.packed_scale[inorm];
    pcp::unravel(bi, s.shape, peak);
    if (peak_index_out)
        for (int k = 0; k < 3; ++k) peak_index_out[k] = peak[k];
    if (peak_abs_out) *peak_abs_out = best / (float)s.n;   // ifftn's 1/N
    pcp::peak_to_shift(peak, s.shape, s.norm[inorm].shift);
}

int reserve_refinement_scratch(Phasecorr& s) {
    if (!s.plan.refine) return MVS_OK;
    s.up_base = (char*)mvs_scratch(s.c, 7, s.up.total);
    return s.up_base ? MVS_OK : mvs_alloc_failed(s.c);
}

// stage 2 (y -> (z, uy, ux)) and, in 3D, stage 3 (z -> (uz, uy, ux)) of one normalisation; the last one writes the mailbox
void later_stages(Phasecorr& s, int j) {
    const NormRefine& sj = s.norm[j];
    const int U = s.plan.U;
    hipLaunchKernelGGL(updft_mid_kernel, dim3((unsigned)std::min<long long>(((long long)s.up.s2 + 3) / 4, 4096)), dim3(256), 0, s.c->stream, sj.o1, sj.dk + sj.koff[1], sj.o2, s.nz, s.ny, U, U);
    if (s.ndim == 3)
        hipLaunchKernelGGL(updft_mid_kernel, dim3((unsigned)std::min<long long>(((long long)s.up.s3 + 3) / 4, 4096)), dim3(256), 0, s.c->stream, sj.o2, sj.dk + sj.koff[0], sj.o3, 1, s.nz, U * U, U);
}

// stage 1 (x -> (z, y, ux)) of ONE normalisation from its stored cross power, then its later stages
int stage1_one_norm(Phasecorr& s, int inorm) {
    const NormRefine& st = s.norm[inorm];
    const long long nrows = (long long)s.nz * s.ny;
    hipLaunchKernelGGL(updft_x_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, s.c->stream, st.P, st.dk + st.koff[2], st.o1, nrows, s.nx, s.plan.U);
    later_stages(s, inorm);
    MVS_HIP_TRY(s.c, hipGetLastError());
    return MVS_OK;
}

// stage 1 of BOTH normalisations from the plain cross power alone, then their later stages
int stage1_both_norms(Phasecorr& s) {
    const long long nrows = (long long)s.nz * s.ny;
    UpdftX2 q;
    for (int j = 0; j < 2; ++j) { q.K[j] = s.norm[j].dk + s.norm[j].koff[2]; q.out[j] = s.norm[j].o1; q.phase[j] = s.sel(j); }
    hipLaunchKernelGGL(updft_x2_kernel<4>, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, s.c->stream, s.P2, q, nrows, s.nx, s.plan.U);
    for (int j = 0; j < s.n_norm; ++j) later_stages(s, j);
    MVS_HIP_TRY(s.c, hipGetLastError());
    return MVS_OK;
}

// stages 1 AND 2 of both normalisations: partial sums per (z, y chunk) in the stage-1 area (they fit: tests/test_phasecorr_plan_host.py),
// folded by stage 3
int stage1_and_2_both_norms(Phasecorr& s) {
    const int U = s.plan.U, chunks = s.plan.yx_chunks;
    UpdftYX q;
    for (int j = 0; j < 2; ++j) {
        q.Kx[j] = s.norm[j].dk + s.norm[j].koff[2]; q.Ky[j] = s.norm[j].dk + s.norm[j].koff[1]; q.out[j] = s.norm[j].o1;
        q.phase[j] = s.sel(j);
    }
    MVS_DUP("updft", hipLaunchKernelGGL(updft_yx2_kernel<3>, dim3((unsigned)(s.nz * chunks)), dim3(256), 0, s.c->stream, s.P2, q, s.nz, s.ny, s.nx,
                       s.plan.rows_per_chunk, chunks));
    for (int j = 0; j < s.n_norm; ++j)
        MVS_DUP("updft_mid", hipLaunchKernelGGL(updft_mid_kernel, dim3((unsigned)std::min<long long>(((long long)s.up.s3 + 3) / 4, 4096)), dim3(256), 0, s.c->stream,
                           s.norm[j].o1, s.norm[j].dk + s.norm[j].koff[0], s.norm[j].o3, 1, s.nz * chunks, U * U, U, chunks));
    MVS_HIP_TRY(s.c, hipGetLastError());
    return MVS_OK;
}

// The upsampled DFT around one normalisation's integer peak: its kernel vectors go into the mailbox, and its launches are queued -- at
// once when every normalisation runs its own stage 1, after the last normalisation when one launch serves both.  Nothing is waited for.
int queue_refinements(Phasecorr& s, int inorm) {
    NormRefine& st = s.norm[inorm];
    float offs[3];
    pcp::round_to_grid(st.shift, s.upsample, s.plan.U, offs);
    float2* hk = (float2*)(s.mb_host + s.mb.kvec_of(inorm));   // stays untouched until the caller's wait
    size_t nk = 0;
    for (int k = (s.ndim == 3) ? 0 : 1; k < 3; ++k) {
        st.koff[k] = nk;
        nk += pcp::fill_kernel(hk + nk, (int)s.shape[k], s.plan.U, offs[k], s.upsample);
    }
    st.P = s.norms[inorm] ? s.P1 : s.P2;
    st.dk = (float2*)(s.up_base + s.up.kvec_of(inorm));
    st.o1 = (float2*)(s.up_base + s.up.stage_of(inorm));
    st.o2 = st.o1 + s.up.s1;
    st.o3 = st.o2 + s.up.s2;
    (s.ndim == 3 ? st.o3 : st.o2) = (float2*)(s.mb_dev + s.mb.res_of(inorm));     // the last stage writes host memory
    st.nout = s.ndim == 3 ? s.up.s3 : s.up.s2;
    // (the vectors are copied by a kernel out of the mapped mailbox: a DMA upload would queue behind any tile upload in flight)
    if (!s.plan.fuse_xp) {
        const int rc = mvs_upload_from_mapped(s.c, st.dk, s.mb_dev + s.mb.kvec_of(inorm), pcp::upload_bytes(nk * sizeof(float2)));
        return rc ? rc : stage1_one_norm(s, inorm);
    }
    if (inorm != s.n_norm - 1) return MVS_OK;
    // one upload for all normalisations: the vectors lie kvec_stride apart in the mailbox and on the device alike
    const int rc = mvs_upload_from_mapped(s.c, s.up_base, s.mb_dev + s.mb.kvec, pcp::upload_bytes((size_t)inorm * s.up.kvec_stride + nk * sizeof(float2)));
    if (rc) return rc;
    return s.plan.fuse_yx ? stage1_and_2_both_norms(s) : stage1_both_norms(s);
}

// sub-pixel maximum of every refinement (their results are in the mailbox), then the shifts go out; refined_out (may be NULL) takes a
// copy of every normalisation's result, nout values each
void finish_shifts(Phasecorr& s, double* shifts_out, float2* refined_out) {
    for (int inorm = 0; inorm < s.n_norm; ++inorm) {
        NormRefine& st = s.norm[inorm];
        if (s.plan.refine) {
            const float2* res = (const float2*)(s.mb_host + s.mb.res_of(inorm));
            const size_t iu = pcp::subpixel_argmax(res, st.nout);
            pcp::add_subpixel(st.shift, iu, s.plan.U, s.ndim, s.upsample);
            if (refined_out) std::copy(res, res + st.nout, refined_out + (size_t)inorm * st.nout);
        }
        pcp::zero_unit_axes(st.shift, s.shape);
        for (int k = 0; k < 3; ++k) shifts_out[3 * inorm + k] = (double)st.shift[k];
    }
}

// the body of mvs_phasecorr_multi and mvs_phasecorr_multi_refined: the same launches whether or not the refinement is read back
int phasecorr_multi(MvsContext* c, int device, const float* fixed, const float* moving, int32_t mem, int32_t ndim, const int64_t shape[3],
                    const int32_t* normalizations, int32_t n_norm, int32_t upsample_factor, double* shifts_out, int64_t* peak_indices_out,
                    float* peak_abs_out_all, float2* refined_out) {
    int rc;
    Phasecorr s;
    rc = validate_and_stage(s, c, device, fixed, moving, mem, ndim, shape, normalizations, n_norm, upsample_factor, shifts_out);
    if (rc) return rc;
    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    rc = forward_transform(s);
    if (rc) return rc;
    rc = reserve_mailbox(s);
    if (rc) return rc;
    // two different normalisations share one correlation pass and one host round trip ...
    if (s.plan.route == pcp::kSlab) rc = correlate_slab(s);
    else if (s.plan.route == pcp::kPacked) rc = correlate_packed(s);
    if (rc) return rc;
    rc = reserve_refinement_scratch(s);
    if (rc) return rc;
    // ... otherwise every normalisation has its own.  Per normalisation: integer peak -> upsampled DFT around it; the refinements
    // of all normalisations are queued before the host waits once for their results.
    for (int inorm = 0; inorm < n_norm; ++inorm) {
        if (s.plan.route == pcp::kPerNorm) rc = correlate_one_norm(s, inorm);
        if (rc) return rc;
        read_peaks(s, inorm, peak_indices_out ? peak_indices_out + 3 * inorm : nullptr, peak_abs_out_all ? peak_abs_out_all + inorm : nullptr);
        if (s.plan.refine) rc = queue_refinements(s, inorm);
        if (rc) return rc;
    }
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    if (s.plan.refine) MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    finish_shifts(s, shifts_out, refined_out);
    return MVS_OK;
}

}  // namespace

extern "C" int mvs_phasecorr_multi(int device, const float* fixed, const float* moving, int32_t mem, int32_t ndim,
                                   const int64_t shape[3], const int32_t* normalizations, int32_t n_norm,
                                   int32_t upsample_factor, double* shifts_out, int64_t* peak_indices_out,
                                   float* peak_abs_out_all) {
    MvsContext* c;
    const int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    return phasecorr_multi(c, device, fixed, moving, mem, ndim, shape, normalizations, n_norm, upsample_factor, shifts_out, peak_indices_out,
                           peak_abs_out_all, nullptr);
}

extern "C" int mvs_phasecorr_multi_refined(int device, const float* fixed, const float* moving, int32_t mem, int32_t ndim,
                                           const int64_t shape[3], const int32_t* normalizations, int32_t n_norm,
                                           int32_t upsample_factor, double* shifts_out, int64_t* peak_indices_out,
                                           float* peak_abs_out_all, float* refined_out, int64_t refined_capacity) {
    MvsContext* c;
    const int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    // refused before anything is staged or launched
    if (upsample_factor > 1 && (ndim == 2 || ndim == 3) && n_norm >= 1) {
        const long long U = pcp::refine_samples(upsample_factor);
        const long long need = 2 * (long long)n_norm * (ndim == 3 ? U * U * U : U * U);
        if (!refined_out) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_phasecorr_multi_refined: NULL refined_out");
        if (refined_capacity < need) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_phasecorr_multi_refined: refined_capacity too small");
    }
    return phasecorr_multi(c, device, fixed, moving, mem, ndim, shape, normalizations, n_norm, upsample_factor, shifts_out, peak_indices_out,
                           peak_abs_out_all, (float2*)refined_out);
}
