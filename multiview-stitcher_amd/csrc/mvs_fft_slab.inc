// mvs_fft_slab.inc -- two axes of the phase correlation's 3D transform in ONE pass over HBM; included by mvs_fft_slab_lo.hip /
// _hi.hip, which instantiate the short lengths 17..44 / 45..64 (two units build side by side, like the whole-line kernels).
//
// The overlap crop of two neighbouring tiles is a slab itself: ~50 samples across the overlap, 256 along the other two axes
// (registration.py:314-316), and the three-pass transform reads and writes its 27 MB once per axis.  All samples of the short axis
// and of one long axis at ONE index of the third are S x L <= 64 x 256 complex numbers = 2 S registers for each of L threads: a
// workgroup takes such a slab, thread k loads the S samples of its long-axis position k (coalesced: the threads' samples of one s
// lie side by side) and transforms them as a whole-line DFT in its registers (mvs_dft_small.h); the L-point lines then go through
// LDS sixteen at a time (35 KB: four workgroups per CU) onto the register butterflies of mvs_fft_reg.h, whose second pass writes
// the result out (or reduces it to the peaks).  The pair of passes costs one read and one write.  With the remaining axis done by
// long_xp_kernel (forward, cross power, inverse in one pass) the phase correlation of a pair moves 5 x 27 MB where the six
// single-axis passes moved 12-13 x 27 MB.
// Fusions at the two ends as in the single-axis kernels (MvsFftFuse): the forward slab reads the real and imaginary parts from two
// float volumes; the inverse slab reduces its output to the per-workgroup peaks instead of storing it.
// (First version: the whole slab in LDS, 111 KB, one workgroup per CU -- alone as fast as this one, but a launch then waits for a
// CU whose LDS the kernels of the other context lanes have left free: 115 us per launch inside the 8-lane pair loop.)
#include "mvs_dft_small.h"
#include "mvs_fft_dev.h"
#include "mvs_fft_reg.h"

namespace {

__device__ __forceinline__ float2 slab_load(const SlabArgs& A, long long g, bool inv) {
    if (A.re_src) {
        float re = A.re_src[g], im = A.im_src[g];          // NaN -> 0 (np.nan_to_num, registration.py:403-408)
        re = (re != re) ? 0.f : re;
        im = (im != im) ? 0.f : im;
        return make_float2(re, im);
    }
    const float2 x = A.data[g];
    return inv ? make_float2(x.y, x.x) : x;                // IDFT(x) = swap(DFT(swap(x))), swap = exchange of re and im
}

// the L = R1 x R2 point transforms of the slab's S lines, LPB lines at a time through LDS: thread k hands over its sample of every
// line of the batch, the 16 (8) threads of a line run fft_reg2_kernel's two register transforms around one exchange, the second
// one's output goes to memory (or into the peak search).  Same factorisation, twiddles and order of operations as fft_reg2_kernel.
template <int S, int R1, int R2>
__device__ __forceinline__ void slab_long_axis(float2 (&v)[S], float2* __restrict__ T, const float2* __restrict__ tw, const SlabArgs& A,
                                               long long base, bool inv, Peak2& pk) {
    constexpr int M = R1 * R2, TPL = R1 > R2 ? R1 : R2, LPB = 256 / TPL, PS = R2 + 1;
    constexpr int LS = ((R1 * PS > M ? R1 * PS : M) + 1) | 1;
    constexpr int NB = (S + LPB - 1) / LPB;
    const int tid = (int)threadIdx.x;
    // rows of L contiguous samples: the threads of a line are adjacent (a line's 16 outputs of one k are 128 contiguous bytes);
    // rows of S contiguous samples: adjacent threads hold adjacent lines (the 16 lines' outputs of one position are contiguous)
    const int line = A.short_contig ? tid % LPB : tid / TPL, idx = A.short_contig ? tid / LPB : tid % TPL;
    float2* row = T + line * LS;
    sdft::static_for<0, NB>([&](auto b_) {
        constexpr int s0 = decltype(b_)::value * LPB;
        if (tid < M) {
            sdft::static_for<0, LPB>([&](auto l_) {
                constexpr int l = decltype(l_)::value;
                if constexpr (s0 + l < S) T[l * LS + tid] = v[s0 + l];
            });
        }
        __syncthreads();
        const int s = s0 + line;
        const bool live = s < S;
        float2 x[R1];
        if (live && idx < R2) {
#pragma unroll
            for (int q = 0; q < R1; ++q) x[q] = row[q * R2 + idx];
            dft_reg<R1>(x);
        }
        __syncthreads();                                   // every sample of the batch's lines has been read
        if (live && idx < R2) {
#pragma unroll
            for (int p = 0; p < R1; ++p) row[p * PS + idx] = p == 0 ? x[0] : cmul(x[p], tw_at(tw, idx * p, M / 2));
        }
        __syncthreads();
        if (live && idx < R1) {
            float2 u[R2];
#pragma unroll
            for (int j = 0; j < R2; ++j) u[j] = row[idx * PS + j];
            dft_reg<R2>(u);
            if (A.dc && s == 0 && idx == 0) A.dc[blockIdx.x] = u[0];
#pragma unroll
            for (int k = 0; k < R2; ++k) {
                const int m = idx + R1 * k;
                const float2 o = inv ? make_float2(u[k].y, u[k].x) : u[k];
                const long long g = A.short_contig ? base + (long long)m * S + s : base + (long long)s * A.row_stride + m;
                if (A.peak_val[0]) peak_add(pk, o, g); else A.data[g] = o;
            }
        }
        __syncthreads();                                   // the next batch overwrites the lines
    });
}

template <int S>
__global__ __launch_bounds__(256) void slab_kernel(SlabArgs A) {
    constexpr int LSH = S | 1;                             // line pitch of the staging area (rows of S contiguous samples)
    constexpr int NW = (64 * S + 255) / 256;
    extern __shared__ float2 T[];
    __shared__ float2 tw[128];
    const int tid = (int)threadIdx.x;
    const int L = A.L;
    for (int t = tid; t < L / 2; t += 256) tw[t] = A.tw[t];
    const long long base = (long long)blockIdx.x * A.slab_stride;
    const bool inv = A.inverse != 0;
    const bool mine = tid < L;
    float2 v[S];
    // ---- the short axis: thread k takes the S samples at its position k of the long axis ----
    if (!A.short_contig) {
        // S rows of L contiguous samples: sample s of the threads is one contiguous piece; all S requests are issued before the first
        // value is used
        sdft::static_for<0, S>([&](auto s_) {
            constexpr int s = decltype(s_)::value;
            v[s] = mine ? slab_load(A, base + (long long)s * A.row_stride + tid, inv) : make_float2(0.f, 0.f);
        });
    } else {
        // L rows of S contiguous samples back to back: 64 rows at a time are copied through LDS, coalesced on the global side, one row
        // per thread on the register side (row pitch S | 1: conflict-free 8-byte reads), like dft_line_kernel's contiguous lines
        sdft::static_for<0, S>([&](auto s_) { constexpr int s = decltype(s_)::value; v[s] = make_float2(0.f, 0.f); });
        for (int r0 = 0; r0 < L; r0 += 64) {
            const int nt = (L - r0 < 64 ? L - r0 : 64) * S;
            float2 w[NW];
            sdft::static_for<0, NW>([&](auto i_) {
                constexpr int i = decltype(i_)::value;
                const int t = i * 256 + tid;
                w[i] = t < nt ? slab_load(A, base + (long long)r0 * S + t, inv) : make_float2(0.f, 0.f);
            });
            sdft::static_for<0, NW>([&](auto i_) {
                constexpr int i = decltype(i_)::value;
                const int t = i * 256 + tid;
                if (t < nt) {
                    const int r = t / S, s = t - r * S;
                    T[r * LSH + s] = w[i];
                }
            });
            __syncthreads();
            if (tid >= r0 && tid < r0 + 64 && mine)
                sdft::static_for<0, S>([&](auto s_) { constexpr int s = decltype(s_)::value; v[s] = T[(tid - r0) * LSH + s]; });
            __syncthreads();
        }
    }
    if (mine) sdft::dft_nat<S>(v);
    __syncthreads();                                       // (twiddles; the staging area is free)
    // ---- the long axis ----
    Peak2 pk;
    peak_init(pk);
    if (L == 256) slab_long_axis<S, 16, 16>(v, T, tw, A, base, inv, pk);
    else if (L == 128) slab_long_axis<S, 16, 8>(v, T, tw, A, base, inv, pk);
    else slab_long_axis<S, 8, 8>(v, T, tw, A, base, inv, pk);
    if (A.peak_val[0]) peak_flush<4>(pk, A.peak_val, A.peak_idx);
}

template <int N, int LO>
bool launch_slab(MvsContext* c, const SlabArgs& A, unsigned grid, size_t lds_bytes, hipError_t* err) {
    if constexpr (N < LO) {
        return false;
    } else {
        if constexpr (mvs_dft_line_length(N))
            if (A.S == N) {
                MVS_DUP("slab", hipLaunchKernelGGL(slab_kernel<N>, dim3(grid), dim3(256), lds_bytes, c->stream, A));
                *err = hipGetLastError();
                return true;
            }
        return launch_slab<N - 1, LO>(c, A, grid, lds_bytes, err);
    }
}

}  // namespace
