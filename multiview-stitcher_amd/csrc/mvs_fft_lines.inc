// mvs_fft_lines.inc -- the whole-line DFT kernels (see mvs_dft_small.h); included by mvs_fft_lines_lo.hip / _hi.hip, which
// instantiate the lengths MVS_LINES_LO .. MVS_LINES_HI each (two units build side by side).
#include "mvs_dft_small.h"
#include "mvs_fft_dev.h"

namespace {

// ---- short composite lines (N <= 64, prime factors <= 19) as whole-line transforms in the registers of one thread --------------
// mvs_dft_small.h.  One wavefront per workgroup, one line per lane.  Lines along y / z: sample j of the 64 lines of a wavefront
// is 512 contiguous bytes (adjacent x positions), loaded and stored directly.  Lines along x lie back to back in memory: the
// wavefront copies its 64 lines (64 N contiguous samples) through LDS, coalesced on the global side, one line per lane on the
// register side (line stride N | 1 float2: conflict-free 8-byte reads).  Carries every fusion of the other register kernels
// (MvsFftFuse): real / imaginary parts from two float volumes, the cross power formed on the fly, the peak search instead of a store.
template <int N>
__global__ __launch_bounds__(64) void dft_line_kernel(FftArgs A) {
    constexpr int LS = N | 1;
    extern __shared__ float2 ex[];      // 64 * LS samples for contiguous lines, nothing otherwise (launch_dft_line): lines along y / z must
                                        // not hold 26 KB of LDS per wavefront that the kernels of the other context lanes could use
    const bool inv = A.inverse != 0;
    const bool contig = A.stride == 1 && A.inner == 1 && A.outer_stride == N;
    const int lane = threadIdx.x;
    const long long l0 = (long long)blockIdx.x * 64;
    const long long l = l0 + lane;
    const bool live = l < A.n_lines;
    const int nl = (int)(A.n_lines - l0 < 64 ? A.n_lines - l0 : 64);
    const long long base = live ? line_base(A, (int)l) : 0;
    float2 v[N];
    if (contig) {
        // element t = lane + 64 i of the wavefront's 64 N contiguous samples: all N requests are issued before the first is used
        const long long base0 = l0 * N;
        const int nt = nl * N;
        if (A.xp_src) {
            // (ky, kz) of the workgroup's first line once; a sample's line is at most 63 further: one float reciprocal instead
            // of a 64-bit division per sample; the channel scales are the same for every line
            XpLine xl = xp_line(A, l0);
            const int ky0 = (int)(l0 % A.xp_ny), kz0 = (int)(l0 / A.xp_ny);
            const float rny = 1.f / (float)A.xp_ny;
            sdft::static_for<0, N>([&](auto i_) {
                constexpr int i = decltype(i_)::value;
                const int t = lane + 64 * i;
                v[i] = make_float2(0.f, 0.f);
                if (t < nt) {
                    const int ln = t / N, k = t - ln * N;
                    const int kyl = ky0 + ln;
                    int q = (int)((float)kyl * rny);
                    int ky = kyl - q * A.xp_ny;
                    if (ky < 0) { ky += A.xp_ny; --q; }
                    if (ky >= A.xp_ny) { ky -= A.xp_ny; ++q; }
                    const int kz = kz0 + q;
                    const int my = ky ? A.xp_ny - ky : 0, mz = kz ? A.xp_nz - kz : 0;
                    xl.mbase = ((long long)mz * A.xp_ny + my) * N;
                    v[i] = xp_load(A, xl, base0 + (long long)ln * N, k);
                }
            });
        } else {
            sdft::static_for<0, N>([&](auto i_) {
                constexpr int i = decltype(i_)::value;
                const int t = lane + 64 * i;
                v[i] = t < nt ? fft_load(A, base0 + t) : make_float2(0.f, 0.f);
            });
        }
        sdft::static_for<0, N>([&](auto i_) {
            constexpr int i = decltype(i_)::value;
            const int t = lane + 64 * i;
            const int ln = t / N, k = t - ln * N;
            ex[ln * LS + k] = v[i];
        });
        __syncthreads();
        sdft::static_for<0, N>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            v[j] = ex[lane * LS + j];
        });
    } else {
        sdft::static_for<0, N>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            v[j] = live ? fft_load(A, base + (long long)j * A.stride) : make_float2(0.f, 0.f);
        });
    }
    if (inv) {      // IDFT(x) = swap(DFT(swap(x))), swap = exchange of real and imaginary parts
        sdft::static_for<0, N>([&](auto j_) { constexpr int j = decltype(j_)::value; v[j] = make_float2(v[j].y, v[j].x); });
    }
    sdft::dft_nat<N>(v);
    if (inv) {
        sdft::static_for<0, N>([&](auto j_) { constexpr int j = decltype(j_)::value; v[j] = make_float2(v[j].y, v[j].x); });
    }
    if (A.peak_val[0]) {
        Peak2 pk;
        peak_init(pk);
        if (live) {
            sdft::static_for<0, N>([&](auto j_) {
                constexpr int j = decltype(j_)::value;
                peak_add(pk, v[j], base + (long long)j * A.stride);
            });
        }
        peak_flush<1>(pk, A.peak_val, A.peak_idx);
        return;
    }
    if (contig) {
        __syncthreads();
        sdft::static_for<0, N>([&](auto j_) { constexpr int j = decltype(j_)::value; ex[lane * LS + j] = v[j]; });
        __syncthreads();
        const long long base0 = l0 * N;
        const int nt = nl * N;
        sdft::static_for<0, N>([&](auto i_) {
            constexpr int i = decltype(i_)::value;
            const int t = lane + 64 * i;
            const int ln = t / N, k = t - ln * N;
            v[i] = ex[ln * LS + k];
        });
        sdft::static_for<0, N>([&](auto i_) {
            constexpr int i = decltype(i_)::value;
            const int t = lane + 64 * i;
            if (t < nt) A.data[base0 + t] = v[i];
        });
    } else if (live) {
        sdft::static_for<0, N>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            A.data[base + (long long)j * A.stride] = v[j];
        });
    }
}


template <int N, int LO>
bool launch_dft_line(MvsContext* c, const FftArgs& A, unsigned grid) {
    if constexpr (N < LO) {
        return false;
    } else {
        if constexpr (mvs_dft_line_length(N))
            if (A.n == N) {
                const bool contig = A.stride == 1 && A.inner == 1 && A.outer_stride == N;
                hipLaunchKernelGGL(dft_line_kernel<N>, dim3(grid), dim3(64), contig ? sizeof(float2) * 64 * (N | 1) : 0, c->stream, A);
                return true;
            }
        return launch_dft_line<N - 1, LO>(c, A, grid);
    }
}

}  // namespace
