// mvs_phasecorr_plan.h -- the one definition of everything mvs_phasecorr_multi (mvs_reg.hip) decides without the device: which
// kernel family a line pass of the transform runs on (mvs_fft3_c2c takes its dispatch from the same rule), which route a phase
// correlation takes, where its results lie in the mailbox and in the refinement scratch, and the host arithmetic of skimage's
// phase_cross_correlation around the device work.  Plain functions, no HIP calls: tests/native/phasecorr_plan_host_test.cpp
// compiles them for the host (tests/test_phasecorr_plan_host.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

// lengths the whole-line kernel is built for: non-powers of two from 17 to 64 whose prime factors are <= 19 (mvs_dft_small.h)
constexpr bool mvs_dft_line_length(int n) {
    if (n < 17 || n > 64 || (n & (n - 1)) == 0) return false;
    for (int p = 2; p <= 19; ++p)
        while (n % p == 0) n /= p;
    return n == 1;
}

// channel scales of the packed pair of correlations (exact powers of two, see xpower_packed_kernel): the device brings both
// channels to O(1) with them, the host divides the peak heights by them again
__host__ __device__ __forceinline__ void mvs_xpower_scales(float2 z0, long long n, float* scale_phase, float* scale_plain) {
    const float dc = fabsf(z0.x * z0.y);           // sum(a) * sum(b): the DC term of the plain cross power
    *scale_plain = (dc > 0.f && dc < INFINITY) ? ldexpf(1.f, -ilogbf(dc)) : 1.f;
    *scale_phase = ldexpf(1.f, -ilogbf((float)n));
}

namespace mvs_phasecorr_plan {

constexpr int kYxChunksMax = 64, kYxRows = 64;      // updft_yx2_kernel: rows of a chunk, 16 per wavefront (measured 8 ... 128 rows: 60.6, 42.7, 33.9, 33.0, 38.2 us for stages 1-3)

// ---- the pass rule: one line pass of mvs_fft3_c2c -------------------------------------------------------------------------------
// kLine / kRegPow2 / kRegBluestein are the register kernels, the ones that carry the fusions of MvsFftFuse.
enum PassKind { kLine, kRegPow2, kRegBluestein, kLds, kFourStep };
struct Pass {
    PassKind kind;
    int M;               // Stockham size: n for powers of two, else the Bluestein length (the first power of two >= 2 n - 1)
    int lines_per_wg;    // 0 for kFourStep
    long long grid;      // workgroups of the pass (kFourStep: 0, it runs several launches of its own)
    bool fused() const { return kind == kLine || kind == kRegPow2 || kind == kRegBluestein; }
};
// lines per workgroup of the LDS kernel (measured on 51 x 256 x 256: 8 beats 4 and 16 for both kinds of pass; LDS 33 KB -> 4 workgroups / CU)
inline int lds_lines_per_wg(int M, bool contiguous) {
    const int l = (contiguous ? 2048 : 4096) / M;
    return l < 1 ? 1 : l > 8 ? 8 : l;
}
inline Pass line_pass(int n, long long n_lines, bool contiguous, bool fft_no_line) {
    Pass p;
    const bool pow2 = (n & (n - 1)) == 0;
    p.M = 1;
    if (pow2) p.M = n;
    else while (p.M < 2 * n - 1) p.M <<= 1;
    if (n > 4096 || (!pow2 && n > 2048)) {      // beyond the LDS core (Bluestein of n > 2048 needs M = 8192 points per line)
        p.kind = kFourStep; p.lines_per_wg = 0; p.grid = 0;
        return p;
    }
    if (mvs_dft_line_length(n) && !fft_no_line) { p.kind = kLine; p.lines_per_wg = 64; }
    else if (pow2 && (n == 64 || n == 128 || n == 256)) { p.kind = kRegPow2; p.lines_per_wg = n == 64 ? 32 : 16; }
    else if (!pow2 && p.M >= 64 && p.M <= 256) { p.kind = kRegBluestein; p.lines_per_wg = p.M == 64 ? 32 : 16; }
    else { p.kind = kLds; p.lines_per_wg = lds_lines_per_wg(p.M, contiguous); }
    p.grid = (n_lines + p.lines_per_wg - 1) / p.lines_per_wg;
    return p;
}
// The first inverse pass along x that forms the cross power takes its lines as partner pairs (kz, ky), (-kz, -ky) on the
// power-of-two register kernel: does it, and with how many workgroups
inline bool xp_pairs(const Pass& p, bool fft_no_pair) { return p.kind == kRegPow2 && p.lines_per_wg % 2 == 0 && !fft_no_pair; }
inline long long xp_pair_grid(const Pass& p, long long nz, long long ny) {
    const long long h = ny / 2 + 1, ncanon = h + ((nz - 1) / 2) * ny + ((nz % 2 == 0) ? h : 0);
    return (ncanon + p.lines_per_wg / 2 - 1) / (p.lines_per_wg / 2);
}

// first / last transformed axis: the transform runs x, y, z and skips axes of length 1 (-1: there is none)
inline void transformed_axes(const int64_t shape[3], int* first_axis, int* last_axis) {
    *first_axis = *last_axis = -1;
    for (int axis = 2; axis >= 0; --axis)
        if (shape[axis] > 1) { if (*first_axis < 0) *first_axis = axis; *last_axis = axis; }
}

// ---- switches (options of the context) and the slab rule -------------------------------------------------------------------------
struct Switches {
    bool reg_unfused = false, materialize_shifts = false, fft_no_slab = false, fft_no_line = false, fft_no_pair = false;
    int fft_slab_axes = 4;
};
inline bool slab_long_length(int64_t n) { return n == 64 || n == 128 || n == 256; }
// the three-pass form (mvs_fft_slab.hip): one short axis (a whole-line DFT length) and two power-of-two axes; which axis is the
// short one (-1: the crop is not of the slab kind)
inline int slab_axis(const int64_t shape[3], const Switches& sw) {
    if (sw.fft_no_slab || sw.fft_no_line || sw.reg_unfused) return -1;
    int as = -1;
    for (int k = 0; k < 3; ++k) {
        if (slab_long_length(shape[k])) continue;
        if (shape[k] > 64 || !mvs_dft_line_length((int)shape[k]) || as >= 0) return -1;
        as = k;
    }
    if (as >= 0 && !((sw.fft_slab_axes >> as) & 1)) return -1;
    return as;
}
// workgroups of its last pass (= entries of the peak arrays the caller must provide)
inline int slab_peaks(const int64_t shape[3], int short_axis) { return (int)(short_axis == 0 ? shape[1] : shape[0]); }

// ---- the plan ------------------------------------------------------------------------------------------------------------------
// kSlab: forward transform, cross power and inverse in three passes (mvs_phasecorr_slab); kPacked: two different normalisations
// share ONE inverse transform (real and imaginary channel, see xpower_packed_kernel) and one host round trip; kPerNorm: one
// inverse transform and one round trip per normalisation.
enum Route { kSlab, kPacked, kPerNorm };
struct Plan {
    Route route;
    int first_axis, last_axis;      // transformed_axes
    int short_axis;                 // kSlab: the short axis
    int U;                          // samples per axis of the refinement: ceil(1.5 * upsample_factor)
    bool refine;                    // upsample_factor > 1
    bool forward_reads_crops;       // the first forward pass reads a and b themselves: no packed copy is written and read back
    // stage 1 of the refinement runs per normalisation on its stored cross power (updft_x_kernel), or
    bool fuse_xp;                   // the cross power is formed inside the first inverse pass (slab route: inside long_xp_kernel) and stage 1 of
                                    // both refinements reads the plain one in one launch (updft_x2_kernel), or
    bool fuse_yx;                   // stages 1 and 2 of both refinements are one launch (updft_yx2_kernel)
    int yx_chunks, rows_per_chunk;
    bool last_pass_peaks;           // kPacked: the last inverse pass reduces its output to per-workgroup peaks instead of storing it
    int gb;                         // workgroups of the voxel-sized kernels
    int ga;                         // peak entries per array the mailbox holds (= workgroups of the stand-alone peak kernels)
    int n_peak;                     // peak entries the correlation leaves per channel
};

inline int refine_samples(int upsample_factor) { return (int)ceilf((float)upsample_factor * 1.5f); }
inline int voxel_grid(long long n) { const long long b = (n + 255) / 256; return (int)(b < 256 * 8 ? b : 256 * 8); }

inline Plan plan(int ndim, const int64_t shape[3], const int32_t* normalizations, int n_norm, int upsample_factor, const Switches& sw) {
    Plan p;
    const long long nz = shape[0], ny = shape[1], nx = shape[2], n = nz * ny * nx;
    transformed_axes(shape, &p.first_axis, &p.last_axis);
    p.U = refine_samples(upsample_factor);
    p.refine = upsample_factor > 1;
    auto pass_of = [&](int axis) { return line_pass((int)shape[axis], n / shape[axis], axis == 2, sw.fft_no_line); };
    const bool packed = n_norm == 2 && (normalizations[0] != 0) != (normalizations[1] != 0) && !sw.materialize_shifts;
    // crops with one short axis and two power-of-two axes, two normalisations, small refinement: three passes in all
    p.short_axis = (ndim == 3 && packed && p.U <= 4) ? slab_axis(shape, sw) : -1;
    p.route = p.short_axis >= 0 ? kSlab : packed ? kPacked : kPerNorm;
    p.forward_reads_crops = p.route != kSlab && p.first_axis >= 0 && pass_of(p.first_axis).fused() && !sw.reg_unfused;
    // ... when the first inverse pass (along x) runs on the register kernels and the refinement is small, it forms the cross power
    // itself and both refinements' first stage read it in one launch: the combined spectrum and the phase-normalised cross power
    // are never stored
    p.fuse_xp = p.route == kSlab || (p.route == kPacked && p.first_axis == 2 && pass_of(2).fused() && p.U <= 4 && !sw.reg_unfused);
    // ... and in 3D (refinement of 3 samples per axis: upsample factor 2) the first TWO stages of both refinements are one pass
    p.fuse_yx = p.fuse_xp && ndim == 3 && p.U == 3 && nx <= 256 && ny >= 4;
    p.yx_chunks = 1;
    if (p.fuse_yx) {
        const int want = ((int)ny + kYxRows - 1) / kYxRows;
        p.yx_chunks = want < 1 ? 1 : want > kYxChunksMax ? kYxChunksMax : want;
    }
    p.rows_per_chunk = ((int)ny + p.yx_chunks - 1) / p.yx_chunks;
    // blocks of the peak searches (one host-memory write each): 512 for the stand-alone kernels, or the workgroups of the inverse
    // transform's last pass when that pass does the search itself (16 lines each at the least)
    p.gb = voxel_grid(n);
    long long ga = p.gb < 512 ? p.gb : 512;
    const bool last_fused = p.last_axis >= 0 && pass_of(p.last_axis).fused();
    if (last_fused && (n / shape[p.last_axis] + 15) / 16 > ga) ga = (n / shape[p.last_axis] + 15) / 16;
    if (p.route == kSlab && slab_peaks(shape, p.short_axis) > ga) ga = slab_peaks(shape, p.short_axis);
    p.ga = (int)ga;
    // the correlation volume is only ever searched for its two peaks: when the last pass of the inverse transform runs on the
    // register kernels it reduces its output to per-workgroup maxima instead of storing it
    p.last_pass_peaks = p.route == kPacked && last_fused && !sw.reg_unfused;
    p.n_peak = p.ga;
    if (p.route == kSlab) p.n_peak = slab_peaks(shape, p.short_axis);
    if (p.last_pass_peaks) {
        const Pass last = pass_of(p.last_axis);
        const bool pairs = p.fuse_xp && p.last_axis == p.first_axis && xp_pairs(last, sw.fft_no_pair);
        p.n_peak = (int)(pairs ? xp_pair_grid(last, nz, ny) : last.grid);
    }
    return p;
}

// ---- layouts -------------------------------------------------------------------------------------------------------------------
inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }
// bytes between the kernel vectors of two normalisations: the SAME in the mailbox (where the host fills them) and in the scratch
// (where the kernels read them), so that one copy carries the vectors of all normalisations
inline size_t kvec_stride(const int64_t shape[3], int U) { return align256((size_t)U * (size_t)(shape[0] + shape[1] + shape[2]) * sizeof(float2)); }
inline size_t upload_bytes(size_t nbytes) { return (nbytes + 15) / 16 * 16; }      // mvs_upload_from_mapped copies 16-byte units

// mailbox (host memory written by the kernels): [peaks: per channel ga values, ga indices | z0 (the DC term of the packed spectrum)
// | refinement results of every normalisation | kernel vectors of every normalisation (pinned: filled by the host, copied by a kernel)]
struct Mailbox {
    size_t ga, z0, res, res_stride, kvec, kvec_stride, total;
    size_t peak_val(int ch) const { return (size_t)ch * ga * 16; }
    size_t peak_idx(int ch) const { return (size_t)ch * ga * 16 + ga * 8; }
    size_t res_of(int inorm) const { return res + res_stride * (size_t)inorm; }
    size_t kvec_of(int inorm) const { return kvec + kvec_stride * (size_t)inorm; }
};
inline Mailbox mailbox(const Plan& p, int ndim, const int64_t shape[3], int n_norm) {
    Mailbox m;
    const size_t U = (size_t)p.U, res_elems = p.refine ? (ndim == 3 ? U * U * U : U * U) : 0;
    m.ga = (size_t)p.ga;
    m.z0 = m.ga * 32;
    m.res = m.z0 + 256;
    m.res_stride = align256(res_elems * sizeof(float2));
    m.kvec = m.res + m.res_stride * (size_t)n_norm;
    m.kvec_stride = p.refine ? kvec_stride(shape, p.U) : 0;
    m.total = m.kvec + m.kvec_stride * (size_t)n_norm;
    return m;
}

// refinement scratch: [kernel vectors of every normalisation | stage outputs of every normalisation: s1 (z, y, ux), s2 (z, uy, ux),
// s3 (uz, uy, ux) complex values].  With merged stages 1 and 2 the chunk partials (nz * yx_chunks * U * U) live in the s1 area.
struct Scratch {
    size_t kvec_stride, s1, s2, s3, stage_stride, stages, total;
    size_t kvec_of(int inorm) const { return kvec_stride * (size_t)inorm; }
    size_t stage_of(int inorm) const { return stages + stage_stride * (size_t)inorm; }
};
inline Scratch scratch(const Plan& p, const int64_t shape[3], int n_norm) {
    Scratch s;
    const size_t U = (size_t)p.U;
    s.kvec_stride = kvec_stride(shape, p.U);
    s.s1 = (size_t)shape[0] * (size_t)shape[1] * U;
    s.s2 = (size_t)shape[0] * U * U;
    s.s3 = U * U * U;
    s.stage_stride = (s.s1 + s.s2 + s.s3) * sizeof(float2) + 1024;
    s.stages = s.kvec_stride * (size_t)n_norm;
    s.total = (s.kvec_stride + s.stage_stride) * (size_t)n_norm;
    return s;
}

// ---- host arithmetic of skimage.registration.phase_cross_correlation ------------------------------------------------------------
// arg max over per-workgroup partials; the lowest flat index wins among equal values (np.argmax)
inline void argmax_partials(const float* val, const long long* idx, int n, float* best_out, long long* idx_out) {
    float best = -1.f;
    long long bi = 0;
    for (int i = 0; i < n; ++i)
        if (val[i] > best || (val[i] == best && idx[i] < bi)) { best = val[i]; bi = idx[i]; }
    *best_out = best;
    *idx_out = bi;
}
inline void unravel(long long flat, const int64_t shape[3], long long peak[3]) {
    peak[0] = flat / ((long long)shape[1] * shape[2]);
    peak[1] = (flat / shape[2]) % shape[1];
    peak[2] = flat % shape[2];
}
// signed shift, float32 arithmetic like skimage
inline void peak_to_shift(const long long peak[3], const int64_t shape[3], float shift[3]) {
    for (int k = 0; k < 3; ++k) {
        shift[k] = (float)peak[k];
        const float mid = truncf((float)shape[k] / 2.f);   // np.fix(axis_size / 2)
        if (shift[k] > mid) shift[k] -= (float)shape[k];
    }
}
inline float dft_shift(int U) { return truncf((float)U / 2.f); }
// the shift rounded to the upsampling grid, and where the refinement window starts relative to it
inline void round_to_grid(float shift[3], int upsample_factor, int U, float offs[3]) {
    const float uf = (float)upsample_factor;
    for (int k = 0; k < 3; ++k) {
        shift[k] = nearbyintf(shift[k] * uf) / uf;            // np.round: half to even
        offs[k] = dft_shift(U) - shift[k] * uf;
    }
}
// fftfreq(n, d)[x] as numpy computes it: the integer frequency times 1 / (n d)
inline double fftfreq(int n, double d, int x) {
    const int half = (n - 1) / 2 + 1;
    return (double)(x < half ? x : x - n) * (1.0 / ((double)n * d));
}
// kernel exp(-2 pi i (a - off) * fftfreq(n, uf)[x]), a < U, computed in double in the order of skimage's _upsampled_dft -- (a - off)
// times the frequency first, then times -2 pi: where the exact value of a component is 0 the result is the rounding of that phase, and
// only the same phase gives the same float32 -- cast to complex64; returns U * n
inline size_t fill_kernel(float2* out, int n, int U, float off, int upsample_factor) {
    size_t nk = 0;
    for (int a = 0; a < U; ++a)
        for (int x = 0; x < n; ++x) {
            const double ph = -2.0 * M_PI * (((double)a - (double)off) * fftfreq(n, (double)(float)upsample_factor, x));
            out[nk++] = make_float2((float)cos(ph), (float)sin(ph));
        }
    return nk;
}
// argmax |.| of a refinement's result (conj does not change the modulus), lowest flat index
inline size_t subpixel_argmax(const float2* res, size_t nout) {
    float bu = -1.f;
    size_t iu = 0;
    for (size_t i = 0; i < nout; ++i) {
        const float a = hypotf(res[i].x, res[i].y);
        if (a > bu) { bu = a; iu = i; }
    }
    return iu;
}
inline void add_subpixel(float shift[3], size_t iu, int U, int ndim, int upsample_factor) {
    const float uf = (float)upsample_factor;
    int m[3] = {0, 0, 0};
    m[2] = (int)(iu % U);
    m[1] = (int)((iu / U) % U);
    if (ndim == 3) m[0] = (int)(iu / ((size_t)U * U));
    for (int k = (ndim == 3) ? 0 : 1; k < 3; ++k) shift[k] += ((float)m[k] - dft_shift(U)) / uf;
}
inline void zero_unit_axes(float shift[3], const int64_t shape[3]) {
    for (int k = 0; k < 3; ++k)
        if (shape[k] == 1) shift[k] = 0.f;
}

}  // namespace mvs_phasecorr_plan
