// mvs_masked_corr.hip -- masked normalised cross-correlation of two overlap crops on gfx950 (Padfield 2012; what
// skimage.registration.phase_cross_correlation computes with reference_mask / moving_mask): for every integer shift of a window the
// Pearson correlation of the two crops over the voxels valid in both, and the arg-max among the shifts with enough overlap.  The
// contract is stated with mvs_masked_corr in mvs_hip.h.  The chain, queued on one stream without a host step in the middle:
//   statistics (count, sum, min, max of the valid voxels of either crop) -> pack (three zero-padded complex volumes) ->
//   three forward transforms (mvs_fft3_c2c) -> spectral combine, in place -> three inverse transforms ->
//   window maximum -> window search -> result record.
// 256-thread workgroups, fixed-tree reductions, no atomics at all: equal inputs give equal bits.  Padded shape, window and limit:
// mvs_masked_corr_plan.h.
#include "mvs_internal.h"
#include "mvs_fft.h"
#include "mvs_fold_dev.h"
#include "mvs_masked_corr_plan.h"

#include <cfloat>
#include <climits>
#include <cmath>

namespace {

using namespace mvs_masked_corr_plan;
static_assert(kMaxVoxels == MVS_MASKED_CORR_MAX_VOXELS, "limits of mvs_hip.h and mvs_masked_corr_plan.h differ");
static_assert(kOk == MVS_MASKED_CORR_OK && kNoEligibleShift == MVS_MASKED_CORR_NO_ELIGIBLE_SHIFT && kTooFewValid == MVS_MASKED_CORR_TOO_FEW_VALID &&
                  kConstantCrop == MVS_MASKED_CORR_CONSTANT_CROP,
              "status codes of mvs_hip.h and mvs_masked_corr_plan.h differ");

// ---- what the kernels share ---------------------------------------------------------------------------------------------------------
struct Crops {
    const float* im[2];                // fixed, moving: C-contiguous, the crop's shape
    const unsigned char* mask[2];      // or NULL
    double thr[2];
    int has_thr[2];
};

// all extents fit an int: prod(P) <= 2^28 (the plan's limit) and every other product is below it
struct Dims {
    int nz, ny, nx;          // crop
    int Sz, Sy, Sx;          // largest |shift|
    int Pz, Py, Px;          // padded, powers of two
    int ly, lx;              // log2 Py, log2 Px
    int Wz, Wy, Wx;          // window
    int voxels, padded, window;
};

struct StatPartial {
    double sum;
    long long n;
    float mn, mx;
    __device__ __forceinline__ void merge(const StatPartial& o) { sum += o.sum; n += o.n; mn = fminf(mn, o.mn); mx = fmaxf(mx, o.mx); }
    template <typename S> __device__ __forceinline__ StatPartial shuffled(S sh, int off) const { return {sh(sum, off), sh(n, off), sh(mn, off), sh(mx, off)}; }
};

// what the pack pass needs of a crop, and the status rule: n, mu = sum / n, range = max - min (1 where that is 0 or n == 0)
struct CropNorm {
    long long n;
    float mu, range, mn, mx;
};

__device__ __forceinline__ bool voxel_valid(const Crops& C, int k, int i, float v) {
    bool ok = fabsf(v) < INFINITY;                                   // (a NaN is not)
    if (C.mask[k]) ok = ok && C.mask[k][i] != 0;
    if (C.has_thr[k]) ok = ok && (double)v > C.thr[k];
    return ok;
}

// ---- statistics ---------------------------------------------------------------------------------------------------------------------
// grid (nb, 2): crop blockIdx.y, one partial per workgroup ...
__global__ __launch_bounds__(kThreads) void mc_stats_kernel(Crops C, int voxels, StatPartial* partials) {
    const int k = blockIdx.y;
    StatPartial a{0.0, 0, INFINITY, -INFINITY};
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < voxels; i += gridDim.x * kThreads) {
        const float v = C.im[k][i];
        if (voxel_valid(C, k, i, v)) a.merge({(double)v, 1, v, v});
    }
    a = mvs_fold::block_fold<kWaves>(a);
    if (threadIdx.x == 0) partials[k * gridDim.x + blockIdx.x] = a;
}

// ... and one workgroup per crop that folds them in a fixed order
__global__ __launch_bounds__(kThreads) void mc_stats_final_kernel(const StatPartial* partials, int nb, CropNorm* norms) {
    const int k = blockIdx.x;
    StatPartial a{0.0, 0, INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < nb; i += kThreads) a.merge(partials[k * nb + i]);
    a = mvs_fold::block_fold<kWaves>(a);
    if (threadIdx.x == 0) {
        CropNorm r;
        r.n = a.n;
        r.mu = a.n ? (float)(a.sum / (double)a.n) : 0.f;
        r.mn = a.mn;
        r.mx = a.mx;
        const float range = a.mx - a.mn;
        r.range = (a.n && range > 0.f && range < INFINITY) ? range : 1.f;
        norms[k] = r;
    }
}

// ---- pack ---------------------------------------------------------------------------------------------------------------------------
// One pass over the padded index space: Z1 = f + i g, Z2 = vF + i vM, Z3 = f^2 + i g^2 with f = (F - mu_F) / range_F on the valid
// voxels of the fixed crop and 0 elsewhere (outside the crop too), g likewise of the moving crop.  Centring keeps the variance sums
// of the search out of float32 cancellation.
__global__ __launch_bounds__(kThreads) void mc_pack_kernel(Crops C, Dims D, const CropNorm* __restrict__ norms, float2* Z1, float2* Z2, float2* Z3) {
    const CropNorm nf = norms[0], nm = norms[1];
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < D.padded; i += gridDim.x * kThreads) {
        const int x = i & (D.Px - 1), y = (i >> D.lx) & (D.Py - 1), z = i >> (D.lx + D.ly);
        float f = 0.f, g = 0.f, vf = 0.f, vm = 0.f;
        if (z < D.nz && y < D.ny && x < D.nx) {
            const int j = (z * D.ny + y) * D.nx + x;
            const float a = C.im[0][j], b = C.im[1][j];
            if (voxel_valid(C, 0, j, a)) { vf = 1.f; f = (a - nf.mu) / nf.range; }
            if (voxel_valid(C, 1, j, b)) { vm = 1.f; g = (b - nm.mu) / nm.range; }
        }
        Z1[i] = make_float2(f, g);
        Z2[i] = make_float2(vf, vm);
        Z3[i] = make_float2(f * f, g * g);
    }
}

// ---- spectral combine ---------------------------------------------------------------------------------------------------------------
// the spectra of the two real volumes packed as Z = fft(a + i b), at k, from z = Z(k) and m = Z(-k)
__device__ __forceinline__ void split_pair(float2 z, float2 m, float2* a, float2* b) {
    *a = make_float2(0.5f * (z.x + m.x), 0.5f * (z.y - m.y));      // (Z(k) + conj Z(-k)) / 2
    *b = make_float2(0.5f * (z.y + m.y), -0.5f * (z.x - m.x));     // (Z(k) - conj Z(-k)) / 2i
}
// conj(a) b: the spectrum of corr(a, b)(s) = sum_x a(x) b(x + s)
__device__ __forceinline__ float2 corr_spec(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x); }
// Two real correlations with the spectra c and d at k, packed as c + i d: its value at k and, both being Hermitian, at -k.
__device__ __forceinline__ void pack_pair(float2 c, float2 d, float scale, float2* at_k, float2* at_mk) {
    *at_k = make_float2((c.x - d.y) * scale, (c.y + d.x) * scale);
    *at_mk = make_float2((c.x + d.y) * scale, (d.x - c.y) * scale);
}

// In place: X1 = corr(vF, vM) + i corr(f, g), X2 = corr(f, vM) + i corr(vF, g), X3 = corr(f^2, vM) + i corr(vF, g^2) as spectra,
// scaled by 1 / prod(P) (a power of two: exact) for the unnormalised inverse transform.  One thread owns the pair {k, -k mod P}: the
// one of the two with the lower flat index takes it, reads all six values, then writes them; a self-paired k is written once.
__global__ __launch_bounds__(kThreads) void mc_combine_kernel(Dims D, float scale, float2* Z1, float2* Z2, float2* Z3) {
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < D.padded; i += gridDim.x * kThreads) {
        const int x = i & (D.Px - 1), y = (i >> D.lx) & (D.Py - 1), z = i >> (D.lx + D.ly);
        const int mx = (D.Px - x) & (D.Px - 1), my = (D.Py - y) & (D.Py - 1), mz = (D.Pz - z) & (D.Pz - 1);
        const int m = (((mz << D.ly) + my) << D.lx) + mx;
        if (m < i) continue;
        const float2 z1 = Z1[i], z2 = Z2[i], z3 = Z3[i], m1 = Z1[m], m2 = Z2[m], m3 = Z3[m];
        float2 f, g, vf, vm, f2, g2;
        split_pair(z1, m1, &f, &g);
        split_pair(z2, m2, &vf, &vm);
        split_pair(z3, m3, &f2, &g2);
        float2 k1, k2, k3, n1, n2, n3;
        pack_pair(corr_spec(vf, vm), corr_spec(f, g), scale, &k1, &n1);
        pack_pair(corr_spec(f, vm), corr_spec(vf, g), scale, &k2, &n2);
        pack_pair(corr_spec(f2, vm), corr_spec(vf, g2), scale, &k3, &n3);
        Z1[i] = k1; Z2[i] = k2; Z3[i] = k3;
        if (m != i) { Z1[m] = n1; Z2[m] = n2; Z3[m] = n3; }
    }
}

// ---- assemble and search ------------------------------------------------------------------------------------------------------------
struct ShiftTerms {
    int n;                // rint(N)
    float num, den;       // cFM - cF cM / N and sqrt(dF dM)
};

// flat padded index of the window entry (wz, wy, wx)
__device__ __forceinline__ int window_index(const Dims& D, int wz, int wy, int wx) {
    const int sz = wz - D.Sz, sy = wy - D.Sy, sx = wx - D.Sx;
    const int iz = sz < 0 ? sz + D.Pz : sz, iy = sy < 0 ? sy + D.Py : sy, ix = sx < 0 ? sx + D.Px : sx;
    return (((iz << D.ly) + iy) << D.lx) + ix;
}

// N is divided by as max(rint(N), 1): where no voxel overlaps every sum is rounding noise and the denominator falls below the tolerance
__device__ __forceinline__ ShiftTerms shift_terms(const float2* __restrict__ X1, const float2* __restrict__ X2, const float2* __restrict__ X3, int idx) {
    const float2 a = X1[idx], b = X2[idx], c = X3[idx];
    const float nr = rintf(a.x), nc = fmaxf(nr, 1.f);
    const float dF = fmaxf(c.x - b.x * b.x / nc, 0.f), dM = fmaxf(c.y - b.y * b.y / nc, 0.f);
    ShiftTerms t;
    t.n = (int)nr;
    t.num = a.y - b.x * b.y / nc;
    t.den = sqrtf(dF * dM);
    return t;
}

__device__ __forceinline__ float shift_r(const ShiftTerms& t, float tol) { return t.den > tol ? fminf(fmaxf(t.num / t.den, -1.f), 1.f) : 0.f; }
__device__ __forceinline__ bool shift_eligible(int n, int nmax, double overlap_ratio, long long min_overlap) {
    return (double)n >= fmax(overlap_ratio * (double)nmax, (double)min_overlap);
}

struct MaxPartial {
    int nmax;
    float denmax;
    __device__ __forceinline__ void merge(const MaxPartial& o) { nmax = max(nmax, o.nmax); denmax = fmaxf(denmax, o.denmax); }
    template <typename S> __device__ __forceinline__ MaxPartial shuffled(S sh, int off) const { return {sh(nmax, off), sh(denmax, off)}; }
};
struct PeakPartial {
    float r;            // -inf: none
    int w;              // window index, INT_MAX: none
    int any_positive;   // an eligible shift whose denominator is above the tolerance
    // larger r wins, among equals the lower window index
    __device__ __forceinline__ void merge(const PeakPartial& o) {
        if (o.r > r || (o.r == r && o.w < w)) { r = o.r; w = o.w; }
        any_positive |= o.any_positive;
    }
    template <typename S> __device__ __forceinline__ PeakPartial shuffled(S sh, int off) const { return {sh(r, off), sh(w, off), sh(any_positive, off)}; }
};

// (a) the largest rint(N) and the largest denominator of the window
__global__ __launch_bounds__(kThreads) void mc_window_max_kernel(Dims D, const float2* __restrict__ X1, const float2* __restrict__ X2, const float2* __restrict__ X3,
                                                                 MaxPartial* partials) {
    MaxPartial a{0, 0.f};
    for (int w = blockIdx.x * kThreads + threadIdx.x; w < D.window; w += gridDim.x * kThreads) {
        const int wx = w % D.Wx, wy = (w / D.Wx) % D.Wy, wz = w / (D.Wx * D.Wy);
        const ShiftTerms t = shift_terms(X1, X2, X3, window_index(D, wz, wy, wx));
        a.merge({t.n, t.den});
    }
    a = mvs_fold::block_fold<kWaves>(a);
    if (threadIdx.x == 0) partials[blockIdx.x] = a;
}

struct SearchArgs {
    double overlap_ratio;
    long long min_overlap;
    const MaxPartial* max_partials;
    int n_max_partials;
    float* r_out;       // or NULL: the window's r ...
    int* n_out;         // ... and rint(N)
};

// (b) r of every window entry and the arg-max among the eligible ones, one partial per workgroup
__global__ __launch_bounds__(kThreads) void mc_window_search_kernel(Dims D, SearchArgs A, const float2* __restrict__ X1, const float2* __restrict__ X2,
                                                                    const float2* __restrict__ X3, PeakPartial* partials) {
    MaxPartial mp{0, 0.f};
    for (int i = threadIdx.x; i < A.n_max_partials; i += kThreads) mp.merge(A.max_partials[i]);
    mp = mvs_fold::block_fold_all<kWaves>(mp);      // (every thread: the search needs it in all)
    const float tol = 1e3f * FLT_EPSILON * mp.denmax;
    PeakPartial a{-INFINITY, INT_MAX, 0};
    for (int w = blockIdx.x * kThreads + threadIdx.x; w < D.window; w += gridDim.x * kThreads) {
        const int wx = w % D.Wx, wy = (w / D.Wx) % D.Wy, wz = w / (D.Wx * D.Wy);
        const ShiftTerms t = shift_terms(X1, X2, X3, window_index(D, wz, wy, wx));
        const float r = shift_r(t, tol);
        if (A.r_out) A.r_out[w] = r;
        if (A.n_out) A.n_out[w] = t.n;
        if (shift_eligible(t.n, mp.nmax, A.overlap_ratio, A.min_overlap)) a.merge({r, w, t.den > tol ? 1 : 0});
    }
    a = mvs_fold::block_fold<kWaves>(a);
    if (threadIdx.x == 0) partials[blockIdx.x] = a;
}

// One workgroup: the fold of the search's partials, the status, and the record with the peak's axis neighbours.
__global__ __launch_bounds__(kThreads) void mc_result_kernel(Dims D, SearchArgs A, const float2* __restrict__ X1, const float2* __restrict__ X2,
                                                             const float2* __restrict__ X3, const PeakPartial* partials, int n_partials,
                                                             const CropNorm* norms, mvs_masked_corr_result_t* out) {
    MaxPartial mp{0, 0.f};
    for (int i = threadIdx.x; i < A.n_max_partials; i += kThreads) mp.merge(A.max_partials[i]);
    mp = mvs_fold::block_fold_all<kWaves>(mp);      // (every thread: the search needs it in all)
    const float tol = 1e3f * FLT_EPSILON * mp.denmax;
    PeakPartial a{-INFINITY, INT_MAX, 0};
    for (int i = threadIdx.x; i < n_partials; i += kThreads) a.merge(partials[i]);
    a = mvs_fold::block_fold<kWaves>(a);
    if (threadIdx.x != 0) return;
    const CropNorm nf = norms[0], nm = norms[1];
    mvs_masked_corr_result_t R;
    R.status = kOk;
    if (nf.n < A.min_overlap || nm.n < A.min_overlap) R.status = kTooFewValid;
    else if (nf.mn == nf.mx || nm.mn == nm.mx) R.status = kConstantCrop;
    else if (!a.any_positive) R.status = kNoEligibleShift;
    R.reserved = 0;
    R.n_max = mp.nmax;
    R.n_valid[0] = nf.n;
    R.n_valid[1] = nm.n;
    R.padded[0] = D.Pz; R.padded[1] = D.Py; R.padded[2] = D.Px;
    R.max_shift[0] = D.Sz; R.max_shift[1] = D.Sy; R.max_shift[2] = D.Sx;
    const int S[3] = {D.Sz, D.Sy, D.Sx}, W[3] = {D.Wz, D.Wy, D.Wx};
    int pw[3] = {D.Sz, D.Sy, D.Sx};      // no peak: the zero shift
    R.r = NAN;
    R.n_peak = 0;
    const bool found = a.w != INT_MAX;
    if (found) {
        pw[2] = a.w % D.Wx; pw[1] = (a.w / D.Wx) % D.Wy; pw[0] = a.w / (D.Wx * D.Wy);
        R.r = a.r;
        R.n_peak = shift_terms(X1, X2, X3, window_index(D, pw[0], pw[1], pw[2])).n;
    }
    for (int d = 0; d < 3; ++d) {
        R.peak[d] = pw[d] - S[d];
        for (int side = 0; side < 2; ++side) {
            int q[3] = {pw[0], pw[1], pw[2]};
            q[d] += side ? 1 : -1;
            float r = NAN;
            int ok = 0;
            if (found && q[d] >= 0 && q[d] < W[d]) {
                const ShiftTerms t = shift_terms(X1, X2, X3, window_index(D, q[0], q[1], q[2]));
                r = shift_r(t, tol);
                ok = shift_eligible(t.n, mp.nmax, A.overlap_ratio, A.min_overlap) ? 1 : 0;
            }
            R.neighbour_r[2 * d + side] = r;
            R.neighbour_ok[2 * d + side] = ok;
        }
    }
    *out = R;
}

}  // namespace

extern "C" int mvs_masked_corr(int device, const float* fixed, const float* moving, const uint8_t* fixed_mask, const uint8_t* moving_mask,
                               const int64_t shape[3], const mvs_masked_corr_opts_t* opts, mvs_masked_corr_result_t* result, float* r_out,
                               int32_t* n_out) {
    const char* what = "mvs_masked_corr";
    MvsContext* c0 = mvs_ctx(device);
    if (!fixed || !moving || !shape || !opts || !result) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (opts->mem != MVS_MEM_HOST && opts->mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: bad mem", what);
    if ((fixed_mask || moving_mask) && opts->mask_mem != MVS_MEM_HOST && opts->mask_mem != MVS_MEM_DEVICE)
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: bad mask_mem", what);
    if (!(opts->overlap_ratio > 0.0 && opts->overlap_ratio <= 1.0)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: overlap_ratio must be in (0, 1]", what);
    if (opts->min_overlap < 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: min_overlap < 1", what);
    for (int k = 0; k < 2; ++k)
        if (opts->has_valid_above[k] && std::isnan(opts->valid_above[k])) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: valid_above is NaN", what);
    Plan plan;
    const PlanCode pc = make_plan(opts->ndim, shape, opts->max_shift, &plan);
    if (pc == kPlanBadShape) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3, shape[k] >= 1, 2D crops have shape[0] == 1", what);
    if (pc == kPlanTooLarge)
        return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: the padded volume exceeds MVS_MASKED_CORR_MAX_VOXELS = %lld voxels; lower max_shift", what, kMaxVoxels);
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    Dims D;
    D.nz = (int)plan.n[0]; D.ny = (int)plan.n[1]; D.nx = (int)plan.n[2];
    D.Sz = (int)plan.S[0]; D.Sy = (int)plan.S[1]; D.Sx = (int)plan.S[2];
    D.Pz = (int)plan.P[0]; D.Py = (int)plan.P[1]; D.Px = (int)plan.P[2];
    D.ly = plan.lp[1]; D.lx = plan.lp[2];
    D.Wz = (int)plan.W[0]; D.Wy = (int)plan.W[1]; D.Wx = (int)plan.W[2];
    D.voxels = (int)plan.voxels; D.padded = (int)plan.padded; D.window = (int)plan.window;

    // one block: the spectra, the partials of the reductions, the window volumes of the debug output, host crops and host masks
    const size_t spec_bytes = align_up((size_t)plan.padded * sizeof(float2));
    const size_t stat_bytes = align_up(sizeof(StatPartial) * 2 * (size_t)plan.voxel_blocks);
    const size_t norm_bytes = align_up(sizeof(CropNorm) * 2);
    const size_t max_bytes = align_up(sizeof(MaxPartial) * (size_t)plan.window_blocks);
    const size_t peak_bytes = align_up(sizeof(PeakPartial) * (size_t)plan.window_blocks);
    const size_t win_bytes = align_up((size_t)plan.window * 4);
    const size_t crop_bytes = opts->mem == MVS_MEM_HOST ? align_up((size_t)plan.voxels * 4) : 0;
    const size_t mask_bytes = opts->mask_mem == MVS_MEM_HOST ? align_up((size_t)plan.voxels) : 0;
    MvsWorkArea area(c);
    rc = area.alloc(3 * spec_bytes + stat_bytes + norm_bytes + max_bytes + peak_bytes + (r_out ? win_bytes : 0) + (n_out ? win_bytes : 0) + 2 * crop_bytes +
                    (fixed_mask ? mask_bytes : 0) + (moving_mask ? mask_bytes : 0));
    if (rc) return rc;
    char* cursor = (char*)area.ptr;
    auto take = [&](size_t nbytes) { char* p = cursor; cursor += nbytes; return p; };
    float2* Z[3];
    for (int k = 0; k < 3; ++k) Z[k] = (float2*)take(spec_bytes);
    StatPartial* d_stat = (StatPartial*)take(stat_bytes);
    CropNorm* d_norm = (CropNorm*)take(norm_bytes);
    MaxPartial* d_max = (MaxPartial*)take(max_bytes);
    PeakPartial* d_peak = (PeakPartial*)take(peak_bytes);
    float* d_r = r_out ? (float*)take(win_bytes) : nullptr;
    int* d_n = n_out ? (int*)take(win_bytes) : nullptr;
    Crops C;
    const float* im[2] = {fixed, moving};
    const uint8_t* mk[2] = {fixed_mask, moving_mask};
    for (int k = 0; k < 2; ++k) {
        C.im[k] = im[k];
        if (opts->mem == MVS_MEM_HOST) {
            float* d = (float*)take(crop_bytes);
            MVS_HIP_TRY(c, hipMemcpyAsync(d, im[k], (size_t)plan.voxels * 4, hipMemcpyHostToDevice, c->stream));
            C.im[k] = d;
        }
        C.mask[k] = mk[k];
        if (mk[k] && opts->mask_mem == MVS_MEM_HOST) {
            unsigned char* d = (unsigned char*)take(mask_bytes);
            MVS_HIP_TRY(c, hipMemcpyAsync(d, mk[k], (size_t)plan.voxels, hipMemcpyHostToDevice, c->stream));
            C.mask[k] = d;
        }
        C.has_thr[k] = opts->has_valid_above[k] ? 1 : 0;
        C.thr[k] = opts->has_valid_above[k] ? opts->valid_above[k] : 0.0;
    }
    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    hipLaunchKernelGGL(mc_stats_kernel, dim3(plan.voxel_blocks, 2), dim3(kThreads), 0, c->stream, C, D.voxels, d_stat);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(mc_stats_final_kernel, dim3(2), dim3(kThreads), 0, c->stream, (const StatPartial*)d_stat, plan.voxel_blocks, d_norm);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(mc_pack_kernel, dim3(plan.padded_blocks), dim3(kThreads), 0, c->stream, C, D, (const CropNorm*)d_norm, Z[0], Z[1], Z[2]);
    MVS_HIP_TRY(c, hipGetLastError());
    for (int k = 0; k < 3; ++k) {
        rc = mvs_fft3_c2c(c, Z[k], plan.P, false);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(mc_combine_kernel, dim3(plan.padded_blocks), dim3(kThreads), 0, c->stream, D, 1.f / (float)plan.padded, Z[0], Z[1], Z[2]);
    MVS_HIP_TRY(c, hipGetLastError());
    for (int k = 0; k < 3; ++k) {
        rc = mvs_fft3_c2c(c, Z[k], plan.P, true);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(mc_window_max_kernel, dim3(plan.window_blocks), dim3(kThreads), 0, c->stream, D, (const float2*)Z[0], (const float2*)Z[1],
                       (const float2*)Z[2], d_max);
    MVS_HIP_TRY(c, hipGetLastError());
    SearchArgs A;
    A.overlap_ratio = opts->overlap_ratio;
    A.min_overlap = opts->min_overlap;
    A.max_partials = d_max;
    A.n_max_partials = plan.window_blocks;
    A.r_out = d_r;
    A.n_out = d_n;
    hipLaunchKernelGGL(mc_window_search_kernel, dim3(plan.window_blocks), dim3(kThreads), 0, c->stream, D, A, (const float2*)Z[0], (const float2*)Z[1],
                       (const float2*)Z[2], d_peak);
    MVS_HIP_TRY(c, hipGetLastError());
    void *mh, *md;      // (asked for after the transforms: a mailbox is valid until the next request)
    rc = mvs_mailbox(c, sizeof(mvs_masked_corr_result_t), &mh, &md);
    if (rc) return rc;
    hipLaunchKernelGGL(mc_result_kernel, dim3(1), dim3(kThreads), 0, c->stream, D, A, (const float2*)Z[0], (const float2*)Z[1], (const float2*)Z[2],
                       (const PeakPartial*)d_peak, plan.window_blocks, (const CropNorm*)d_norm, (mvs_masked_corr_result_t*)md);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    if (r_out) MVS_HIP_TRY(c, hipMemcpyAsync(r_out, d_r, (size_t)plan.window * 4, hipMemcpyDeviceToHost, c->stream));
    if (n_out) MVS_HIP_TRY(c, hipMemcpyAsync(n_out, d_n, (size_t)plan.window * 4, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));      // (host crops and masks were copied from pageable memory of this call)
    *result = *(const mvs_masked_corr_result_t*)mh;
    return area.release();
}
