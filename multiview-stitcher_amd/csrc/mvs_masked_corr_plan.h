// mvs_masked_corr_plan.h -- host-only pure C++ of the masked normalised cross-correlation (mvs_masked_corr.hip): the padded shape
// of its transforms, the shift window and its wrapped indices, the limit and the launch geometry.  No HIP:
// tests/native/masked_corr_plan_host_test.cpp compiles it with the host compiler under the address and undefined-behaviour
// sanitizers.
#pragma once
#include <cstdint>

namespace mvs_masked_corr_plan {

constexpr long long kMaxVoxels = 1LL << 28;      // MVS_MASKED_CORR_MAX_VOXELS: three complex64 volumes of that many voxels are 6.4 GB
constexpr int kThreads = 256;                    // four waves per workgroup in every kernel of the file
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 1024;                 // grid cap of the grid-stride kernels = the most partials a reduction leaves

enum PlanCode { kPlanOk = 0, kPlanBadShape = 1, kPlanTooLarge = 2 };
// status of a result (mvs_masked_corr_result_t.status)
enum Status { kOk = 0, kNoEligibleShift = 1, kTooFewValid = 2, kConstantCrop = 3 };

// Smallest power of two >= n + S; 1 for an axis of one voxel.  The circular correlation of two sequences of n samples, zero-padded
// to that length, equals their linear correlation at every shift |s| <= S: x in [0, n) and x + s in [-S, n - 1 + S] leave the
// wrapped positions x + s + P >= P - S >= n and x + s - P <= n - 1 + S - P < 0 outside both supports.
inline long long padded_length(long long n, long long S) {
    if (n <= 1) return 1;
    long long p = 1;
    while (p < n + S) p <<= 1;
    return p;
}

inline int log2_of(long long p) {
    int l = 0;
    while ((1LL << l) < p) ++l;
    return l;
}

// Workgroups of a grid-stride launch over `items` items, one per thread and step: at least 1, at most kMaxBlocks.
inline int grid_blocks(long long items) {
    const long long want = (items + kThreads - 1) / kThreads;
    return (int)(want < 1 ? 1 : (want > kMaxBlocks ? kMaxBlocks : want));
}

struct Plan {
    int64_t n[3];          // crop shape z, y, x (2D: n[0] == 1)
    int64_t S[3];          // largest |shift| searched per axis
    int64_t P[3];          // padded (transform) shape
    int64_t W[3];          // the shift window: 2 S + 1 per axis
    long long voxels, padded, window;      // products of n, P, W
    int lp[3];             // log2 P
    int voxel_blocks, padded_blocks, window_blocks;
};

// max_shift (may be NULL): per axis the largest |shift| to search; a negative entry, or one above n - 1, means n - 1 (a shift of n or
// more leaves no overlap).  Every product is formed only while it is known to fit: n[k] <= 2^31 - 1, the running product <= 2^28.
inline PlanCode make_plan(int ndim, const int64_t shape[3], const int64_t* max_shift, Plan* out) {
    if ((ndim != 2 && ndim != 3) || !shape || !out) return kPlanBadShape;
    if (ndim == 2 && shape[0] != 1) return kPlanBadShape;
    Plan p{};
    p.voxels = p.padded = p.window = 1;
    for (int k = 0; k < 3; ++k) {
        if (shape[k] < 1 || shape[k] > 0x7fffffffLL) return kPlanBadShape;
        p.n[k] = shape[k];
        const long long most = shape[k] - 1;
        p.S[k] = (max_shift && max_shift[k] >= 0 && max_shift[k] < most) ? max_shift[k] : most;
        p.P[k] = padded_length(p.n[k], p.S[k]);
        p.W[k] = 2 * p.S[k] + 1;
        p.lp[k] = log2_of(p.P[k]);
        p.padded *= p.P[k];
        if (p.padded > kMaxVoxels) return kPlanTooLarge;
        p.voxels *= p.n[k];        // <= padded
        p.window *= p.W[k];        // 2 S + 1 <= n + S <= P: <= padded
    }
    p.voxel_blocks = grid_blocks(p.voxels);
    p.padded_blocks = grid_blocks(p.padded);
    p.window_blocks = grid_blocks(p.window);
    *out = p;
    return kPlanOk;
}

// the index along an axis of length P at which the circular correlation holds the shift s, -P < s < P
inline long long wrapped_index(long long s, long long P) { return s < 0 ? s + P : s; }

// flat index into the padded volume of the window entry w (first axis slowest, shifts ascending from -S)
inline long long window_to_padded(const Plan& p, long long w) {
    const long long wx = w % p.W[2], wy = (w / p.W[2]) % p.W[1], wz = w / (p.W[2] * p.W[1]);
    const long long iz = wrapped_index(wz - p.S[0], p.P[0]), iy = wrapped_index(wy - p.S[1], p.P[1]), ix = wrapped_index(wx - p.S[2], p.P[2]);
    return (iz * p.P[1] + iy) * p.P[2] + ix;
}

}  // namespace mvs_masked_corr_plan
