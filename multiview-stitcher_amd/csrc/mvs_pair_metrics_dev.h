// mvs_pair_metrics_dev.h -- the moment records of mvs_pair_moments and the arithmetic that folds them, host/device: the kernels
// (mvs_pair_metrics.hip) and tests/native/pair_moments_host_test.cpp compile the same functions.
#pragma once
#include <hip/hip_runtime.h>

#define MVS_HD __host__ __device__ __forceinline__

constexpr int kPairBlockThreads = 256;   // one voxel per thread and step of the grid-stride loop
constexpr int kPairMaxBlocks = 2048;     // workgroups of one launch = min(ceil(voxels / 256), 2048): a function of the voxel count only

// (n, mean_f, mean_m, M2_f, M2_m, C_fm) of a set of sample pairs: M2 = sum of squared deviations from the mean, C = sum of the
// products of the two deviations.  n is kept as a double (exact up to 2^53).
struct PairMoments {
    double n, mean_f, mean_m, m2_f, m2_m, c_fm;
    // a partial of mvs_fold_dev.h: merge is pair_moments_merge(*this, b)
    __device__ __forceinline__ void merge(const PairMoments& b);
    template <typename S> __device__ __forceinline__ PairMoments shuffled(S sh, int off) const {
        return PairMoments{sh(n, off), sh(mean_f, off), sh(mean_m, off), sh(m2_f, off), sh(m2_m, off), sh(c_fm, off)};
    }
};

MVS_HD PairMoments pair_moments_empty() { return PairMoments{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

// What one thread gathered: sums of the samples shifted by its own first valid pair (f0, m0), so that neither the mean nor the
// spread of a tile with a large offset (a 16-bit camera at 60000 +- 3) is lost, and a constant tile gives sums of exact zeros.
struct PairSums {
    long long n;
    double f0, m0, sf, sm, sff, smm, sfm;
};

MVS_HD void pair_sums_add(PairSums& s, float f, float m) {
    if (s.n == 0) {
        s.f0 = (double)f;
        s.m0 = (double)m;
    }
    const double df = (double)f - s.f0, dm = (double)m - s.m0;     // differences of two floats: exact in double
    s.n += 1;
    s.sf += df;
    s.sm += dm;
    s.sff += df * df;
    s.smm += dm * dm;
    s.sfm += df * dm;
}

MVS_HD PairMoments pair_sums_to_moments(const PairSums& s) {
    if (s.n == 0) return pair_moments_empty();
    const double n = (double)s.n;
    PairMoments r;
    r.n = n;
    r.mean_f = s.f0 + s.sf / n;
    r.mean_m = s.m0 + s.sm / n;
    // sum (d - mean d)^2 = sum d^2 - (sum d)^2 / n; with the shift this subtracts numbers of the size of the result, and it is
    // never taken below zero (Cauchy-Schwarz holds up to rounding)
    const double m2f = s.sff - s.sf * s.sf / n, m2m = s.smm - s.sm * s.sm / n;
    r.m2_f = m2f > 0.0 ? m2f : 0.0;
    r.m2_m = m2m > 0.0 ? m2m : 0.0;
    r.c_fm = s.sfm - s.sf * s.sm / n;
    return r;
}

// Pairwise update of Chan, Golub and LeVeque (1979): the moments of the union of two disjoint sets.  `a` is the left operand of
// every tree below (lower lane, lower wave, lower record index); an empty side leaves the other unchanged, bit for bit.
MVS_HD PairMoments pair_moments_merge(const PairMoments& a, const PairMoments& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    PairMoments r;
    const double n = a.n + b.n;
    const double df = b.mean_f - a.mean_f, dm = b.mean_m - a.mean_m;
    const double w = a.n * b.n / n;
    r.n = n;
    r.mean_f = a.mean_f + df * (b.n / n);
    r.mean_m = a.mean_m + dm * (b.n / n);
    r.m2_f = (a.m2_f + b.m2_f) + df * df * w;
    r.m2_m = (a.m2_m + b.m2_m) + dm * dm * w;
    r.c_fm = (a.c_fm + b.c_fm) + df * dm * w;
    return r;
}
__device__ __forceinline__ void PairMoments::merge(const PairMoments& b) { *this = pair_moments_merge(*this, b); }
