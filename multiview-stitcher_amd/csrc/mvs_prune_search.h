// mvs_prune_search.h -- the host arithmetic of the pruned arg-max search of the candidate scoring (mvs_score.hip), and the
// geometry of the fused SSIM walk that the search and the kernels share.  No HIP header, no MvsContext: a plain host compile
// takes it (tests/native/prune_search_host_test.cpp drives the search with a fake walk).
#pragma once

#include <algorithm>
#include <cmath>

#if defined(__HIPCC__)
#define MVS_WALK_HD __host__ __device__
#else
#define MVS_WALK_HD
#endif

// ---- work items of the fused walk (ssim_fused_batch_body, ssim_fixed_walk_kernel) ---------------------------------------------
// A work item is a TY x TX tile of the cropped interior (crop = PAD per side) of one z segment of `zseg` planes, numbered x
// fastest.  The pruned search walks a candidate in K-ths: residue r of group g (items g K .. g K + K - 1) is item
// g K + (r + kSelRot g) mod K.  Without the rotation a residue class of a crop with 16 tiles per z segment (x neighbours:
// 256 x 256 x 51) is ONE tile row -- class 0 the row along the crop's border -- and the first 1 / 32 of a candidate says
// little about the rest of it (a wrong leader is completed, the others are walked further than needed).
constexpr int kSelRot = 7;

struct WalkItem { int tx, ty, zs, z0, z1, y0, x0; };      // tile and segment numbers; first / end plane; first row / column

template <int WIN>
struct WalkGeom {
    static constexpr int TY = 16, TX = 56, H = WIN / 2, PAD = (WIN - 1) / 2;
    static constexpr int kMinSeg = 8;                      // a z segment is not planned shorter (every segment re-reads WIN - 1 halo planes)
    int nz, ny, nx, zseg, cz, cy, cx, nty, ntx, nzs, nitems;

    MVS_WALK_HD static constexpr int crop(int n) { return n - 2 * PAD; }
    MVS_WALK_HD static constexpr int lesser(int a, int b) { return a < b ? a : b; }
    MVS_WALK_HD static constexpr int tiles(int ny, int nx) { return ((crop(ny) + TY - 1) / TY) * ((crop(nx) + TX - 1) / TX); }
    MVS_WALK_HD WalkGeom(int nz_, int ny_, int nx_, int zseg_)
        : nz(nz_), ny(ny_), nx(nx_), zseg(zseg_), cz(crop(nz_)), cy(crop(ny_)), cx(crop(nx_)), nty((cy + TY - 1) / TY), ntx((cx + TX - 1) / TX),
          nzs((cz + zseg_ - 1) / zseg_), nitems(nty * ntx * nzs) {}
    MVS_WALK_HD WalkItem item(int i) const {
        WalkItem w;
        w.tx = i % ntx; w.ty = (i / ntx) % nty; w.zs = i / (ntx * nty);
        w.z0 = PAD + w.zs * zseg;
        w.z1 = lesser(w.z0 + zseg, nz - PAD);
        w.y0 = PAD + w.ty * TY; w.x0 = PAD + w.tx * TX;
        return w;
    }
    // the item that is residue `res` of group `grp` (in two parts: the walk kernel adds them itself, multiply first, so that its
    // instructions stay in the order they have been tuned and measured in), and the residue class an item belongs to
    MVS_WALK_HD static int group_first(int grp, int K) { return grp * K; }
    MVS_WALK_HD static int rotated(int res, int grp, int K) { return (res + kSelRot * grp) % K; }
    MVS_WALK_HD static int item_of(int grp, int res, int K) { return group_first(grp, K) + rotated(res, grp, K); }
    MVS_WALK_HD static int residue_of(int item, int K) { return (((item % K) - kSelRot * (item / K)) % K + K) % K; }
    // output voxels of an item (the last tile of a row / column and the last segment may be partial)
    MVS_WALK_HD double voxels(int i) const {
        const WalkItem w = item(i);
        return (double)(w.z1 - w.z0) * (double)lesser(TY, cy - w.ty * TY) * (double)lesser(TX, cx - w.tx * TX);
    }
    // segment length that gives about `budget` work items to `sharers` walks of this volume in one launch
    static int zseg_for(int nz, int ny, int nx, int budget, int sharers = 1) {
        const int cz = crop(nz);
        const int nzs = std::max(1, std::min(budget / std::max(tiles(ny, nx) * sharers, 1), (cz + kMinSeg - 1) / kMinSeg));
        return (cz + nzs - 1) / nzs;
    }
};

// ---- the pruned arg-max search --------------------------------------------------------------------------------------------------
// The SSIM of a candidate is the mean of per-voxel values S <= 1 (S = l * cs with l <= 1 by the AM-GM inequality and |cs| <= 1 by
// Cauchy-Schwarz; the float32 window means move a variance by at most a few 2^-23 M^2, M the largest value, against
// C2 = (0.03 R)^2 in the denominator: S <= 1 + slack).  So once ONE candidate is scored completely (sum S*), a candidate with
// partial sum p over n of the N voxels can at best reach p + (N - n)(1 + slack); if that is below S* it cannot be the arg max,
// whatever the rest of its volume holds -- the reference's nanargmax picks the same candidate, and the Spearman coefficient is
// only ever evaluated for that one.  All candidates are walked on 1 / K of the work items (spread over the volume), the leader
// is completed, the others continue in rounds only while their bound still reaches the best complete sum.  On the bench mosaic
// the decorrelated candidates (mean 0.01-0.15 against 0.90-0.975) leave after 3/32-8/32 of their volume, the sign flips of a
// half-pixel axis (0.6-0.94) after 6/32-22/32: 2.6 instead of 9.2 candidate volumes per pair (profiles/round4_prune_ab.txt).
//
// A candidate whose region maximum does not exceed im1_min is the reference's `continue` case (registration.py:530-533): it takes
// no part in the arg max, so its sum must never be the one the others are dropped against (against a sparse fixed image an
// all-background candidate can hold the highest sum).  Complete candidates know their maximum; the leader is re-elected among
// the open candidates when it turns out to be such a candidate.
//
// margin > 0: the rounds are walked in float32 and the complete candidates that end within `margin` (mean SSIM) of the best are
// walked again in float64 when there are two or more of them; candidates are dropped only when their bound stays below the best
// sum by it.  The arg max is the reference's if the float32 MEAN of every candidate is within margin / 2 of its float64 value: a
// dropped candidate was more than the margin below the best in float32, so it is below it in float64; so is a complete one that
// is not walked again; and the arg max compares float64 sums of the re-walked with float32 sums of the others, which are more than
// margin - margin / 2 apart.  A float32 window variance is off by a few 1e-7 (values rescaled to [0, 1], sums restarted per
// segment) against C2 = 9e-4 in the denominator.  Measured against the oracle (tests/test_ssim_f32_walk_gpu.py, table in DESIGN.md
// 3.3): the mean is off by +1.0e-4 to +1.25e-4 on a bright flat background (level 0.9-0.97 of the range, texture 0.005-0.02), the
// same for z segments of 7, 13 and 24 planes, by 1e-6 on mid-level texture -- a quarter of the margin / 2 = 5e-4 that
// kPruneMarginF32 = 1e-3 allows.  The search keeps the sum the rounds ended with (round_sum) next to the re-walk's.
//
// Use: while (s.next_round(masks)) { walk candidate j on the residue classes masks[j] (in float64 when s.rewalk()); s.take(...) }
constexpr int kPruneMaxCand = 16;
constexpr double kPruneMarginF32 = 1e-3;

// vol_res[r]: output voxels of the work items of residue class r (the kernel's own geometry)
template <int WIN>
inline void prune_residue_volumes(const WalkGeom<WIN>& g, int K, double vol_res[32]) {
    for (int r = 0; r < 32; ++r) vol_res[r] = 0.0;
    for (int item = 0; item < g.nitems; ++item) vol_res[WalkGeom<WIN>::residue_of(item, K)] += g.voxels(item);
}

class PruneSearch {
public:
    PruneSearch(int n, const bool* takes_part, int K, const double vol_res[32], double Ntot, double slack, double margin, double im1_min)
        : nb(n), K(K), kAll(K == 32 ? 0xffffffffu : 0xffffu), Ntot(Ntot), slack(slack), margin(margin), im1_min(im1_min) {
        for (int r = 0; r < 32; ++r) this->vol_res[r] = vol_res[r];
        for (int j = 0; j < kPruneMaxCand; ++j) {
            in[j] = j < n && takes_part[j];
            acc[j] = 0.0; amx[j] = -INFINITY; ahn[j] = 0; done[j] = 0; masks[j] = 0; dropped[j] = false; again[j] = false; ub[j] = 0.0; racc[j] = 0.0;
        }
    }

    // the residue classes every candidate walks next (0: none); false when the search is over
    bool next_round(unsigned int out[kPruneMaxCand]) {
        bool more = false;
        if (phase == kFirst) {
            for (int j = 0; j < nb; ++j) { masks[j] = in[j] ? 0x0001u : 0u; more = more || in[j]; }
        } else if (phase == kRounds && round < 34) {
            more = plan();
        }
        if (!more && phase != kFirst && phase != kOver) {
            more = phase == kRounds && select_rewalk();
            phase = more ? kRewalk : kOver;
        }
        for (int j = 0; j < kPruneMaxCand; ++j) out[j] = more ? masks[j] : 0u;
        return more;
    }
    bool rewalk() const { return phase == kRewalk; }

    // what the round handed out last gave: the sum of the per-voxel values, the maximum and the has-NaN flag per candidate
    void take(const double* sum, const float* mx, const int* hasnan) {
        for (int j = 0; j < nb; ++j) {
            if (!masks[j]) continue;
            acc[j] += sum[j];
            amx[j] = fmaxf(amx[j], mx[j]);
            ahn[j] |= hasnan[j];
            done[j] |= masks[j];
            masks[j] = 0;
        }
        if (phase == kFirst) { leader = elect(); phase = kRounds; round = 0; }
        else if (phase == kRounds) { drop(); ++round; }
        else phase = kOver;
    }

    // per candidate, once next_round() has returned false
    double sum(int j) const { return dropped[j] ? ub[j] : acc[j]; }      // dropped: the bound it could not exceed (< the best sum)
    float maximum(int j) const { return amx[j]; }
    int hasnan(int j) const { return ahn[j]; }
    bool pruned(int j) const { return dropped[j]; }
    bool rewalked(int j) const { return again[j]; }
    double round_sum(int j) const { return again[j] ? racc[j] : acc[j]; }      // the sum the rounds ended with (a re-walk replaces acc)
    double volume_fraction(int j) const { return vol_of(done[j]) / Ntot; }      // of the rounds (a re-walk is one more volume)
    // for the debug line
    int classes_done(int j) const { return __builtin_popcount(done[j]); }
    double mean(int j) const { return mean_of(j); }
    bool has_best() const { return have_best; }
    double best_sum() const { return s_best; }

private:
    enum Phase { kFirst, kRounds, kRewalk, kOver };
    int nb, K;
    unsigned int kAll;
    double vol_res[32], Ntot, slack, margin, im1_min;
    bool in[kPruneMaxCand], dropped[kPruneMaxCand], again[kPruneMaxCand];
    double acc[kPruneMaxCand], ub[kPruneMaxCand], racc[kPruneMaxCand];
    float amx[kPruneMaxCand];
    int ahn[kPruneMaxCand];
    unsigned int done[kPruneMaxCand], masks[kPruneMaxCand];
    Phase phase = kFirst;
    int round = 0, leader = -1;
    bool have_best = false;
    double s_best = 0.0;

    double vol_of(unsigned int m) const { double v = 0.0; for (int r = 0; r < 32; ++r) if ((m >> r) & 1u) v += vol_res[r]; return v; }
    bool excluded(int j) const { return done[j] == kAll && !((double)amx[j] > im1_min); }
    double mean_of(int j) const { return acc[j] / std::max(vol_of(done[j]), 1.0); }
    int elect() const {
        int l = -1;
        for (int j = 0; j < nb; ++j)
            if (in[j] && !excluded(j) && !(done[j] == kAll && !std::isfinite(acc[j])) && (l < 0 || mean_of(j) > mean_of(l))) l = j;
        return l;
    }
    // Plan: the leader is completed; every other open candidate advances to the fraction at which its bound would fall below the
    // reference sum if its mean stayed what it is so far (residues are taken in rising order; the reference is the best complete
    // sum, before there is one the leader's extrapolated sum -- a guess that only sizes the round: candidates are dropped against
    // complete sums alone).
    bool plan() {
        if (!have_best && (leader < 0 || done[leader] == kAll)) leader = elect();      // the leader was a `continue` candidate / NaN
        const double s_ref = have_best ? s_best : leader >= 0 ? mean_of(leader) * Ntot : Ntot * (1.0 + slack);
        bool more = false;
        for (int j = 0; j < nb; ++j) {
            if (!in[j] || done[j] == kAll || dropped[j]) continue;
            const int k_done = __builtin_popcount(done[j]);
            int k_to = K;
            if (j != leader && (double)amx[j] > im1_min) {
                const double mean_c = acc[j] / std::max(vol_of(done[j]), 1.0);
                const double den = (1.0 + slack) - mean_c;
                const double f = den > 0.0 ? ((1.0 + slack) - s_ref / Ntot) / den : 2.0;
                if (f < 1.0) k_to = std::min(K, std::max(k_done + 1, (int)std::ceil((double)K * f * 1.15 + 0.25)));
                if (4 * k_to >= 3 * K) k_to = K;
            }
            masks[j] = (unsigned int)((1ull << k_to) - 1ull) & ~(unsigned int)((1ull << k_done) - 1ull);
            more = true;
        }
        return more;
    }
    void drop() {
        for (int j = 0; j < nb; ++j)
            if (in[j] && done[j] == kAll && !excluded(j) && std::isfinite(acc[j]) && (!have_best || acc[j] > s_best)) {
                s_best = acc[j];
                have_best = true;
            }
        for (int j = 0; j < nb; ++j) {
            if (!in[j] || done[j] == kAll || dropped[j]) continue;
            // (a candidate whose samples so far do not exceed im1_min may still be the reference's `continue` case: in full;
            // without a reference sum -- the completed leader was such a candidate or NaN -- nothing is dropped)
            ub[j] = acc[j] + (Ntot - vol_of(done[j])) * (1.0 + slack);
            if (have_best && (double)amx[j] > im1_min && ub[j] < s_best - (1e-9 + margin) * Ntot) dropped[j] = true;
        }
    }
    // the complete candidates within the margin of the best float32 sum: with two or more of them the arg max is decided by their
    // float64 sums (whole volume, fresh accumulators)
    bool near_best(int j) const {
        return in[j] && done[j] == kAll && !dropped[j] && !excluded(j) && std::isfinite(acc[j]) && acc[j] >= s_best - margin * Ntot;
    }
    bool select_rewalk() {
        if (!(margin > 0.0) || !have_best) return false;
        int near = 0;
        for (int j = 0; j < nb; ++j) near += near_best(j) ? 1 : 0;
        if (near < 2) return false;
        for (int j = 0; j < nb; ++j) {
            again[j] = near_best(j);
            masks[j] = again[j] ? kAll : 0u;
        }
        for (int j = 0; j < nb; ++j) if (again[j]) { racc[j] = acc[j]; acc[j] = 0.0; }
        return true;
    }
};
