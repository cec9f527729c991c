// Host build of csrc/mvs_pair_metrics_dev.h: the reduction of mvs_pair_moments with its launch structure replayed on the CPU --
// 256 "threads" per workgroup in a grid-stride loop, shifted sums per thread, the shuffle tree of a wave, the waves of a workgroup in
// order, the records folded by 64 lanes in runs and merged in the same tree.  Prints the samples and the six moments.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mvs_pair_metrics_dev.h"

static PairMoments wave_tree(std::vector<PairMoments> r) {       // r[lane]; lane + off beyond the wave: the lane's own value, unused
    for (int off = 32; off >= 1; off >>= 1) {
        std::vector<PairMoments> nxt = r;
        for (int l = 0; l < 64; ++l) nxt[l] = pair_moments_merge(r[l], r[l + off < 64 ? l + off : l]);
        r = nxt;
    }
    return r[0];
}

static PairMoments reduce(const std::vector<float>& f, const std::vector<float>& m) {
    const long long n = (long long)f.size();
    long long nblocks = (n + kPairBlockThreads - 1) / kPairBlockThreads;
    if (nblocks > kPairMaxBlocks) nblocks = kPairMaxBlocks;
    std::vector<PairMoments> records;
    for (long long b = 0; b < nblocks; ++b) {
        std::vector<PairMoments> waves;
        for (int w = 0; w < kPairBlockThreads / 64; ++w) {
            std::vector<PairMoments> lanes;
            for (int l = 0; l < 64; ++l) {
                PairSums s{0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (long long i = b * kPairBlockThreads + w * 64 + l; i < n; i += nblocks * kPairBlockThreads)
                    if (f[i] == f[i] && m[i] == m[i]) pair_sums_add(s, f[i], m[i]);
                lanes.push_back(pair_sums_to_moments(s));
            }
            waves.push_back(wave_tree(lanes));
        }
        PairMoments r = waves[0];
        for (size_t w = 1; w < waves.size(); ++w) r = pair_moments_merge(r, waves[w]);
        records.push_back(r);
    }
    const int R = (int)records.size(), run = (R + 63) / 64;
    std::vector<PairMoments> lanes;
    for (int l = 0; l < 64; ++l) {
        PairMoments r = pair_moments_empty();
        for (int i = l * run; i < (l + 1) * run && i < R; ++i) r = pair_moments_merge(r, records[i]);
        lanes.push_back(r);
    }
    return wave_tree(lanes);
}

int main() {
    // 16-bit camera values at 60000 +- a few counts, half a count apart (exact in float32), 3 workgroups and 5 samples
    uint64_t state = 12345;
    auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (int)((state >> 33) % 13) - 6; };
    for (int variant = 0; variant < 3; ++variant) {
        const int n = variant == 2 ? kPairMaxBlocks * kPairBlockThreads + 1234 : 3 * kPairBlockThreads + 5;
        std::vector<float> f(n), m(n);
        for (int i = 0; i < n; ++i) {
            const int c = next();
            f[i] = variant == 1 ? 60123.0f : 60000.0f + (float)c + 0.5f * (float)next();
            m[i] = 60000.0f + (float)c + 0.5f * (float)next();
            if (i % 97 == 13) m[i] = 0.0f / 0.0f;
        }
        const PairMoments r = reduce(f, m);
        printf("M %d %d %.17g %.17g %.17g %.17g %.17g %.17g\n", variant, n, r.n, r.mean_f, r.mean_m, r.m2_f, r.m2_m, r.c_fm);
        if (variant == 0)
            for (int i = 0; i < n; ++i) printf("S %.9g %.9g\n", f[i], m[i]);
    }
    printf("done\n");
    return 0;
}
