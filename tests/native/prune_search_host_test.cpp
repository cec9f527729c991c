// Host-side check of csrc/mvs_prune_search.h: the pruned arg-max search of the candidate scoring, driven by a fake walk instead
// of the SSIM kernels, and the work-item geometry it shares with them.  The fake walk holds, per candidate, one per-voxel value
// per work item (a multiple of 2^-10 that never exceeds 1 + slack, so every sum is exact in any order) and walks the items of
// the residue classes it is handed by the kernel's own rule (WalkGeom::item_of).  Built and run by
// tests/test_prune_search_host.py with hipcc as a host compiler (no GPU needed).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mvs_prune_search.h"

typedef WalkGeom<7> G;
static const int N = kPruneMaxCand;

struct Rng {
    unsigned long long s;
    unsigned next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); }
    int below(int n) { return (int)(next() % (unsigned)n); }
    bool chance(int percent) { return below(100) < percent; }
};

struct Case {
    const char* name;
    int nz, ny, nx, zseg, K, n;
    bool in[N];
    double slack, margin, im1_min;
    // per candidate and work item: the per-voxel value of the float32 walk (v[0]) and of the float64 walk (v[1]; the same
    // without a margin), and the largest sample of the candidate image there
    std::vector<double> v[2][N];
    std::vector<float> mx[N];
    std::vector<int> hn[N];
    int expect_winner = -1, expect_rewalks = -1;      // hand-made cases: the arg max and the number of re-walked candidates
};

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { printf("FAIL %s (%dx%dx%d zseg %d K %d n %d): ", C.name, C.nz, C.ny, C.nx, C.zseg, C.K, C.n); printf(__VA_ARGS__); printf("\n"); } return; } } while (0)

static void walk(const Case& C, const G& g, const unsigned int* masks, int prec, double* sum, float* mx, int* hn) {
    const int ngroups = (g.nitems + C.K - 1) / C.K;
    for (int j = 0; j < C.n; ++j) {
        sum[j] = 0.0; mx[j] = -INFINITY; hn[j] = 0;
        if (!masks[j]) continue;
        for (int grp = 0; grp < ngroups; ++grp)
            for (int r = 0; r < C.K; ++r) {
                if (!((masks[j] >> r) & 1u)) continue;
                const int item = G::item_of(grp, r, C.K);
                if (item >= g.nitems) continue;
                sum[j] += C.v[prec][j][item] * g.voxels(item);
                mx[j] = fmaxf(mx[j], C.mx[j][item]);
                hn[j] |= C.hn[j][item];
            }
    }
}

static void run(const Case& C) {
    const G g(C.nz, C.ny, C.nx, C.zseg);
    const double Ntot = (double)g.cz * (double)g.cy * (double)g.cx;
    // ---- geometry: the residue volumes the search is given against the items the walk visits ----
    double vol_res[32];
    prune_residue_volumes(g, C.K, vol_res);
    {
        double tot = 0.0, fwd[32];
        for (int r = 0; r < 32; ++r) { tot += vol_res[r]; fwd[r] = 0.0; }
        CHECK(tot == Ntot, "residue volumes add up to %.0f, the cropped interior holds %.0f", tot, Ntot);
        std::vector<int> seen((size_t)g.nitems, 0);
        double cover = 0.0;
        for (int grp = 0; grp < (g.nitems + C.K - 1) / C.K; ++grp)
            for (int r = 0; r < C.K; ++r) {
                const int item = G::item_of(grp, r, C.K);
                CHECK(item >= grp * C.K && item < (grp + 1) * C.K, "item %d of group %d", item, grp);
                if (item >= g.nitems) continue;
                CHECK(G::residue_of(item, C.K) == r, "item %d: walked as residue %d, counted as residue %d", item, r, G::residue_of(item, C.K));
                const WalkItem w = g.item(item);
                const int ylen = std::min(w.y0 + G::TY, C.ny - G::PAD) - w.y0, xlen = std::min(w.x0 + G::TX, C.nx - G::PAD) - w.x0;
                CHECK(w.z1 > w.z0 && ylen > 0 && xlen > 0 && w.z1 <= C.nz - G::PAD, "item %d is empty or leaves the interior", item);
                CHECK(g.voxels(item) == (double)(w.z1 - w.z0) * ylen * xlen, "item %d: %.0f voxels", item, g.voxels(item));
                fwd[r] += g.voxels(item);
                cover += g.voxels(item);
                ++seen[(size_t)item];
            }
        for (int i = 0; i < g.nitems; ++i) CHECK(seen[(size_t)i] == 1, "item %d walked %d times", i, seen[(size_t)i]);
        CHECK(cover == Ntot, "the items hold %.0f voxels of %.0f", cover, Ntot);
        for (int r = 0; r < 32; ++r) CHECK(fwd[r] == vol_res[r], "residue %d: %.0f voxels walked, %.0f counted", r, fwd[r], vol_res[r]);
    }
    // ---- the complete sums ----
    const unsigned int all = C.K == 32 ? 0xffffffffu : 0xffffu;
    unsigned int every[N];
    for (int j = 0; j < N; ++j) every[j] = all;
    double full[2][N];
    float fmx[N];
    int fhn[N];
    walk(C, g, every, 0, full[0], fmx, fhn);
    walk(C, g, every, 1, full[1], fmx, fhn);
    bool elig[N];
    bool any_elig = false;
    double best[2] = {-INFINITY, -INFINITY};
    for (int j = 0; j < C.n; ++j) {
        elig[j] = C.in[j] && (double)fmx[j] > C.im1_min && std::isfinite(full[0][j]) && std::isfinite(full[1][j]);
        if (elig[j]) { any_elig = true; best[0] = std::max(best[0], full[0][j]); best[1] = std::max(best[1], full[1][j]); }
    }
    // ---- the search ----
    PruneSearch s(C.n, C.in, C.K, vol_res, Ntot, C.slack, C.margin, C.im1_min);
    unsigned int masks[N];
    int rounds = 0;
    bool rewalk_seen = false;
    while (s.next_round(masks)) {
        CHECK(++rounds <= 37, "no end after %d rounds", rounds);
        CHECK(!rewalk_seen, "a round after the re-walk");
        rewalk_seen = s.rewalk();
        CHECK(!rewalk_seen || C.margin > 0.0, "re-walk without a margin");
        bool some = false;
        for (int j = 0; j < N; ++j) {
            CHECK(!masks[j] || (j < C.n && C.in[j]), "candidate %d takes no part and is walked", j);
            CHECK((masks[j] & ~all) == 0, "candidate %d: classes %08x of %d", j, masks[j], C.K);
            some = some || masks[j];
        }
        CHECK(some, "an empty round");
        double sum[N];
        float mx[N];
        int hn[N];
        walk(C, g, masks, (C.margin > 0.0 && !s.rewalk()) ? 0 : 1, sum, mx, hn);
        s.take(sum, mx, hn);
        if (s.has_best()) {      // the reference sum is the complete sum of a candidate that takes part in the arg max
            bool found = false;
            for (int j = 0; j < C.n; ++j) found = found || (elig[j] && full[C.margin > 0.0 ? 0 : 1][j] == s.best_sum());
            CHECK(found, "reference sum %.17g is no eligible candidate's complete sum", s.best_sum());
        }
    }
    const int p = C.margin > 0.0 ? 0 : 1;      // precision of the rounds
    int winner = -1;
    for (int j = 0; j < C.n; ++j) {
        if (!C.in[j]) { CHECK(!s.pruned(j) && !s.rewalked(j) && s.sum(j) == 0.0, "candidate %d takes no part", j); continue; }
        CHECK(s.rewalked(j) == (rewalk_seen && s.rewalked(j)), "candidate %d", j);
        if (s.pruned(j)) {
            CHECK(any_elig && s.sum(j) < best[p], "candidate %d dropped with bound %.17g, best complete sum %.17g", j, s.sum(j), best[p]);
            CHECK(!(full[p][j] > s.sum(j)), "candidate %d: bound %.17g below its sum %.17g", j, s.sum(j), full[p][j]);
            CHECK(!s.rewalked(j), "candidate %d dropped and walked again", j);
            continue;
        }
        CHECK(s.volume_fraction(j) == 1.0, "candidate %d neither complete nor dropped (%.4f)", j, s.volume_fraction(j));
        CHECK(s.maximum(j) == fmx[j] && s.hasnan(j) == fhn[j], "candidate %d: region statistics", j);
        const double want = full[s.rewalked(j) ? 1 : p][j];
        CHECK(s.sum(j) == want || (want != want && s.sum(j) != s.sum(j)), "candidate %d: sum %.17g, complete sum %.17g", j, s.sum(j), want);
        // the sum the rounds ended with survives the re-walk: the float32 complete sum next to the float64 one that replaced it
        if (s.rewalked(j)) {
            CHECK(s.round_sum(j) == full[0][j], "candidate %d: kept round sum %.17g, float32 complete sum %.17g", j, s.round_sum(j), full[0][j]);
            CHECK(s.sum(j) == full[1][j], "candidate %d: sum after the re-walk %.17g, float64 complete sum %.17g", j, s.sum(j), full[1][j]);
        } else {
            CHECK(s.round_sum(j) == s.sum(j) || (s.sum(j) != s.sum(j) && s.round_sum(j) != s.round_sum(j)), "candidate %d: round sum %.17g, sum %.17g", j, s.round_sum(j), s.sum(j));
        }
        if (!((double)s.maximum(j) > C.im1_min) || !std::isfinite(s.sum(j))) continue;      // the reference's `continue` / no number
        if (winner < 0 || s.sum(j) > s.sum(winner)) winner = j;
    }
    CHECK((winner >= 0) == any_elig, "winner %d", winner);
    if (winner >= 0) {
        CHECK(elig[winner] && full[1][winner] == best[1], "winner %d holds %.17g, the arg max holds %.17g", winner, full[1][winner], best[1]);
        CHECK(s.has_best(), "no reference sum");
    }
    int nrewalk = 0;
    for (int j = 0; j < C.n; ++j) nrewalk += s.rewalked(j) ? 1 : 0;
    CHECK(C.expect_winner < 0 || winner == C.expect_winner, "winner %d, expected %d", winner, C.expect_winner);
    CHECK(C.expect_rewalks < 0 || nrewalk == C.expect_rewalks, "%d candidates re-walked, expected %d", nrewalk, C.expect_rewalks);
    if (C.margin > 0.0) {      // who is walked again: the complete candidates within the margin of the best float32 sum, if two or more
        int near = 0;
        for (int j = 0; j < C.n; ++j) near += (elig[j] && !s.pruned(j) && full[0][j] >= best[0] - C.margin * Ntot) ? 1 : 0;
        for (int j = 0; j < C.n; ++j) {
            const bool want = near >= 2 && elig[j] && !s.pruned(j) && full[0][j] >= best[0] - C.margin * Ntot;
            CHECK(s.rewalked(j) == want, "candidate %d: re-walked %d, expected %d (%d near the best)", j, (int)s.rewalked(j), (int)want, near);
        }
    }
}

// ---- cases ----
static void shape(Case& C, int nz, int ny, int nx, int zseg, int K, int n) {
    C.nz = nz; C.ny = ny; C.nx = nx; C.zseg = zseg; C.K = K; C.n = n;
    const G g(nz, ny, nx, zseg);
    for (int j = 0; j < N; ++j) {
        C.in[j] = j < n;
        for (int q = 0; q < 2; ++q) C.v[q][j].assign((size_t)g.nitems, 0.0);
        C.mx[j].assign((size_t)g.nitems, 1.f);
        C.hn[j].assign((size_t)g.nitems, 0);
    }
}
static void fill(Case& C, int j, double value) { for (double& x : C.v[0][j]) x = value; C.v[1][j] = C.v[0][j]; }
static void fill_class(Case& C, int j, int r, double value) {      // the items of residue class r
    for (size_t i = 0; i < C.v[0][j].size(); ++i) if (G::residue_of((int)i, C.K) == r) C.v[0][j][i] = C.v[1][j][i] = value;
}

static const int kShapes[][4] = {      // nz, ny, nx, zseg: partial last tiles, one item, fewer items than K, the bench crop
    {51, 256, 256, 8}, {51, 256, 256, 12}, {20, 40, 70, 5}, {7, 7, 7, 1}, {9, 22, 62, 3}, {30, 23, 63, 7}, {13, 38, 118, 2}, {40, 100, 180, 9}, {8, 54, 174, 1}, {64, 39, 62, 4},
};

static void handmade(int K) {
    const double q = 1.0 / 1024.0;
    for (const auto& sh : kShapes) {
        Case C;
        C.slack = 1.0 / 32.0; C.margin = 0.0; C.im1_min = 0.25;
        // background-only candidate 0 (no sample above im1_min) holds the highest sum and is the first leader
        C.name = "background first leader"; shape(C, sh[0], sh[1], sh[2], sh[3], K, 4);
        fill(C, 0, 1.0); for (float& m : C.mx[0]) m = 0.25f;
        fill(C, 1, 922 * q); fill(C, 2, 512 * q); fill(C, 3, 900 * q);
        C.expect_winner = 1; C.expect_rewalks = 0;
        run(C);
        // ... holds the highest sum, but not on the first class
        C.name = "background late leader"; fill_class(C, 0, 0, 100 * q);
        run(C);
        // ... and a candidate whose samples exceed im1_min only in its last class
        C.expect_winner = -1;
        C.name = "late maximum"; for (size_t i = 0; i < C.mx[2].size(); ++i) C.mx[2][i] = G::residue_of((int)i, K) == K - 1 ? 1.f : 0.f;
        run(C);
        // a NaN sum in the class every candidate starts with, on the first candidate
        C.name = "NaN first leader"; shape(C, sh[0], sh[1], sh[2], sh[3], K, 3);
        fill(C, 0, 1.0); fill_class(C, 0, 0, NAN); fill(C, 1, 700 * q); fill(C, 2, 800 * q);
        C.expect_winner = 2;
        run(C);
        C.name = "NaN late"; fill(C, 0, 1.0); fill_class(C, 0, G::residue_of((int)C.v[0][0].size() - 1, K), NAN);
        run(C);
        // values that reach 1 + slack: candidate 1 starts at 0 and holds 1 + slack everywhere else
        C.name = "values at 1 + slack"; shape(C, sh[0], sh[1], sh[2], sh[3], K, 3);
        // (on the larger grids candidate 1 is the arg max, and a bound that counted the rest of it as 1 would drop it)
        C.slack = 1.0 / 16.0;
        fill(C, 0, 1.0 - 0.5 / K); fill(C, 1, 1.0 + C.slack); fill_class(C, 1, 0, 0.0); fill(C, 2, 300 * q);
        C.expect_winner = -1;
        run(C);
        C.slack = 1.0 / 32.0;
        // float32 walk: two candidates within the margin, in the wrong order
        C.margin = kPruneMarginF32;
        C.name = "near tie, wrong order"; shape(C, sh[0], sh[1], sh[2], sh[3], K, 4);
        fill(C, 0, 300 * q); fill(C, 1, 920 * q); fill(C, 2, 920 * q); fill(C, 3, 600 * q);
        for (double& x : C.v[0][1]) x += q / 4; for (double& x : C.v[1][2]) x += q / 8;
        C.expect_winner = 2; C.expect_rewalks = 2;
        run(C);
        C.name = "one near the best"; fill(C, 2, 800 * q);
        C.expect_winner = 1; C.expect_rewalks = 0;
        run(C);
    }
}

static void seeded(unsigned long long seed, int K) {
    Rng R{seed * 2654435761ull + 12345u};
    Case C;
    C.name = "seeded";
    const int* sh = kShapes[R.below((int)(sizeof(kShapes) / sizeof(kShapes[0])))];
    const int cz = sh[0] - 6;
    shape(C, sh[0], sh[1], sh[2], R.chance(50) ? sh[3] : 1 + R.below(cz), K, 2 + R.below(N - 1));
    C.slack = R.chance(50) ? 1.0 / 32.0 : 1.0 / 128.0;
    C.margin = R.chance(40) ? kPruneMarginF32 : 0.0;
    C.im1_min = 0.25;
    const int top = (int)((1.0 + C.slack) * 1024.0);          // values are multiples of 2^-10 in [-1, 1 + slack]
    const int kind = R.below(4);                              // spread-out levels / a tight group at the top / everything high / mixed
    for (int j = 0; j < C.n; ++j) {
        if (R.chance(10)) C.in[j] = false;
        int level = kind == 0 ? R.below(top + 200) - 200 : kind == 1 ? (R.chance(50) ? top - 120 + R.below(20) : R.below(top)) : kind == 2 ? top - R.below(40) : R.below(top);
        const int noise = R.chance(50) ? 0 : 1 + R.below(300);
        const bool background = R.chance(12), late_max = R.chance(10), nan = R.chance(3);
        if (background && R.chance(60)) level = top - R.below(8);
        const size_t items = C.v[0][j].size();
        for (size_t i = 0; i < items; ++i) {
            int x = level + (noise ? R.below(2 * noise + 1) - noise : 0);
            if (R.chance(2)) x = top;
            x = std::max(-1024, std::min(top, x));
            C.v[1][j][i] = x / 1024.0;
            // the float32 walk differs by up to 2^-12 per voxel (a quarter of the margin), never above 1 + slack
            C.v[0][j][i] = C.margin > 0.0 ? std::min((x * 4 + R.below(3) - 1) / 4096.0, (double)top / 1024.0) : C.v[1][j][i];
            C.mx[j][i] = background ? (R.chance(50) ? 0.25f : 0.f) : late_max ? (i + 1 == items || R.chance(3) ? 0.75f : 0.125f) : 0.3f + (float)R.below(8) / 8.f;
            C.hn[j][i] = R.chance(1);
        }
        if (nan) C.v[0][j][(size_t)R.below((int)items)] = C.v[1][j][(size_t)R.below((int)items)] = NAN;
    }
    run(C);
}

int main(int argc, char** argv) {
    const int ncases = argc > 1 ? atoi(argv[1]) : 3000;
    int total = 0;
    for (int K : {32, 16}) {
        const int before = g_fail;
        handmade(K);
        printf("K %d hand-made: %s\n", K, g_fail == before ? "ok" : "FAILED");
        for (int i = 0; i < ncases; ++i) seeded((unsigned long long)i * 2 + (K == 16), K);
        total += ncases;
    }
    printf("seeded cases %d failures %d\n", total, g_fail);
    return g_fail ? 1 : 0;
}
