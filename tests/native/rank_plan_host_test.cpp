// Host-side run of csrc/mvs_rank_plan.h (plain integer functions, __host__ __device__): the launch hist_ranks_apply sizes for the
// counting pass of the histogram ranks against the ranges hist_rank_kernel takes from it.  tests/test_rank_plan_host.py builds this
// with hipcc (no GPU needed).  For every n of the list (gb = score_grid(n)):
//   counters   an accepted plan gives a workgroup at most 65535 voxels (4 * per <= 65535: a 16-bit counter holds them all)
//   grid       hgb >= 1
//   cover      hgb * per >= ngroups
//   fold       fold implies hgb <= kHistParts
//   tiling     the ranges of the hgb workgroups of the counting pass, and of the gb workgroups of the correlation pass, are
//              [0, ngroups) without gap or overlap
// Lines:
//   C <n checked> <n accepted>
//   W <what> <n wrong> <first wrong n> <hgb there> <per there>        one per property
#include <cstdio>

#include "mvs_rank_plan.h"

namespace {
using namespace mvs_rank_plan;

struct Wrong { long long wrong = 0, n = 0, hgb = 0, per = 0; };
Wrong w_counters, w_grid, w_cover, w_fold, w_tiling;
long long checked = 0, accepted = 0;

void note(Wrong& w, long long n, long long hgb, long long per) {
    if (!w.wrong) { w.n = n; w.hgb = hgb; w.per = per; }
    ++w.wrong;
}

bool tiles(unsigned int n, unsigned int grid) {
    const unsigned int ngroups = hist_groups(n);
    unsigned int at = 0;
    for (unsigned int b = 0; b < grid; ++b) {
        unsigned int g0, g1;
        hist_range(n, grid, b, &g0, &g1);
        if (g0 != at || g1 < g0 || g1 > ngroups) return false;
        at = g1;
    }
    return at == ngroups;
}

void check(long long n) {
    if (n < 1 || n >= (1ll << 31) - 8) return;
    ++checked;
    const int gb = score_grid(n);
    const HistLaunch h = hist_launch(n, gb);
    const long long ngroups = hist_groups((unsigned int)n);
    const long long per = h.hgb >= 1 ? (long long)hist_per((unsigned int)ngroups, (unsigned int)h.hgb) : 0;
    if (h.hgb < 1) { note(w_grid, n, h.hgb, per); return; }
    if (h.hgb * per < ngroups) note(w_cover, n, h.hgb, per);
    if (h.fold && h.hgb > kHistParts) note(w_fold, n, h.hgb, per);
    if (!tiles((unsigned int)n, (unsigned int)gb)) note(w_tiling, n, gb, hist_per((unsigned int)ngroups, (unsigned int)gb));
    if (!h.ok) return;
    ++accepted;
    if (4 * per > 65535) note(w_counters, n, h.hgb, per);
    if (!tiles((unsigned int)n, (unsigned int)h.hgb)) note(w_tiling, n, h.hgb, per);
}

void report(const char* what, const Wrong& w) { printf("W %s %lld %lld %lld %lld\n", what, w.wrong, w.n, w.hgb, w.per); }
}  // namespace

int main() {
    for (long long n = 1; n <= 70000; ++n) check(n);
    auto around = [](long long k) {
        for (long long r = -4; r <= 4; ++r) check(4 * 16383 * k + r);
    };
    for (long long k = 1; k <= 300; ++k) around(k);
    for (long long k = 2046; k <= 2050; ++k) around(k);
    around(5000);
    around(30000);
    check((1ll << 31) - 9);
    printf("C %lld %lld\n", checked, accepted);
    report("counters", w_counters);
    report("grid", w_grid);
    report("cover", w_cover);
    report("fold", w_fold);
    report("tiling", w_tiling);
    printf("done\n");
    return 0;
}
