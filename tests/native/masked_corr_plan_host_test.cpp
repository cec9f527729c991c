// Stand-alone host program of csrc/mvs_masked_corr_plan.h (tests/test_masked_corr_host.py builds it with the host compiler under
// the address and undefined-behaviour sanitizers and reads its output):
//   P <nz> <ny> <nx> <Sz> <Sy> <Sx> : code, S, P, W, voxels, padded, window, blocks of the three grids
//   A <n> <S>                       : the alias-free property of padded_length(n, S) on a 1-D example, and that half that length breaks it
//   W <n...>                        : window_to_padded of every window entry of a small plan against a direct computation
//   E <nz> <ny> <nx>                : window, window_to_padded of the first and of the last window entry (the large test cases)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mvs_masked_corr_plan.h"

using namespace mvs_masked_corr_plan;

static void print_plan(int ndim, long long nz, long long ny, long long nx, long long sz, long long sy, long long sx) {
    const int64_t shape[3] = {nz, ny, nx}, ms[3] = {sz, sy, sx};
    Plan p;
    const PlanCode code = make_plan(ndim, shape, ms, &p);
    std::printf("P %d %lld %lld %lld %lld %lld %lld : %d", ndim, nz, ny, nx, sz, sy, sx, (int)code);
    if (code == kPlanOk)
        std::printf(" %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %d %d %d", (long long)p.S[0], (long long)p.S[1], (long long)p.S[2],
                    (long long)p.P[0], (long long)p.P[1], (long long)p.P[2], (long long)p.W[0], (long long)p.W[1], (long long)p.W[2], p.voxels, p.padded,
                    p.window, p.voxel_blocks, p.padded_blocks, p.window_blocks);
    std::printf("\n");
}

// window_to_padded at the first and the last entry of the window of a plan
static void print_ends(int ndim, long long nz, long long ny, long long nx, long long sz, long long sy, long long sx) {
    const int64_t shape[3] = {nz, ny, nx}, ms[3] = {sz, sy, sx};
    Plan p;
    if (make_plan(ndim, shape, ms, &p) != kPlanOk) std::exit(1);
    std::printf("E %lld %lld %lld : %lld %lld %lld\n", nz, ny, nx, p.window, window_to_padded(p, 0), window_to_padded(p, p.window - 1));
}

// integer sequences a, b of n samples: mismatches between the circular correlation at length P and the linear one over |s| <= S
static int alias_mismatches(int n, int S, long long P) {
    std::vector<long long> a((size_t)P, 0), b((size_t)P, 0);
    for (int x = 0; x < n; ++x) {
        a[(size_t)x] = 1 + (x * 7) % 5;
        b[(size_t)x] = 2 + (x * 3) % 7;
    }
    int bad = 0;
    for (int s = -S; s <= S; ++s) {
        long long lin = 0, circ = 0;
        for (int x = 0; x < n; ++x)
            if (x + s >= 0 && x + s < n) lin += a[(size_t)x] * b[(size_t)(x + s)];
        for (long long x = 0; x < P; ++x) circ += a[(size_t)x] * b[(size_t)(((x + s) % P + P) % P)];
        if (lin != circ) ++bad;
    }
    return bad;
}

int main() {
    print_plan(2, 1, 13, 20, -1, -1, -1);
    print_plan(3, 6, 9, 11, -1, -1, -1);
    print_plan(2, 1, 24, 40, -1, 5, 7);
    print_plan(2, 1, 1, 17, -1, -1, -1);
    print_plan(3, 8, 16, 16, -1, -1, -1);
    print_plan(2, 1, 5, 31, -1, 4, 9);
    print_plan(3, 8, 16, 16, 0, 0, 0);               // no shift at all: P = n
    print_plan(3, 8, 16, 16, 1, 1, 100);             // above n - 1: n - 1
    print_plan(3, 2, 2, 2, -1, -1, -1);
    print_plan(3, 400, 400, 400, -1, -1, -1);        // 1024^3: over the limit
    print_plan(3, 400, 400, 400, 100, 100, 100);     // 512^3 = 2^27
    print_plan(3, 512, 512, 512, 0, 0, 0);           // 2^27
    print_plan(3, 512, 512, 1024, 0, 0, 0);          // exactly the limit
    print_plan(3, 512, 512, 1024, 0, 0, 1);          // one step over
    print_plan(2, 1, 16384, 16384, 0, 0, 0);         // 2^28
    print_plan(2, 1, 16385, 16384, 0, 0, 0);
    print_plan(3, 2147483647LL, 2147483647LL, 2147483647LL, -1, -1, -1);      // no overflow on the way to the refusal
    print_plan(2, 2, 16, 16, -1, -1, -1);            // 2D with a z extent
    print_plan(4, 1, 16, 16, -1, -1, -1);
    print_plan(3, 0, 16, 16, -1, -1, -1);
    print_plan(3, 4294967296LL, 1, 1, -1, -1, -1);
    // the large test cases: more than kMaxBlocks * kThreads = 262144 items in a grid (a second trip of the grid-stride loops)
    print_plan(2, 1, 520, 520, -1, 300, 300);
    print_plan(3, 20, 130, 130, 3, 40, 40);
    print_plan(2, 1, 3, 4100, -1, 1, 10);
    print_ends(2, 1, 520, 520, -1, 300, 300);
    print_ends(3, 20, 130, 130, 3, 40, 40);
    print_ends(2, 1, 3, 4100, -1, 1, 10);

    const int ex[][2] = {{17, 16}, {17, 4}, {13, 12}, {20, 19}, {16, 15}, {16, 0}, {5, 4}, {2, 1}, {31, 9}, {40, 7}};
    for (const auto& e : ex) {
        const long long P = padded_length(e[0], e[1]);
        // (half the length aliases whenever it is shorter than n + S and a shift is searched at all)
        const long long half = P / 2 >= e[0] ? P / 2 : P;
        std::printf("A %d %d : %lld %d %lld %d\n", e[0], e[1], P, alias_mismatches(e[0], e[1], P), half, alias_mismatches(e[0], e[1], half));
    }

    {
        const int64_t shape[3] = {3, 5, 6}, ms[3] = {1, -1, 2};
        Plan p;
        if (make_plan(3, shape, ms, &p) != kPlanOk) return 1;
        int bad = 0;
        long long w = 0;
        for (long long sz = -p.S[0]; sz <= p.S[0]; ++sz)
            for (long long sy = -p.S[1]; sy <= p.S[1]; ++sy)
                for (long long sx = -p.S[2]; sx <= p.S[2]; ++sx, ++w) {
                    const long long want = (((sz + p.P[0]) % p.P[0]) * p.P[1] + (sy + p.P[1]) % p.P[1]) * p.P[2] + (sx + p.P[2]) % p.P[2];
                    const long long got = window_to_padded(p, w);
                    if (got != want || got < 0 || got >= p.padded) ++bad;
                }
        std::printf("W %lld %lld %d\n", w, p.window, bad);
    }
    std::printf("G %d %d %d %d %d\n", grid_blocks(0), grid_blocks(1), grid_blocks(256), grid_blocks(257), grid_blocks(1LL << 28));
    std::printf("done\n");
    return 0;
}
