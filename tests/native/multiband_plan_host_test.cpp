// Stand-alone host program of csrc/mvs_multiband_plan.h (tests/test_multiband_host.py builds it with -fsanitize=address,undefined and
// runs it directly).  It prints, for every axis start -13 .. 13, length 1 .. 40 and level count 1, 2 and 4 (pyramid top 4), the start
// and extent of every level ("A start n levels top s0 n0 s1 n1 ..."), which the test compares with the numpy restatement, and a few
// facts ("F name value") it checks itself.  The last line is "done".
#include <cstdio>
#include <cstdlib>

#include "mvs_multiband_plan.h"

namespace mp = mvs_multiband_plan;

static void require(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        std::exit(1);
    }
}

int main() {
    const int top = 4;
    const int counts[3] = {1, 2, 4};
    for (long long start = -13; start <= 13; ++start)
        for (long long n = 1; n <= 40; ++n)
            for (int levels : counts) {
                mp::Axis a;
                mp::plan_axis(start, n, levels, top, &a);
                std::printf("A %lld %lld %d %d", start, n, levels, top);
                for (int l = 0; l <= top; ++l) {
                    std::printf(" %lld %lld", a.start[l], a.n[l]);
                    if (l < top && a.decimated[l]) {
                        // every coarse sample's window meets the level below, and the samples next to the ends do not
                        const long long lo = a.start[l + 1], hi = lo + a.n[l + 1] - 1, s = a.start[l], e = s + a.n[l] - 1;
                        require(2 * lo + 2 >= s && 2 * lo - 2 <= e && 2 * hi - 2 <= e && 2 * hi + 2 >= s, "window meets the extent");
                        require(2 * (lo - 1) + 2 < s && 2 * (hi + 1) - 2 > e, "no coarse sample is missing");
                    }
                }
                std::printf("\n");
            }
    require(mp::floor_half(-3) == -2 && mp::floor_half(3) == 1 && mp::ceil_half(-3) == -1 && mp::ceil_half(3) == 2 && mp::floor_half(-4) == -2,
            "floor / ceil of halves");
    require(mp::radius(0) == 0 && mp::radius(3) == 28 && mp::radius(6) == 252, "radius");

    // the whole plan: refusals, sizes, the storage bounds of a large chunk
    mp::Plan p;
    int bad = 0;
    {
        const int32_t lv[3] = {0, 7, 1};
        const int64_t o[3] = {0, 0, 0}, s[3] = {1, 8, 8};
        bad += !mp::make_plan(lv, o, s, &p);
    }
    {
        const int32_t lv[3] = {0, -1, 1};
        const int64_t o[3] = {0, 0, 0}, s[3] = {1, 8, 8};
        bad += !mp::make_plan(lv, o, s, &p);
    }
    {
        const int32_t lv[3] = {0, 1, 1};
        const int64_t o[3] = {0, 0, 0}, s[3] = {1, 0, 8};
        bad += !mp::make_plan(lv, o, s, &p);
    }
    {
        const int32_t lv[3] = {0, 1, 1};
        const int64_t o[3] = {0, mp::kMaxIndex + 1, 0}, s[3] = {1, 8, 8};
        bad += !mp::make_plan(lv, o, s, &p);
    }
    {
        const int32_t lv[3] = {0, 1, 1};
        const int64_t o[3] = {0, 0, 0}, s[3] = {1, 8, mp::kMaxIndex};
        bad += !mp::make_plan(lv, o, s, &p);
    }
    std::printf("F bad_plans_refused %d\n", bad == 5);
    {
        const int32_t lv[3] = {0, 6, 6};
        const int64_t o[3] = {0, -5, 3}, s[3] = {1, 4096, 4096};
        require(mp::make_plan(lv, o, s, &p) && p.top == 6, "2D plan");
        std::printf("F storage_2d_ok %d\n", (double)(p.size[0] + mp::coarse_samples(p)) < 1.34 * (double)p.size[0]);
    }
    {
        const int32_t lv[3] = {6, 6, 6};
        // (every level holds 2 or 3 samples more than half the level below, so the bound needs axes of some length: 256^3 costs 1.157)
        const int64_t o[3] = {7, -5, 3}, s[3] = {512, 512, 512};
        require(mp::make_plan(lv, o, s, &p) && p.top == 6, "3D plan");
        std::printf("F storage_3d_ok %d\n", (double)(p.size[0] + mp::coarse_samples(p)) < 1.15 * (double)p.size[0]);
        for (int l = 0; l <= p.top; ++l) require(p.size[l] == p.axis[0].n[l] * p.axis[1].n[l] * p.axis[2].n[l], "level size");
    }
    {
        const int32_t lv[3] = {1, 2, 0};
        const int64_t o[3] = {0, 0, 0}, s[3] = {6, 40, 44};
        require(mp::make_plan(lv, o, s, &p) && p.top == 2, "mixed plan");
        require(p.axis[0].decimated[0] && !p.axis[0].decimated[1] && p.axis[1].decimated[1] && !p.axis[2].decimated[0], "decimated axes");
        require(p.axis[2].n[2] == 44 && p.axis[0].n[2] == p.axis[0].n[1], "undecimated axes keep their extent");
    }
    std::printf("F grid_capped %d\n", mp::grid_blocks(0, 256) == 1 && mp::grid_blocks(257, 256) == 2 && mp::grid_blocks(1LL << 40, 256) == mp::kMaxBlocks);
    require(mp::tiles_y(33) == 3 && mp::tiles_x(32) == 1 && mp::tiles_x(33) == 2, "tiles");
    std::printf("F max_levels %d\nF max_views %d\nF tile_y %d\nF tile_x %d\nF lds_bytes %d\n", mp::kMaxLevels, mp::kMaxViews, mp::kTileY, mp::kTileX,
                mp::kLdsBytes);
    std::printf("done\n");
    return 0;
}
