// Translation-path view records made by hand and the geometries they are made for, shared by the host tests under tests/native/:
// region_plan_host_test.cpp plans with such views, fuse_chunk_plan_host_test.cpp compares them with what prepare_translation_view +
// fill_tr_view (csrc/mvs_fuse_chunk_plan.h) derive from the same geometry, field by field and bit for bit.  The way
// weights.blending_supports lays a view out for unit spacings: a view of n pixels whose first pixel lies at chunk coordinate p has the
// valid box [ceil(p), floor(p + n - 1)], support nodes 0 and 4 at p - 1 and p + n, (n + 1) / 4 pixels per node and the tent scale
// (n + 1) / 4 / blending width, no larger than twice the scale of another axis (the form in which the support table holds it).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mvs_fuse_tr.h"

namespace {

const double kBlend[3] = {3.0, 10.0, 10.0};   // default blending widths z, y, x

// One view: n pixels per axis, first pixel at chunk coordinate p (2-D: n[0] = 1, p[0] = 0), chunk of `cs` voxels.
TrView make_view(int ndim, const double p[3], const int n[3], const int cs[3]) {
    TrView V;
    memset(&V, 0, sizeof(V));
    V.wnz = ndim == 3 ? 5 : 1;
    V.linear = 1;
    for (int k = 0; k < 3; ++k) {
        const double off = -p[k];                       // slab pixel = chunk index + off
        const double f = floor(off);
        V.io[k] = (int)f;
        V.fw[k] = (float)(off - f);
        long long lo = (long long)ceil(-off), hi = (long long)floor((double)(n[k] - 1) - off);
        if (lo < 0) lo = 0;
        if (hi > cs[k] - 1) hi = cs[k] - 1;
        V.lo[k] = (int)lo;
        V.hi[k] = (int)std::max<long long>(hi, -1);
        V.n[k] = n[k];
        if (k == 0 && ndim == 2) continue;              // no support along z: sup_* and ws stay 0
        const double S = (double)(n[k] + 1) / 4.0;      // support spacing: (shape - 1) / 4 * (shape + 1) / (shape - 1)
        const double wm = 1.0 / S, wo = -(p[k] - 1.0) / S;
        const double slo = -wo / wm, shi = (4.0 - wo) / wm;
        V.sup_k[k] = (float)wm;
        V.sup_ilo[k] = (int)floor(slo);
        V.sup_flo[k] = (float)(slo - floor(slo));
        V.sup_ihi[k] = (int)ceil(shi);
        V.sup_fhi[k] = (float)(ceil(shi) - shi);
        V.ws[k] = (float)(S / kBlend[k]);
    }
    // the scales as prepare_translation_view reads them off the support table min_d(ws_d * tent(i_d)): the entry next to the centre
    // along k holds min(ws_k, 2 ws_j of the other axes) -- the same table, whichever of the two sets of scales spans it
    const float spacing_scale[3] = {V.ws[0], V.ws[1], V.ws[2]};
    for (int k = 3 - ndim; k < 3; ++k)
        for (int j = 3 - ndim; j < 3; ++j)
            if (j != k) V.ws[k] = fminf(V.ws[k], 2.f * spacing_scale[j]);
    V.stride_y = n[2];
    V.stride_z = n[2] * n[1];
    V.span = (long long)n[0] * n[1] * n[2];
    return V;
}

unsigned long long rng_state = 88172645463325252ull;
unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }
int rnd_int(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }   // inclusive

struct Geometry {
    std::string name;
    int ndim = 2;
    std::vector<std::array<double, 3>> origin;   // first pixel of every view, chunk coordinates before the shift to >= 0
    std::vector<std::array<int, 3>> shape;
    int trim = 0;
};

// views of a geometry in the chunk that is their union (origins shifted so that the union starts at 0)
void build(const Geometry& g, std::vector<TrView>* views, int cs[3]) {
    double mn[3] = {1e30, 1e30, 1e30}, mx[3] = {-1e30, -1e30, -1e30};
    for (size_t i = 0; i < g.origin.size(); ++i)
        for (int k = 0; k < 3; ++k) {
            mn[k] = std::min(mn[k], g.origin[i][k]);
            mx[k] = std::max(mx[k], g.origin[i][k] + g.shape[i][k] - 1);
        }
    for (int k = 0; k < 3; ++k) cs[k] = (int)floor(mx[k] - mn[k] + 1e-9) + 1;
    views->clear();
    for (size_t i = 0; i < g.origin.size(); ++i) {
        double p[3];
        for (int k = 0; k < 3; ++k) p[k] = g.origin[i][k] - mn[k];
        views->push_back(make_view(g.ndim, p, g.shape[i].data(), cs));
    }
}

Geometry grid(const char* name, int ndim, const int tiles[3], const int shape[3], const int overlap[3], int jitter, bool frac, int trim = 0) {
    Geometry g;
    g.name = name;
    g.ndim = ndim;
    g.trim = trim;
    for (int iz = 0; iz < tiles[0]; ++iz)
        for (int iy = 0; iy < tiles[1]; ++iy)
            for (int ix = 0; ix < tiles[2]; ++ix) {
                const int idx[3] = {iz, iy, ix};
                std::array<double, 3> p;
                std::array<int, 3> n;
                for (int k = 0; k < 3; ++k) {
                    n[k] = shape[k];
                    p[k] = (double)idx[k] * (shape[k] - overlap[k]);
                    if (k == 0 && ndim == 2) continue;
                    if (jitter) p[k] += rnd_int(-jitter, jitter);
                    if (frac) p[k] += (double)rnd_int(1, 15) / 16.0;
                }
                g.origin.push_back(p);
                g.shape.push_back(n);
            }
    return g;
}

Geometry stair(const char* name, int ndim, int nviews, const int shape[3], const double step[3], double frac = 0.0) {
    Geometry g;
    g.name = name;
    g.ndim = ndim;
    for (int i = 0; i < nviews; ++i) {
        std::array<double, 3> p;
        std::array<int, 3> n;
        for (int k = 0; k < 3; ++k) {
            n[k] = shape[k];
            p[k] = (k == 0 && ndim == 2) ? 0.0 : i * step[k] + ((i & 1) ? frac : 0.0);
        }
        g.origin.push_back(p);
        g.shape.push_back(n);
    }
    return g;
}

Geometry placed(const char* name, int ndim, std::vector<std::array<double, 3>> origin, std::vector<std::array<int, 3>> shape) {
    Geometry g;
    g.name = name;
    g.ndim = ndim;
    g.origin = origin;
    g.shape = shape;
    return g;
}

// every geometry the region plan is checked on, in one fixed order (the random ones draw from rnd): run(g) for each
template <typename F>
void geometries(F run) {
    char name[96];
    // registered grids: whole-pixel and fractional jitter, 2-D and 3-D, one trimmed
    {
        const int t2[3] = {1, 2, 3}, s2[3] = {1, 72, 200}, o2[3] = {0, 20, 50};
        run(grid("grid_2d_exact", 2, t2, s2, o2, 0, false));
        run(grid("grid_2d_registered", 2, t2, s2, o2, 3, false));
        run(grid("grid_2d_registered_frac", 2, t2, s2, o2, 3, true));
        run(grid("grid_2d_registered_trimmed", 2, t2, s2, o2, 3, false, 5));
        const int t3[3] = {2, 2, 2}, s3[3] = {24, 40, 72}, o3[3] = {8, 12, 20};
        run(grid("grid_3d_registered", 3, t3, s3, o3, 3, false));
        run(grid("grid_3d_registered_frac", 3, t3, s3, o3, 2, true));
    }
    // clustering limit: y origins 0, 16, 17 in a row along x; z origins 0, 2, 5 (everything clusters along z)
    run(placed("row_y_0_16_17", 2, {{0, 0, 0}, {0, 16, 90}, {0, 17, 180}}, {{1, 48, 120}, {1, 48, 120}, {1, 48, 120}}));
    run(placed("row_z_0_2_5", 3, {{0, 0, 0}, {2, 0, 52}, {5, 0, 104}}, {{12, 40, 72}, {12, 40, 72}, {12, 40, 72}}));
    // stairs: 1..8 views on a cell, without and with clustered borders, whole-pixel and fractional
    {
        const int big[3] = {1, 136, 168}, small[3] = {1, 64, 96};
        const double sb[3] = {0, 18, 20}, ss[3] = {0, 6, 9};
        for (int nv = 7; nv <= 8; ++nv)
            for (int f = 0; f < 2; ++f) {
                snprintf(name, sizeof(name), "stair_2d_%d_wide%s", nv, f ? "_frac" : "");
                run(stair(name, 2, nv, big, sb, f ? 0.375 : 0.0));
                snprintf(name, sizeof(name), "stair_2d_%d_clustered%s", nv, f ? "_frac" : "");
                run(stair(name, 2, nv, small, ss, f ? 0.375 : 0.0));
            }
        const int s3[3] = {28, 36, 44};
        const double st3[3] = {5, 6, 7};
        run(stair("stair_3d_5", 3, 5, s3, st3));
        run(stair("stair_3d_5_frac", 3, 5, s3, st3, 0.625));
    }
    // brick widths: two tiles that share W columns (overlap boxes at the limits 32 | 33 and 136 | 137), single views whose interior
    // box is 160 | 161 wide, a z-stacked pair
    for (int W : {9, 32, 33, 136, 137, 300})
        for (int f = 0; f < 2; ++f) {
            snprintf(name, sizeof(name), "pair_W%d%s", W, f ? "_frac" : "");
            const int rows = W == 300 ? 80 : 37;
            run(placed(name, 2, {{0, 0, 0}, {0, f ? 0.25 : 0.0, 140.0 + (f ? 0.5 : 0.0)}}, {{1, rows, W + 140}, {1, rows, W + 140}}));
        }
    run(placed("pair_3d_W33", 3, {{0, 0, 0}, {0, 0, 140}}, {{6, 37, 173}, {6, 37, 173}}));
    run(placed("pair_3d_W137", 3, {{0, 0, 0}, {0, 0, 140}}, {{6, 37, 277}, {6, 37, 277}}));
    run(placed("pair_z_stacked", 3, {{0, 0, 0}, {8, 0, 0}}, {{24, 40, 72}, {24, 40, 72}}));
    for (int nx : {40, 41, 168, 169, 529}) {
        snprintf(name, sizeof(name), "single_%d", nx);
        run(placed(name, 2, {{0, 0, 0}}, {{1, 37, nx}}));
    }
    run(placed("sole_contributor_pair", 2, {{0, 0, 0}, {0, 0, 60}}, {{1, 40, 72}, {1, 40, 72}}));
    // random stairs and grids
    for (int i = 0; i < 12; ++i) {
        const int ndim = 2 + (i & 1);
        const int nv = rnd_int(2, 8);
        const int shape[3] = {ndim == 3 ? rnd_int(8, 20) : 1, rnd_int(30, 70), rnd_int(40, 180)};
        const double step[3] = {ndim == 3 ? (double)rnd_int(1, 6) : 0.0, (double)rnd_int(2, 24), (double)rnd_int(3, 40)};
        snprintf(name, sizeof(name), "random_stair_%d", i);
        run(stair(name, ndim, nv, shape, step, (i & 2) ? (double)rnd_int(1, 7) / 8.0 : 0.0));
    }
    for (int i = 0; i < 8; ++i) {
        const int ndim = 2 + (i & 1);
        const int tiles[3] = {ndim == 3 ? 2 : 1, rnd_int(1, 3), rnd_int(2, 3)};
        const int shape[3] = {ndim == 3 ? rnd_int(8, 16) : 1, rnd_int(30, 60), rnd_int(50, 190)};
        const int overlap[3] = {ndim == 3 ? rnd_int(2, 6) : 0, rnd_int(4, 24), rnd_int(8, 40)};
        snprintf(name, sizeof(name), "random_grid_%d", i);
        run(grid(name, ndim, tiles, shape, overlap, rnd_int(0, 5), (i & 2) != 0, (i & 4) ? 3 : 0));
    }
}

}  // namespace
