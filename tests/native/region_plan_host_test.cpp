// Host-side run of csrc/mvs_region_plan.h (the plan of the region fuse kernels: regions, flags, classes, brick lists; no HIP call).
// tests/test_region_plan_host.py builds this with hipcc (no GPU needed) and reads
//   C <group> <n checked>                         one per group of properties
//   W <property> <n wrong> <first wrong case>     one per property
// Every property is checked by brute force over the voxels of small chunks: the flags of a region are promises about EVERY voxel of
// its box (the planner itself looks at the 8 corners only and relies on the concavity of the weight profile), and a wrong flag
// gives wrong voxels in a few cells only.  The views are made by hand the way prepare_translation_view (mvs_fuse.hip) and
// weights.blending_supports derive them for unit spacings: a view of n pixels whose first pixel lies at chunk coordinate p has the
// valid box [ceil(p), floor(p + n - 1)], support nodes 0 and 4 at p - 1 and p + n, (n + 1) / 4 pixels per node and the tent scale
// (n + 1) / 4 / blending width.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "mvs_region_plan.h"

namespace {

std::map<std::string, long long> n_checked;
struct Wrong { long long wrong = 0; std::string first; };
std::map<std::string, Wrong> wrongs;
const char* group = "";
char where[256] = "";

void check(const char* prop, bool ok) {
    ++n_checked[group];
    Wrong& w = wrongs[prop];
    if (ok) return;
    if (!w.wrong) w.first = where;
    ++w.wrong;
}

unsigned long long rng_state = 88172645463325252ull;
unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }
int rnd_int(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }   // inclusive

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
    V.stride_y = n[2];
    V.stride_z = n[2] * n[1];
    V.span = (long long)n[0] * n[1] * n[2];
    return V;
}

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

inline bool in_box(const TrView& V, int z, int y, int x) {
    return z >= V.lo[0] && z <= V.hi[0] && y >= V.lo[1] && y <= V.hi[1] && x >= V.lo[2] && x <= V.hi[2];
}

// every property of one plan, by brute force over the voxels of the trimmed chunk
void check_plan(const Geometry& g, bool mixed) {
    std::vector<TrView> views;
    int cs[3];
    build(g, &views, cs);
    const int nviews = (int)views.size();
    int t[3], o[3];
    for (int k = 0; k < 3; ++k) { t[k] = (k == 0 && g.ndim == 2) ? 0 : g.trim; o[k] = cs[k] - 2 * t[k]; }
    RegionPlan plan;
    mvs_region_plan(views.data(), nviews, t, o, mixed, &plan);
    snprintf(where, sizeof(where), "%s mixed %d", g.name.c_str(), (int)mixed);
    group = "plans";
    check("small_chunk_is_accepted", !plan.declined);
    if (plan.declined) return;
    check("regions_below_the_padding_id", plan.regions.size() < 65535);

    // ---- regions: tiling, view lists, flags ----
    group = "voxels";
    std::vector<int> owner((size_t)o[0] * o[1] * o[2], 0);
    for (size_t rid = 0; rid < plan.regions.size(); ++rid) {
        const Region& R = plan.regions[rid];
        const int nv = R.nviews & 0xff, lxb = (R.nviews >> 8) & 7, cls = (R.nviews >> 12) & 7;
        snprintf(where, sizeof(where), "%s mixed %d region %zu [%d,%d)x[%d,%d)x[%d,%d) nv %d masks %#x", g.name.c_str(), (int)mixed, rid, R.z0, R.z1,
                 R.y0, R.y1, R.x0, R.x1, nv, (unsigned)R.allone_mask);
        const bool inside = R.z0 >= t[0] && R.z1 <= t[0] + o[0] && R.y0 >= t[1] && R.y1 <= t[1] + o[1] && R.x0 >= t[2] && R.x1 <= t[2] + o[2] &&
                            R.z0 < R.z1 && R.y0 < R.y1 && R.x0 < R.x1;
        check("region_is_a_box_of_the_trimmed_chunk", inside);
        if (!inside) continue;
        std::vector<char> met(nviews, 0);
        bool full[kMaxRV], unit_everywhere[kMaxRV], positive_everywhere[kMaxRV];
        for (int v = 0; v < kMaxRV; ++v) full[v] = unit_everywhere[v] = positive_everywhere[v] = true;
        for (int z = R.z0; z < R.z1; ++z)
            for (int y = R.y0; y < R.y1; ++y)
                for (int x = R.x0; x < R.x1; ++x) {
                    ++owner[((size_t)(z - t[0]) * o[1] + (y - t[1])) * o[2] + (x - t[2])];
                    for (int v = 0; v < nviews; ++v)
                        if (in_box(views[v], z, y, x)) met[v] = 1;
                    for (int v = 0; v < nv; ++v) {
                        const TrView& V = views[R.ids[v]];
                        if (!in_box(V, z, y, x)) full[v] = false;
                        const float W = tr_weight_profile(V, z, y, x);
                        if (!(W >= 1.f)) unit_everywhere[v] = false;
                        if (!(W >= 3e-4f)) positive_everywhere[v] = false;
                    }
                }
        std::set<int> listed(R.ids, R.ids + nv), meets;
        for (int v = 0; v < nviews; ++v)
            if (met[v]) meets.insert(v);
        check("region_lists_the_views_that_meet_it", (int)listed.size() == nv && listed == meets);
        bool all_full_positive = nv > 0;
        for (int v = 0; v < nv; ++v) {
            const bool partial = (R.allone_mask >> (16 + v)) & 1, unit = (R.allone_mask >> v) & 1;
            check("view_not_flagged_partial_contains_the_box", partial || full[v]);
            check("partial_flag_only_on_a_view_that_misses_voxels", !partial || !full[v]);
            check("unit_bit_means_weight_1_at_every_voxel", !unit || (full[v] && unit_everywhere[v]));
            all_full_positive = all_full_positive && full[v] && positive_everywhere[v];
        }
        check("bit_15_means_every_view_full_and_positive", !((R.allone_mask >> 15) & 1) || all_full_positive);
        const bool copy = nv == 1 && full[0] && positive_everywhere[0];
        check("copy_class_means_one_full_positive_view", cls != 4 || copy);
        check("class_follows_the_view_count", cls == (copy ? 4 : nv <= 1 ? 0 : nv == 2 ? 1 : nv <= 4 ? 2 : 3));
        const int w = R.x1 - R.x0;
        const int want_lxb = w <= 32 ? 1 : (copy && w > 160) ? 6 : (nv >= 2 && w <= 136) ? 3 : 4;
        check("brick_width_follows_the_box_width", lxb == want_lxb);
        const int limits[6] = {32, 33, 136, 137, 160, 161};
        for (int k = 0; k < 6; ++k) {
            // the limits count only where they decide: 32 | 33 everywhere, 136 | 137 for overlaps, 160 | 161 for the copy class
            const bool decides = k < 2 || (k < 4 ? nv >= 2 : copy);
            if (w == limits[k] && decides) {
                char gname[32];
                snprintf(gname, sizeof(gname), "width_%d", w);
                ++n_checked[gname];
            }
        }
    }
    snprintf(where, sizeof(where), "%s mixed %d", g.name.c_str(), (int)mixed);
    bool once = true;
    for (int c : owner) once = once && c == 1;
    check("regions_tile_the_trimmed_chunk_once", once);

    // ---- brick lists ----
    group = "bricks";
    std::map<std::tuple<int, int, int, int>, int> seen;
    bool in_range = true, padding_ok = true, mixed_classes_ok = true;
    const int nitems = (int)plan.items.size();
    for (int i = 0; i < nitems; ++i) {
        const Item it = plan.items[i];
        const int rid = it.region_bx & 0xffff, bx = (unsigned)it.region_bx >> 16, by = it.by_bz & 0xffff, bz = (unsigned)it.by_bz >> 16;
        if (rid == 0xffff) {
            padding_ok = padding_ok && i < plan.mixed_count && it.region_bx == 0xffff && it.by_bz == 0;
            continue;
        }
        if (rid >= (int)plan.regions.size()) { in_range = false; continue; }
        const Region& R = plan.regions[rid];
        const int bxw = kRV << ((R.nviews >> 8) & 7), cls = (R.nviews >> 12) & 7;
        in_range = in_range && R.x0 + bx * bxw < R.x1 && R.y0 + by * 32 < R.y1 && R.z0 + bz * kRB < R.z1;
        if (i < plan.mixed_count) mixed_classes_ok = mixed_classes_ok && (cls == 4 || cls == 0 || cls == 1);
        ++seen[std::make_tuple(rid, bx, by, bz)];
    }
    check("brick_lies_in_its_region", in_range);
    long long want_bricks = 0;
    bool each_once = true;
    for (size_t rid = 0; rid < plan.regions.size(); ++rid) {
        const Region& R = plan.regions[rid];
        const int bxw = kRV << ((R.nviews >> 8) & 7);
        const int nbz = (R.z1 - R.z0 + kRB - 1) / kRB, nby = (R.y1 - R.y0 + 31) / 32, nbx = (R.x1 - R.x0 + bxw - 1) / bxw;
        for (int bz = 0; bz < nbz; ++bz)
            for (int by = 0; by < nby; ++by)
                for (int bx = 0; bx < nbx; ++bx) {
                    auto f = seen.find(std::make_tuple((int)rid, bx, by, bz));
                    each_once = each_once && f != seen.end() && f->second == 1;
                    ++want_bricks;
                }
    }
    check("every_brick_of_every_region_occurs_once", each_once && (long long)seen.size() == want_bricks);
    check("brick_counter_excludes_the_padding", plan.bricks == want_bricks);
    // class lists: contiguous after the mixed list, in class order, as long as class_count says
    {
        int at = plan.mixed_count;
        bool ok = at <= nitems;
        for (int k = 0; k < 5 && ok; ++k) {
            ok = plan.class_count[k] >= 0 && at + plan.class_count[k] <= nitems;
            for (int i = 0; ok && i < plan.class_count[k]; ++i) {
                const int rid = plan.items[at + i].region_bx & 0xffff;
                ok = rid < (int)plan.regions.size() && ((plan.regions[rid].nviews >> 12) & 7) == k;
            }
            at += plan.class_count[k];
        }
        check("class_items_contiguous_and_counted", ok && at == nitems);
    }
    {   // class voxel counters = the voxels of the class's boxes
        double out_vox[5] = {0, 0, 0, 0, 0}, in_vox[5] = {0, 0, 0, 0, 0};
        for (const Region& R : plan.regions) {
            const double vox = (double)(R.z1 - R.z0) * (R.y1 - R.y0) * (R.x1 - R.x0);
            out_vox[(R.nviews >> 12) & 7] += vox;
            in_vox[(R.nviews >> 12) & 7] += vox * (R.nviews & 0xff);
        }
        bool ok = true;
        for (int k = 0; k < 5; ++k) ok = ok && out_vox[k] == plan.class_out_vox[k] && in_vox[k] == plan.class_in_vox[k];
        check("class_voxel_counters_are_the_boxes", ok);
    }
    if (!mixed) {
        check("no_mixed_list_without_the_option", plan.mixed_count == 0 && padding_ok);
        return;
    }
    group = "mixed";
    check("mixed_padding_items_are_0xffff_inside_the_mixed_list", padding_ok);
    check("mixed_list_holds_classes_4_0_1_only", mixed_classes_ok);
    check("mixed_classes_not_again_in_the_class_lists", plan.class_count[4] == 0 && plan.class_count[0] == 0 && plan.class_count[1] == 0);
    const int L = plan.mixed_count / 8;
    check("mixed_eight_stretches_of_one_length_multiple_of_4", plan.mixed_count % 8 == 0 && L % 4 == 0);
    bool trailing = true;      // a stretch is bricks first, padding after
    for (int k = 0; k < 8 && plan.mixed_count % 8 == 0; ++k) {
        bool pad = false;
        for (int i = 0; i < L; ++i) {
            const bool is_pad = (plan.items[k * L + i].region_bx & 0xffff) == 0xffff;
            trailing = trailing && (is_pad || !pad);
            pad = pad || is_pad;
        }
    }
    check("mixed_padding_ends_a_stretch", trailing);
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

void run(const Geometry& g) {
    check_plan(g, false);
    check_plan(g, true);
}

void geometries() {
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

// ---- break points ----
bool has(const std::vector<int>& v, int x) { return std::find(v.begin(), v.end(), x) != v.end(); }

void breakpoints() {
    group = "breakpoints";
    // two views whose borders along axis d lie `gap` apart, well inside the chunk
    for (int ndim = 2; ndim <= 3; ++ndim)
        for (int d = 3 - ndim; d < 3; ++d)
            for (int gap : {1, 15, 16, 17, 40}) {
                const int cs[3] = {ndim == 3 ? 400 : 1, 400, 400};
                double p0[3] = {0, 0, 0}, p1[3] = {0, 0, 0};
                int n0[3] = {ndim == 3 ? 200 : 1, 200, 200}, n1[3] = {n0[0], n0[1], n0[2]};
                for (int k = 3 - ndim; k < 3; ++k) p0[k] = p1[k] = 50;
                p1[d] = 50 + gap;                 // lower borders at 50 and 50 + gap, upper borders + 1 at 250 and 250 + gap
                const TrView views[2] = {make_view(ndim, p0, n0, cs), make_view(ndim, p1, n1, cs)};
                std::vector<int> pts;
                axis_breakpoints(views, 2, d, 0, cs[d], &pts);
                snprintf(where, sizeof(where), "ndim %d axis %d gap %d", ndim, d, gap);
                if (gap <= 16) {
                    check("borders_16_apart_share_a_break_point", has(pts, 50) && !has(pts, 50 + gap) && has(pts, 250 + gap) && !has(pts, 250));
                } else {
                    check("borders_17_apart_do_not", has(pts, 50) && has(pts, 50 + gap) && has(pts, 250) && has(pts, 250 + gap));
                }
                check("break_points_sorted_unique_within_the_chunk",
                      pts.front() == 0 && pts.back() == cs[d] && std::adjacent_find(pts.begin(), pts.end(), [](int a, int b) { return a >= b; }) == pts.end());
            }
    // the 4-voxel shell along x is cut on the rim of the mosaic only: a lone view has it at both ends, the inner borders of a
    // two-tile row (each covered by the neighbour) have none
    for (int nx : {40, 168, 529}) {
        const int cs[3] = {1, 37, nx}, n[3] = {1, 37, nx};
        const double p[3] = {0, 0, 0};
        const TrView V = make_view(2, p, n, cs);
        std::vector<int> pts;
        axis_breakpoints(&V, 1, 2, 0, nx, &pts);
        snprintf(where, sizeof(where), "lone view of %d columns", nx);
        check("x_shell_is_cut_on_the_rim_only", pts == std::vector<int>({0, 4, nx - 4, nx}));
    }
    for (int W : {33, 136, 300}) {
        const int nx = W + 140, cs[3] = {1, 37, nx + 140}, n[3] = {1, 37, nx};
        const double p0[3] = {0, 0, 0}, p1[3] = {0, 0, 140};
        const TrView views[2] = {make_view(2, p0, n, cs), make_view(2, p1, n, cs)};
        std::vector<int> pts;
        axis_breakpoints(views, 2, 2, 0, cs[2], &pts);
        snprintf(where, sizeof(where), "two tiles sharing %d columns", W);
        check("x_shell_is_cut_on_the_rim_only", pts == std::vector<int>({0, 4, 140, 140 + W, cs[2] - 4, cs[2]}));
    }
}

// ---- declined chunks ----
void declines() {
    group = "declines";
    {   // a ninth view on a cell; eight are taken
        for (int nv = 8; nv <= 9; ++nv) {
            Geometry g;
            g.ndim = 2;
            for (int i = 0; i < nv; ++i) { g.origin.push_back({0, (double)i, (double)(2 * i)}); g.shape.push_back({1, 60, 90}); }
            std::vector<TrView> views;
            int cs[3];
            build(g, &views, cs);
            const int t[3] = {0, 0, 0};
            RegionPlan plan;
            mvs_region_plan(views.data(), nv, t, cs, false, &plan);
            snprintf(where, sizeof(where), "%d views on one cell", nv);
            check("declines_on_a_ninth_view_on_a_cell", plan.declined == (nv == 9));
        }
    }
    // 3-D stairs of N views, step 20, (100, 100, 100) voxels each: at most 5 views on a voxel, so the cell count alone decides.
    // (Every cell becomes a region, so an accepted plan has at most 60 000 regions: the 65 535 limit that keeps region ids apart
    // from the padding id cannot be reached -- regions_below_the_padding_id states what it is there for.)
    bool below = false, above = false;
    for (int nv = 4; nv <= 17; ++nv) {
        const int shape[3] = {100, 100, 100};
        const double step[3] = {20, 20, 20};
        Geometry g = stair("cells", 3, nv, shape, step);
        std::vector<TrView> views;
        int cs[3];
        build(g, &views, cs);
        const int t[3] = {0, 0, 0};
        size_t ncell = 1;
        for (int d = 0; d < 3; ++d) {
            std::vector<int> pts;
            axis_breakpoints(views.data(), nv, d, 0, cs[d], &pts);
            ncell *= pts.size() - 1;
        }
        RegionPlan plan;
        mvs_region_plan(views.data(), nv, t, cs, false, &plan);
        snprintf(where, sizeof(where), "stair of %d views, %zu cells", nv, ncell);
        check("declines_on_more_than_60000_cells", plan.declined == (ncell > 60000));
        if (!plan.declined) check("regions_below_the_padding_id", plan.regions.size() == ncell && ncell < 65535);
        (ncell > 60000 ? above : below) = true;
    }
    snprintf(where, sizeof(where), "stairs on both sides of the limit");
    check("declines_on_more_than_60000_cells", below && above);
}

}  // namespace

int main() {
    geometries();
    breakpoints();
    declines();
    for (auto& kv : n_checked) printf("C %s %lld\n", kv.first.c_str(), kv.second);
    for (auto& kv : wrongs) printf("W %s %lld %s\n", kv.first.c_str(), kv.second.wrong, kv.second.wrong ? kv.second.first.c_str() : "-");
    printf("done\n");
    return 0;
}
