// Host-side run of csrc/mvs_region_plan.h (the plan of the region fuse kernels: regions, flags, classes, brick lists; no HIP call).
// tests/test_region_plan_host.py builds this with hipcc (no GPU needed) and reads
//   C <group> <n checked>                         one per group of properties
//   W <property> <n wrong> <first wrong case>     one per property
// Every property is checked by brute force over the voxels of small chunks: the flags of a region are promises about EVERY voxel of
// its box (the planner itself looks at the 8 corners only and relies on the concavity of the weight profile), and a wrong flag
// gives wrong voxels in a few cells only.  The views are made by hand (make_view, tr_view_by_hand.h) the way
// prepare_translation_view (mvs_fuse_chunk_plan.h) and weights.blending_supports derive them for unit spacings -- which
// fuse_chunk_plan_host_test.cpp checks against the real code: a view of n pixels whose first pixel lies at chunk coordinate p has
// the valid box [ceil(p), floor(p + n - 1)], support nodes 0 and 4 at p - 1 and p + n, (n + 1) / 4 pixels per node and the tent
// scale (n + 1) / 4 / blending width, clipped to twice another axis's as the support table holds it.
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
#include "tr_view_by_hand.h"

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

void run(const Geometry& g) {
    check_plan(g, false);
    check_plan(g, true);
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
    geometries(run);
    breakpoints();
    declines();
    for (auto& kv : n_checked) printf("C %s %lld\n", kv.first.c_str(), kv.second);
    for (auto& kv : wrongs) printf("W %s %lld %s\n", kv.first.c_str(), kv.second.wrong, kv.second.wrong ? kv.second.first.c_str() : "-");
    printf("done\n");
    return 0;
}
