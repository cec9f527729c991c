// mvs_region_plan.h -- internal, host only: the plan of the region-decomposed translation fast path (mvs_fuse_region.hip).
//
// For translation-only views the output chunk decomposes along every axis at the view borders into boxes ("regions") inside
// which the set of contributing views is constant.  mvs_region_plan enumerates the regions, classifies per (region, view) whether
// the blend weight is 1 everywhere in the box, picks the class and the brick width of every region and lists the bricks: one
// function from (views, trim, out shape, mixed) to the lists the kernels walk.  Plain host code without a HIP call, so that
// tests/native/region_plan_host_test.cpp can check every decision by brute force over the voxels.
#pragma once
#include "mvs_fuse_tr.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

constexpr int kRB = 4;       // planes per brick
constexpr int kRV = 8;       // voxels per lane
constexpr int kMaxRV = 8;    // views per region handled by the region kernels

struct Region {
    int z0, z1, y0, y1, x0, x1;   // chunk-index box, end exclusive
    int nviews;                   // bits 0-7: views; bits 8-10: lxb (a brick is 8 << lxb voxels wide); bits 12-14: class
    int allone_mask;              // bits 0-7: view ids[v] has blend weight 1 everywhere in the box; bit 15: every view is in
                                  // bounds with a strictly positive weight everywhere (plain weighted sums suffice);
                                  // bits 16-31: view ids[v] covers the box only partially (per-voxel bounds test)
    int ids[kMaxRV];
};
static_assert(sizeof(Region) == 64, "Region layout");

struct Item { int region_bx, by_bz; };   // region | bx << 16 ; by | bz << 16

// What mvs_region_plan hands to the launch code.  `items`: with `mixed` the padded, space-ordered list of the copy / one-view /
// two-view bricks first (mixed_count entries, padding included), then the bricks of classes 0..4, each class contiguous.
struct RegionPlan {
    bool declined = true;         // more than kMaxRV views on a cell, too many cells / regions / bricks: the column kernel fuses
    std::vector<Region> regions;
    std::vector<Item> items;
    int class_count[5] = {0, 0, 0, 0, 0};        // bricks of regions with <=1, 2, <=4, >4 views, and copy-class bricks (in this order)
    double class_in_vox[5] = {0, 0, 0, 0, 0};    // sum over the class's boxes of voxels x views (input voxel reads the class cannot avoid)
    double class_out_vox[5] = {0, 0, 0, 0, 0};   // voxels of the class's boxes
    int mixed_count = 0;
    int bricks = 0;               // items without the padding of the mixed list
};

// Break points of one axis.  View borders that lie within `tol` of each other (tiles of one grid row/column after
// registration differ by a few pixels) are clustered: a cluster of lower borders contributes its minimum, a cluster
// of upper borders (hi + 1) its maximum, so the sliver between the clustered borders falls into the overlap cell,
// where the affected views are flagged "partial", and the single-view interior cells keep full coverage.
inline void axis_breakpoints(const TrView* htr, int n_views, int d, int t, int o, std::vector<int>* out) {
    // kinds: 0 lower border (cluster -> min), 1 upper border + 1 (-> max),
    //        2 end of the lower ramp zone (-> max), 3 start of the upper ramp zone (-> min)
    std::vector<std::pair<int, int>> ev;
    auto clampi = [&](int v) { return std::min(std::max(v, t), t + o); };
    for (int v = 0; v < n_views; ++v) {
        const int lo = htr[v].lo[d], hi = htr[v].hi[d];
        if (lo > hi) continue;
        ev.push_back({clampi(lo), 0});
        ev.push_back({clampi(hi + 1), 1});
        // A thin shell next to every border: inside it the blend weight of the view can round to 0 (the reference
        // outputs 0 there even for a single view, weights.py:502-507); outside it a voxel seen by ONE view is simply
        // the resampled value whatever the weight is, so single-view boxes off the shell need no weights at all.
        // Along x a 4-voxel sliver costs a whole cache line per row and view, so the shell is only cut where it matters:
        // next to a border that no other view covers (the rim of the mosaic).  Inside an overlap the box simply is not
        // flagged "positive" if a weight can vanish there (it cannot, away from the edges of the view).
        const int shell = 4;
        bool cut_lo = true, cut_hi = true;
        if (d == 2) {
            for (int w = 0; w < n_views; ++w) {
                if (w == v || htr[w].lo[2] > htr[w].hi[2]) continue;
                const bool touches = htr[w].lo[0] <= htr[v].hi[0] && htr[w].hi[0] >= htr[v].lo[0] && htr[w].lo[1] <= htr[v].hi[1] &&
                                     htr[w].hi[1] >= htr[v].lo[1];
                if (!touches) continue;
                if (htr[w].lo[2] <= lo - 8 && htr[w].hi[2] >= lo + shell + 8) cut_lo = false;
                if (htr[w].lo[2] <= hi - shell - 8 && htr[w].hi[2] >= hi + 8) cut_hi = false;
            }
        }
        if (2 * shell + 8 < hi - lo + 1) {
            if (cut_lo) ev.push_back({clampi(lo + shell), 2});
            if (cut_hi) ev.push_back({clampi(hi + 1 - shell), 3});
        }
    }
    const int tol = 16;
    out->clear();
    out->push_back(t);
    for (int kind_group = 0; kind_group < 2; ++kind_group) {
        // borders and shell ends are clustered separately so that a shell end never merges with a border
        std::vector<std::pair<int, int>> e2;
        for (auto& e : ev)
            if (e.second / 2 == kind_group) e2.push_back(e);
        std::sort(e2.begin(), e2.end());
        size_t i = 0;
        while (i < e2.size()) {
            size_t j = i;
            bool want_min = false, want_max = false;
            while (j < e2.size() && e2[j].first - e2[i].first <= tol) {
                // lower borders and the starts of upper shells cluster to their minimum, the rest to the maximum
                if (e2[j].second == 0 || e2[j].second == 3) want_min = true; else want_max = true;
                ++j;
            }
            if (want_min) out->push_back(e2[i].first);
            if (want_max) out->push_back(e2[j - 1].first);
            i = j;
        }
    }
    out->push_back(t + o);
    std::sort(out->begin(), out->end());
    out->erase(std::unique(out->begin(), out->end()), out->end());
}

// The plan of the trimmed chunk [t, t + o) for the views htr[0 .. n_views).  plan->declined stays true when the region kernels
// cannot take the chunk (the lists are then unspecified).
inline void mvs_region_plan(const TrView* htr, int n_views, const int t[3], const int o[3], bool mixed_mode, RegionPlan* plan) {
    *plan = RegionPlan();
    std::vector<int> pts[3];
    for (int d = 0; d < 3; ++d) axis_breakpoints(htr, n_views, d, t[d], o[d], &pts[d]);
    const size_t ncell = (pts[0].size() - 1) * (pts[1].size() - 1) * (pts[2].size() - 1);
    if (ncell == 0 || ncell > 60000) return;
    std::vector<Region>& regions = plan->regions;
    std::vector<Item> items_by_class[5];
    double in_vox[5] = {0, 0, 0, 0, 0}, out_vox[5] = {0, 0, 0, 0, 0};
    regions.reserve(ncell);
    std::vector<int> zviews, yviews;
    struct SlabRegion { int rid, nbx, bytes_per_item; };
    std::vector<SlabRegion> slab;              // the mixed-class regions of the current (z, y) slab, in x order
    std::vector<Item> mixed_items;
    std::vector<int> mixed_work;
    for (size_t iz = 0; iz + 1 < pts[0].size(); ++iz) {
        zviews.clear();
        for (int v = 0; v < n_views; ++v)
            if (htr[v].lo[0] < pts[0][iz + 1] && htr[v].hi[0] >= pts[0][iz] && htr[v].lo[1] <= htr[v].hi[1] && htr[v].lo[2] <= htr[v].hi[2]) zviews.push_back(v);
        for (size_t iy = 0; iy + 1 < pts[1].size(); ++iy) {
            slab.clear();
            yviews.clear();
            for (int v : zviews)
                if (htr[v].lo[1] < pts[1][iy + 1] && htr[v].hi[1] >= pts[1][iy]) yviews.push_back(v);
            for (size_t ix = 0; ix + 1 < pts[2].size(); ++ix) {
                Region R;
                memset(&R, 0, sizeof(R));
                R.z0 = pts[0][iz]; R.z1 = pts[0][iz + 1];
                R.y0 = pts[1][iy]; R.y1 = pts[1][iy + 1];
                R.x0 = pts[2][ix]; R.x1 = pts[2][ix + 1];
                int nv = 0;
                bool positive_full = false, all_positive = true;
                for (int v : yviews) {
                    if (!(htr[v].lo[2] < R.x1 && htr[v].hi[2] >= R.x0)) continue;   // does not touch the box
                    if (nv == kMaxRV) return;                                     // too many views: column kernel
                    const bool full = htr[v].lo[0] <= R.z0 && htr[v].hi[0] >= R.z1 - 1 && htr[v].lo[1] <= R.y0 &&
                                      htr[v].hi[1] >= R.y1 - 1 && htr[v].lo[2] <= R.x0 && htr[v].hi[2] >= R.x1 - 1;
                    // the profile is concave, so its minimum over the box sits at one of the 8 corners
                    float wmin = INFINITY;
                    for (int k = 0; k < 8; ++k) {
                        const int z = (k & 4) ? R.z1 - 1 : R.z0, y = (k & 2) ? R.y1 - 1 : R.y0, x = (k & 1) ? R.x1 - 1 : R.x0;
                        wmin = fminf(wmin, tr_weight_profile(htr[v], z, y, x));
                    }
                    const bool unit = full && wmin >= 1.f;          // weight exactly 1 everywhere
                    // weight > 0 everywhere: the float32 ramp (cos(pi (1 - W)) + 1) / 2 only vanishes when the cosine
                    // rounds to -1, i.e. W < 7.8e-5; at W = 3e-4 the cosine is 7 ulp away from -1
                    if (full && wmin >= 3e-4f) positive_full = true;
                    else all_positive = false;
                    if (unit) R.allone_mask |= 1 << nv;
                    if (!full) R.allone_mask |= 1 << (16 + nv);
                    R.ids[nv++] = v;
                }
                if (nv > 0 && all_positive) R.allone_mask |= 1 << 15;
                // profiling only (WRONG results): every view counts as a full unit view, i.e. every brick takes the plain-average
                // path -- the floor of what the weight evaluation can be brought down to
                // (compiled only into profiling builds -- make CXXFLAGS+=-DMVS_PROFILING_ABLATIONS, tools/fuse_floor.sh: a stray
                // environment variable must not be able to corrupt the shipped path's output)
#ifdef MVS_PROFILING_ABLATIONS
                static const bool ablate_unit = getenv("MVS_FUSE_ALL_UNIT") != nullptr;
                if (ablate_unit) R.allone_mask = ((1 << nv) - 1) | (1 << 15);
#endif
                // brick width: 16 voxels for thin boxes, 512 (one full tile row per load instruction: the longest
                // contiguous runs, 4.0 instead of 3.0 TB/s on the copy class) for wide copy-class boxes, else 128
                int lxb = (R.x1 - R.x0 <= 32) ? 1 : 4;
                if (nv == 1 && positive_full && R.x1 - R.x0 > 160) lxb = 6;
                // overlap zones along x (about 100 voxels wide): 64-voxel bricks, so that each brick holds only ONE of the
                // zone's two ramp ends and the other view classifies as "unit" (measured best of 16/32/64/128)
                if (nv >= 2 && R.x1 - R.x0 > 32 && R.x1 - R.x0 <= 136) lxb = 3;
                // (measured, round 4: 256- / 512-voxel bricks for the wide NV >= 2 boxes -- the copy class's layout -- lose:
                // launch 10.06 -> 10.3 / 11.2 ms; every wavefront then spans a ramp end and takes the per-voxel weights)
                const bool copy_class = (nv == 1) && positive_full;   // one full view with positive weight everywhere
                const int cls = copy_class ? 4 : nv <= 1 ? 0 : nv == 2 ? 1 : nv <= 4 ? 2 : 3;
                R.nviews = nv | (lxb << 8) | (cls << 12);
                {
                    const double vox = (double)(R.z1 - R.z0) * (double)(R.y1 - R.y0) * (double)(R.x1 - R.x0);
                    in_vox[cls] += vox * nv;
                    out_vox[cls] += vox;
                }
                const int rid = (int)regions.size();
                if (rid >= 65535) return;                            // (0xffff marks a padding item)
                regions.push_back(R);
                const int bxw = kRV << lxb;
                const int nbz = (R.z1 - R.z0 + kRB - 1) / kRB, nby = (R.y1 - R.y0 + 31) / 32, nbx = (R.x1 - R.x0 + bxw - 1) / bxw;
                if (nbz >= 65536 || nby >= 65536 || nbx >= 65536) return;
                if (mixed_mode && (cls == 4 || cls <= 1)) {         // joins the space-ordered list of this slab (below)
                    slab.push_back(SlabRegion{rid, nbx, std::min(bxw, R.x1 - R.x0) * (std::max(nv, 1) + 1)});
                    continue;
                }
                std::vector<Item>& dst = items_by_class[cls];
                // x fastest, then z, then y: bricks that are neighbours along x share the cache lines at their common
                // edge, neighbours along z share a whole plane when the offsets are fractional; both reuses then happen
                // within a few bricks, i.e. inside the L2 of the XCD that owns this stretch of the list
                for (int by = 0; by < nby; ++by)
                    for (int bz = 0; bz < nbz; ++bz)
                        for (int bx = 0; bx < nbx; ++bx) dst.push_back({rid | (bx << 16), by | (bz << 16)});
            }
            if (!slab.empty()) {
                // one (z, y) slab of the cell grid: its regions share the z / y extents and the brick grid; y block, then z
                // block, then ALL regions along x -- so the bricks of a row of the mosaic are neighbours in the list whatever
                // their class
                const int z0s = pts[0][iz], z1s = pts[0][iz + 1], y0s = pts[1][iy], y1s = pts[1][iy + 1];
                const int nbz = (z1s - z0s + kRB - 1) / kRB, nby = (y1s - y0s + 31) / 32;
                for (int by = 0; by < nby; ++by)
                    for (int bz = 0; bz < nbz; ++bz)
                        for (const SlabRegion& sr : slab)
                            for (int bx = 0; bx < sr.nbx; ++bx) {
                                mixed_items.push_back({sr.rid | (bx << 16), by | (bz << 16)});
                                mixed_work.push_back(sr.bytes_per_item);
                            }
            }
        }
    }
    std::vector<Item>& items = plan->items;
    if (!mixed_items.empty()) {
        // eight stretches of equal WORK (bytes moved), one per XCD (see the workgroup -> item mapping of the kernels), padded to
        // one length with no-op items
        long long total = 0;
        for (int w : mixed_work) total += w;
        size_t cut[9];
        cut[0] = 0;
        long long acc = 0;
        size_t i = 0;
        for (int k = 1; k <= 8; ++k) {
            const long long target = total * k / 8;
            while (i < mixed_items.size() && acc < target) acc += mixed_work[i++];
            cut[k] = k == 8 ? mixed_items.size() : i;
        }
        size_t longest = 0;
        for (int k = 0; k < 8; ++k) longest = std::max(longest, cut[k + 1] - cut[k]);
        const size_t L = (longest + 3) / 4 * 4;
        items.reserve(8 * L);
        for (int k = 0; k < 8; ++k) {
            items.insert(items.end(), mixed_items.begin() + (long)cut[k], mixed_items.begin() + (long)cut[k + 1]);
            items.resize((size_t)(k + 1) * L, Item{0xffff, 0});
        }
        plan->mixed_count = (int)items.size();
    }
    plan->bricks = (int)mixed_items.size();
    for (int k = 0; k < 5; ++k) {
        plan->class_count[k] = (int)items_by_class[k].size();
        plan->class_in_vox[k] = in_vox[k];
        plan->class_out_vox[k] = out_vox[k];
        plan->bricks += plan->class_count[k];
        items.insert(items.end(), items_by_class[k].begin(), items_by_class[k].end());
    }
    if (items.empty() || items.size() > (1u << 28)) return;
    plan->declined = false;
}
