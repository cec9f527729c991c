// Host-side run of csrc/mvs_fuse_chunk_plan.h (what the chunk entries of mvs_fuse.hip decide without the device; no HIP call).
// tests/test_fuse_chunk_plan_host.py builds this with hipcc (no GPU needed) and reads
//   C <group> <n checked>                         one per group of properties
//   W <property> <n wrong> <first wrong case>     one per property
//   R <route> <n cases>                           one per distinct sequence of kernel families a chunk was sent through
//   N <name> <value>                              sizes of the sweeps
// Groups: valid_range (a), records (b), hand_views (c), routes (d), layouts (e), boxes (f).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "mvs_fuse_chunk_plan.h"
#include "tr_view_by_hand.h"

namespace P = mvs_fuse_chunk_plan;

namespace {

std::map<std::string, long long> n_checked, n_named, n_routes;
struct Wrong { long long wrong = 0; std::string first; };
std::map<std::string, Wrong> wrongs;
const char* group = "";
char where[320] = "";

void check(const char* prop, bool ok) {
    ++n_checked[group];
    Wrong& w = wrongs[prop];
    if (ok) return;
    if (!w.wrong) w.first = where;
    ++w.wrong;
}

template <typename T>
bool same_bits(const T& a, const T& b) { return memcmp(&a, &b, sizeof(T)) == 0; }

// ---- a. exact_valid_range against the index-by-index walk -----------------------------------------------------------------------
void valid_range() {
    group = "valid_range";
    const long long shifts[4] = {0, 3, -3, 1ll << 20};
    long long nonempty = 0, cases = 0;
    for (int n : {1, 2, 5, 64})
        for (int chunk : {1, 7, 40})
            for (long long org : shifts)
                for (long long ioff : shifts) {
                    const double b = (double)(ioff - org);      // with off = b the slab's first pixel is chunk index 0
                    std::vector<double> offs;
                    for (int j : {-3, -1, 0, 1, 4}) offs.push_back(b + j);
                    for (int j : {-2, 0, 3}) offs.push_back(b + j + 0.5);
                    for (int j : {-1, 0, 2}) { offs.push_back(nextafter(b + j, INFINITY)); offs.push_back(nextafter(b + j, -INFINITY)); }
                    offs.push_back(1048576.0 - 0.25);
                    offs.push_back(-(1048576.0 - 0.25));
                    offs.push_back(b - (chunk + 5));      // entirely before the chunk
                    offs.push_back(b + (n + 5));          // entirely after it
                    for (double off : offs) {
                        int lo, hi;
                        P::exact_valid_range(off, n, chunk, &lo, &hi, org, ioff);
                        snprintf(where, sizeof(where), "n %d chunk %d org %lld ioff %lld off %.17g -> [%d, %d]", n, chunk, org, ioff, off, lo, hi);
                        bool equal = true, any = false;
                        for (int i = 0; i < chunk; ++i) {
                            const double c = (double)((long long)i + org) + off;
                            const bool in = c >= (double)ioff && c <= (double)(ioff + n - 1);
                            any = any || in;
                            equal = equal && in == (i >= lo && i <= hi);
                        }
                        check("range_equals_the_walk", equal);
                        check("empty_exactly_when_lo_exceeds_hi", any == (lo <= hi));
                        nonempty += any;
                        ++cases;
                    }
                }
    n_named["valid_range_cases"] = cases;
    n_named["valid_range_nonempty"] = nonempty;
}

// ---- a view the way fusion.py describes a tile of n pixels whose first pixel lies at frame coordinate p (unit spacings): identity
// matrix, offset -p, support grid w_matrix = 1 / S, w_offset = -(p - 1) / S, edt = the closed form with (float)(S / blend) ----
DevView tile_view(int ndim, const double p[3], const int n[3]) {
    DevView d;
    memset(&d, 0, sizeof(d));
    d.data = nullptr;
    d.nz = n[0]; d.ny = n[1]; d.nx = n[2];
    d.stride_y = n[2];
    d.stride_z = (long long)n[2] * n[1];
    d.wnz = ndim == 3 ? 5 : 1;
    float ws[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k) {
        d.m[4 * k] = 1.0;
        d.off[k] = -p[k];
        d.wm[4 * k] = 1.0;
        if (k == 0 && ndim == 2) continue;
        const double S = (double)(n[k] + 1) / 4.0;
        d.wm[4 * k] = 1.0 / S;
        d.woff[k] = -(p[k] - 1.0) / S;
        ws[k] = (float)(S / kBlend[k]);
    }
    for (int i = 0; i < d.wnz; ++i)
        for (int j = 0; j < 5; ++j)
            for (int k = 0; k < 5; ++k) {
                float t = fminf(ws[1] * (float)std::min(j, 4 - j), ws[2] * (float)std::min(k, 4 - k));
                if (d.wnz == 5) t = fminf(t, ws[0] * (float)std::min(i, 4 - i));
                d.edt[(i * 5 + j) * 5 + k] = t;
            }
    return d;
}

const double kOrigins[5][3] = {{3.25, -2.5, 7.0}, {0.0, 0.0, 0.0}, {-4.0, 11.0, -0.5}, {1.0 / 3.0, 5.875, -7.0 / 9.0}, {12.5, 6.0, 2.0 - 1e-9}};

bool prepare(DevView* d, int order, int fusion, const int64_t cs[3], size_t es, const int64_t org[3], const int64_t ioff[3], TrView* t) {
    return P::tr_view_in_chunk(d, order, fusion, cs, es, org, ioff, t);
}

void records() {
    group = "records";
    const int n3[3] = {12, 30, 40};
    // accepted views at order 0 and 1: io, fw are the round / floor split of off + org - ioff
    for (int v = 0; v < 5; ++v)
        for (int order = 0; order < 2; ++order) {
            const int64_t cs[3] = {24, 40, 64}, org[3] = {5, -3, 0}, ioff[3] = {2, 0, 4};
            DevView d = tile_view(3, kOrigins[v], n3);
            const double off[3] = {d.off[0], d.off[1], d.off[2]};
            TrView t;
            snprintf(where, sizeof(where), "view %d order %d", v, order);
            check("plain_view_is_accepted", prepare(&d, order, MVS_FUSE_WEIGHTED_AVERAGE, cs, 2, org, ioff, &t) && d.tr_ok == 1 && t.linear == order);
            for (int k = 0; k < 3; ++k) {
                const double whole = order ? floor(off[k]) : floor(off[k] + 0.5);
                check("io_is_the_whole_part_of_the_offset_plus_the_index_shifts", t.io[k] == (long long)whole + org[k] - ioff[k] && t.io[k] == d.io[k]);
                check("fw_is_the_fraction_in_0_1_and_0_at_order_0",
                      t.fw[k] >= 0.f && t.fw[k] < 1.f && same_bits(t.fw[k], order ? (float)(off[k] - whole) : 0.f) && same_bits(t.fw[k], d.fw[k]));
            }
        }
    // the same view through chunks whose origin differs by d per axis
    for (int v = 0; v < 5; ++v)
        for (int64_t dd : {1, 37, 4096}) {
            const int64_t cs[3] = {8192, 8192, 8192}, org1[3] = {-5000, -5000, -5000}, org2[3] = {-5000 + dd, -5000 + dd, -5000 + dd}, ioff[3] = {1, 0, 2};
            DevView d1 = tile_view(3, kOrigins[v], n3), d2 = d1;
            TrView a, b;
            snprintf(where, sizeof(where), "view %d d %lld", v, (long long)dd);
            const bool ok1 = prepare(&d1, 1, MVS_FUSE_WEIGHTED_AVERAGE, cs, 2, org1, ioff, &a), ok2 = prepare(&d2, 1, MVS_FUSE_WEIGHTED_AVERAGE, cs, 2, org2, ioff, &b);
            check("plain_view_is_accepted", ok1 && ok2);
            check("fw_does_not_depend_on_the_chunk", same_bits(a.fw, b.fw));
            check("sup_flo_does_not_depend_on_the_chunk", same_bits(a.sup_flo, b.sup_flo));
            check("sup_fhi_does_not_depend_on_the_chunk", same_bits(a.sup_fhi, b.sup_fhi));
            check("sup_k_does_not_depend_on_the_chunk", same_bits(a.sup_k, b.sup_k));
            check("ws_does_not_depend_on_the_chunk", same_bits(a.ws, b.ws));
            bool io = true, ilo = true, ihi = true, lo = true, hi = true;
            for (int k = 0; k < 3; ++k) {
                io = io && b.io[k] - a.io[k] == dd;                  // slab pixel = chunk index + io: a later origin, a larger io
                ilo = ilo && a.sup_ilo[k] - b.sup_ilo[k] == dd;      // chunk index = frame index - org
                ihi = ihi && a.sup_ihi[k] - b.sup_ihi[k] == dd;
                lo = lo && a.lo[k] - b.lo[k] == dd && b.lo[k] > 0;   // (inside both chunks: not clamped)
                hi = hi && a.hi[k] - b.hi[k] == dd && a.hi[k] < cs[k] - 1 && a.hi[k] - a.lo[k] == n3[k] - 1 - (a.fw[k] != 0.f);
            }
            check("io_shifts_by_d", io);
            check("sup_ilo_shifts_by_d", ilo);
            check("sup_ihi_shifts_by_d", ihi);
            check("lo_shifts_by_d", lo);
            check("hi_shifts_by_d", hi);
        }
    // refusals: a 2-D view that is accepted, one change each that is refused, and where there is one the nearest accepted neighbour
    struct Case { int n[3]; int64_t cs[3], org[3], ioff[3]; size_t es; int fusion; DevView d; };
    auto base = [&](int ny = 30, int nx = 40) {
        Case c = {{1, ny, nx}, {1, 64, 64}, {0, 0, 0}, {0, 0, 0}, 4, MVS_FUSE_WEIGHTED_AVERAGE, DevView()};
        const double p[3] = {0.0, 3.25, -2.5};
        c.d = tile_view(2, p, c.n);
        return c;
    };
    auto accepted = [&](Case c) { TrView t; return prepare(&c.d, 1, c.fusion, c.cs, c.es, c.org, c.ioff, &t) && c.d.tr_ok == 1; };
    auto refuse = [&](const char* what, const Case& c) { snprintf(where, sizeof(where), "%s", what); check("refused", !accepted(c)); };
    auto accept = [&](const char* what, const Case& c) { snprintf(where, sizeof(where), "%s", what); check("neighbour_of_a_refusal_is_accepted", accepted(c)); };
    auto under_max = [&](const char* what, Case c) { snprintf(where, sizeof(where), "%s", what); c.fusion = MVS_FUSE_MAX; check("weighted_average_refusal_is_accepted_under_max", accepted(c)); };
    { Case c = base(); accept("the plain view", c); }
    { Case c = base(); c.d.m[1] = 1e-9; refuse("matrix is not the identity", c); }
    { Case c = base(); c.d.off[2] = 1048576.0; c.org[2] = -1048570; refuse("|off| = 2^20", c);
      c.d.off[2] = nextafter(1048576.0, 0.0); accept("|off| just below 2^20", c); }
    { Case c = base(30, 65537); refuse("slab axis of 65537", c); c = base(30, 65536); accept("slab axis of 65536", c); }
    { Case c = base(); c.cs[1] = 65537; refuse("chunk axis of 65537", c); c.cs[1] = 65536; accept("chunk axis of 65536", c); }
    { Case c = base(); c.org[1] = (1 << 24) + 1; c.ioff[1] = 1 << 24; refuse("|org| = 2^24 + 1", c);
      c.org[1] = 1 << 24; c.ioff[1] = (1 << 24) + 1; refuse("|ioff| = 2^24 + 1", c);
      c.ioff[1] = 1 << 24; accept("|org| = |ioff| = 2^24", c); }
    { Case c = base(); c.d.off[2] = 0.5; c.org[2] = 65536; refuse("off + org - ioff = 65536.5", c); c.org[2] = 65535; accept("off + org - ioff = 65535.5", c); }
    { Case c = base(); c.d.wm[5] = 1e-12; refuse("w_matrix off the diagonal", c); under_max("w_matrix off the diagonal", c); }
    { Case c = base(); c.d.edt[2 * 5 + 2] = nextafterf(c.d.edt[2 * 5 + 2], INFINITY); refuse("edt one ulp off the closed form", c); under_max("edt one ulp off the closed form", c); }
    { Case c = base(); c.d.wm[4] = 0.0; refuse("w_matrix diagonal 0", c); under_max("w_matrix diagonal 0", c);
      c.d.wm[4] = -0.25; refuse("w_matrix diagonal negative", c); under_max("w_matrix diagonal negative", c); }
    { Case c = base(); c.d.woff[2] = -2e6 * c.d.wm[8]; refuse("support node 0 at 2e6", c); under_max("support node 0 at 2e6", c); }
    { Case c = base(1, 40); c.d.stride_y = -1; refuse("negative stride", c);
      c.d.stride_y = 0x80000000LL; refuse("stride of 2^31", c); c.d.stride_y = 0x7fffffffLL; accept("stride of 2^31 - 1", c); }
    { Case c = base(2, 40); c.d.stride_y = 503316480 - 40; refuse("span of 2^31 - 2^27 bytes", c); c.d.stride_y -= 1; accept("span one element less", c); }
    { Case c = base(); c.d.stride_z = 1 << 24; refuse("stride_z of 2^26 bytes", c); c.d.stride_z -= 1; accept("stride_z one element less", c); }
}

// ---- c. the views tests make by hand (tr_view_by_hand.h) are the ones the real code derives ----------------------------------------
void hand_view_equals_real(const Geometry& g) {
    std::vector<TrView> hand;
    int cs[3];
    build(g, &hand, cs);
    double mn[3] = {1e30, 1e30, 1e30};
    for (size_t i = 0; i < g.origin.size(); ++i)
        for (int k = 0; k < 3; ++k) mn[k] = std::min(mn[k], g.origin[i][k]);
    const int64_t cs64[3] = {cs[0], cs[1], cs[2]}, zero[3] = {0, 0, 0};
    for (size_t i = 0; i < g.origin.size(); ++i) {
        double p[3];
        for (int k = 0; k < 3; ++k) p[k] = g.origin[i][k] - mn[k];
        DevView d = tile_view(g.ndim, p, g.shape[i].data());
        TrView t;
        const TrView& h = hand[i];
        snprintf(where, sizeof(where), "%s view %zu", g.name.c_str(), i);
        check("hand_view_is_accepted", prepare(&d, 1, MVS_FUSE_WEIGHTED_AVERAGE, cs64, 2, zero, zero, &t));
        check("hand_view_wnz_linear_n", t.wnz == h.wnz && t.linear == h.linear && same_bits(t.n, h.n));
        check("hand_view_io", same_bits(t.io, h.io));
        check("hand_view_fw", same_bits(t.fw, h.fw));
        check("hand_view_lo_hi", same_bits(t.lo, h.lo) && same_bits(t.hi, h.hi));
        check("hand_view_sup_k", same_bits(t.sup_k, h.sup_k));
        check("hand_view_sup_ilo_ihi", same_bits(t.sup_ilo, h.sup_ilo) && same_bits(t.sup_ihi, h.sup_ihi));
        check("hand_view_sup_flo_fhi", same_bits(t.sup_flo, h.sup_flo) && same_bits(t.sup_fhi, h.sup_fhi));
        check("hand_view_ws", same_bits(t.ws, h.ws));
        // (where one spacing scale exceeds twice another the table holds -- and both sides carry -- the smaller, clipped one)
        bool is_clipped = false;
        for (int k = 3 - g.ndim; k < 3; ++k) is_clipped = is_clipped || h.ws[k] != (float)((double)(g.shape[i][k] + 1) / 4.0 / kBlend[k]);
        n_named["hand_views_with_a_clipped_scale"] += is_clipped;
        check("hand_view_strides_span", t.stride_y == h.stride_y && t.stride_z == h.stride_z && t.span == h.span);
        ++n_named["hand_views"];
    }
}

void hand_views() {
    group = "hand_views";
    geometries(hand_view_equals_real);
    char name[64];
    for (int i = 0; i < 10; ++i) {      // ten more: 2-D and 3-D in turn, integer and fractional origins in pairs
        const int ndim = 2 + (i & 1);
        const int tiles[3] = {ndim == 3 ? 2 : 1, rnd_int(1, 3), rnd_int(1, 3)};
        const int shape[3] = {ndim == 3 ? rnd_int(5, 40) : 1, rnd_int(9, 300), rnd_int(9, 700)};
        const int overlap[3] = {ndim == 3 ? rnd_int(1, 4) : 0, rnd_int(1, 8), rnd_int(1, 8)};
        snprintf(name, sizeof(name), "more_random_%d", i);
        hand_view_equals_real(grid(name, ndim, tiles, shape, overlap, rnd_int(0, 6), (i & 2) != 0));
    }
}

// ---- d. the route against the conditions the driver evaluated inline before the plan existed ---------------------------------------
struct Walk {
    std::string asked;         // families asked in turn
    std::string checks;        // grids whose block count is checked, in turn (T: column bricks, G: generic bricks); repeats folded
    std::string launches;      // grids of the column / generic launches
    int counters[4] = {0, 0, 0, 0};      // rows, region, column, generic
    bool records = false;      // cull boxes, translation records, x-table offsets are built
    bool flag_read = false;
    void checked(char k) { if (checks.empty() || checks.back() != k) checks += k; }
};
struct Chunk { int dtype, order, fusion; bool dct, all_tr_ok, force_generic, rows_v1, no_regions; int n_views; bool rows_take, regions_take, overflow; };

// the driver's predicates before this header, verbatim; the family calls replaced by what the case says they answer
Walk before(const Chunk& q) {
    Walk w;
    const int dtype = q.dtype, n_views = q.n_views;
    const struct { int order, fusion; } o = {q.order, q.fusion}, *opts = &o;
    const struct { bool force_generic, rows_v1, no_regions; } cc = {q.force_generic, q.rows_v1, q.no_regions}, *c = &cc;
    const bool dct = q.dct;
    bool use_tr = !c->force_generic && !dct;
    for (int i = 0; i < n_views && use_tr; ++i) use_tr = q.all_tr_ok;
    const bool nan_exact = (dtype == MVS_F32 && opts->order == 1);
    if (nan_exact && opts->fusion != MVS_FUSE_WEIGHTED_AVERAGE) use_tr = false;
    w.records = use_tr;
    char grid_kind = 0;
    auto set_brick_grid = [&](bool tr) { grid_kind = tr ? 'T' : 'G'; w.checked(grid_kind); };
    auto launch_generic = [&] { w.asked += " generic"; w.launches += grid_kind; };
    set_brick_grid(use_tr);
    bool regions_done = false;
    if (!regions_done && use_tr && opts->fusion == MVS_FUSE_WEIGHTED_AVERAGE && (c->rows_v1 || (dtype == MVS_F32 && opts->order == 1))) {
        w.asked += " rows";
        regions_done = q.rows_take;
        if (regions_done) w.counters[0] += 1;
    }
    if (!regions_done && nan_exact && use_tr) {
        use_tr = false;
        set_brick_grid(false);
    }
    if (!regions_done && use_tr && opts->fusion == MVS_FUSE_WEIGHTED_AVERAGE && !c->no_regions) {
        w.asked += " regions";
        regions_done = q.regions_take;
        if (regions_done) w.counters[1] += 1;
    }
    if (regions_done) {
    } else if (use_tr) {
        w.asked += " column";
        w.launches += grid_kind;
        w.counters[2] += 1;
    } else {
        launch_generic();
        w.counters[3] += 1;
    }
    if (use_tr && !regions_done && n_views > 64) {
        w.flag_read = true;
        if (q.overflow) {
            set_brick_grid(false);
            launch_generic();
            w.counters[3] += 1;
        }
    }
    return w;
}

// the driver as it walks the plan
Walk after(const Chunk& q) {
    Walk w;
    const P::Route R = P::route(P::RouteInputs{q.dtype, q.order, q.fusion, q.dct, q.all_tr_ok, q.force_generic, q.rows_v1, q.no_regions, q.n_views});
    auto kind = [](P::GridKind k) { return k == P::kTrBricks ? 'T' : 'G'; };
    auto generic = [&] { w.checked(kind(P::family_grid(P::kGeneric))); w.asked += " generic"; w.launches += kind(P::family_grid(P::kGeneric)); w.counters[3] += 1; };
    w.records = R.use_tr;
    w.checked(kind(R.first_grid));
    bool done = false;
    if (R.try_rows) { w.asked += " rows"; done = q.rows_take; if (done) w.counters[0] += 1; }
    if (!done && R.try_regions) { w.asked += " regions"; done = q.regions_take; if (done) w.counters[1] += 1; }
    if (!done) {
        if (R.fallback == P::kColumn) { w.asked += " column"; w.launches += kind(P::family_grid(P::kColumn)); w.counters[2] += 1; }
        else generic();
    }
    if (!done && R.read_overflow) {
        w.flag_read = true;
        if (q.overflow) generic();
    }
    if (!done && kind(R.grid) != w.launches[0]) w.launches = "?";      // Route::grid is the fallback's grid
    return w;
}

void routes() {
    group = "routes";
    long long total = 0;
    for (int dtype : {MVS_U8, MVS_U16, MVS_F32})
        for (int order = 0; order < 2; ++order)
            for (int fusion : {MVS_FUSE_WEIGHTED_AVERAGE, MVS_FUSE_MAX, MVS_FUSE_SIMPLE_AVERAGE})
                for (int bits = 0; bits < 256; ++bits)
                    for (int n_views : {1, 64, 65}) {
                        const Chunk q = {dtype, order, fusion, (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0,
                                         n_views, (bits & 32) != 0, (bits & 64) != 0, (bits & 128) != 0};
                        const Walk a = before(q), b = after(q);
                        snprintf(where, sizeof(where), "dtype %d order %d fusion %d dct %d tr_ok %d force_generic %d rows_v1 %d no_regions %d views %d take %d %d overflow %d:%s |%s",
                                 dtype, order, fusion, q.dct, q.all_tr_ok, q.force_generic, q.rows_v1, q.no_regions, n_views, q.rows_take, q.regions_take, q.overflow,
                                 a.asked.c_str(), b.asked.c_str());
                        check("families_asked_and_the_one_that_fuses", a.asked == b.asked);
                        check("counters_bumped", memcmp(a.counters, b.counters, sizeof(a.counters)) == 0);
                        check("grids_checked_and_launched", a.checks == b.checks && a.launches == b.launches);
                        check("overflow_flag_read", a.flag_read == b.flag_read);
                        check("records_built", a.records == b.records);
                        std::string name = a.asked.substr(1);
                        std::replace(name.begin(), name.end(), ' ', '_');
                        ++n_routes[name];
                        ++total;
                    }
    n_named["route_cases"] = total;
}

// ---- e. layouts ---------------------------------------------------------------------------------------------------------------------
void layouts() {
    group = "layouts";
    for (int n_views : {1, 2, 8, 64, 65, 4096}) {
        const P::ParamBlock b = P::param_block(n_views);
        snprintf(where, sizeof(where), "%d views", n_views);
        // (the driver's lines)
        const size_t views_bytes = align_up(sizeof(DevView) * (size_t)n_views);
        const size_t cull_bytes = align_up(sizeof(int) * 6 * (size_t)n_views);
        const size_t params_bytes = views_bytes + cull_bytes + sizeof(TrView) * (size_t)n_views;
        check("parts_on_256_bytes", b.views % 256 == 0 && b.cull % 256 == 0 && b.tr % 256 == 0);
        check("parts_ordered_and_disjoint", b.views + sizeof(DevView) * (size_t)n_views <= b.cull && b.cull + sizeof(int) * 6 * (size_t)n_views <= b.tr &&
                                                b.tr + sizeof(TrView) * (size_t)n_views <= b.total);
        check("parts_where_the_driver_had_them", b.views == 0 && b.cull == views_bytes && b.tr == views_bytes + cull_bytes);
        check("total_is_params_bytes", b.total == params_bytes);
    }
    const int sizes[10] = {1, 3, 4, 5, 16, 17, 63, 64, 65, 257};
    for (int oz : sizes)
        for (int oy : sizes)
            for (int ox : sizes)
                for (int tr = 0; tr < 2; ++tr) {
                    const int64_t os[3] = {oz, oy, ox};
                    const P::BrickGrid g = P::brick_grid(tr ? P::kTrBricks : P::kGenericBricks, os);
                    snprintf(where, sizeof(where), "%d x %d x %d %s", oz, oy, ox, tr ? "column" : "generic");
                    const int bx = tr ? P::kTrBrickX : P::kBrickX;
                    check("bricks_cover_the_result_and_none_is_empty", (long long)g.nbz * g.bz >= oz && (long long)(g.nbz - 1) * g.bz < oz && (long long)g.nby * g.by >= oy &&
                                                                           (long long)(g.nby - 1) * g.by < oy && (long long)g.nbx * bx >= ox && (long long)(g.nbx - 1) * bx < ox);
                    // (the driver's lambda, its constants written out)
                    struct { int oz, oy, ox, bz, by, nbz, nby, nbx; } Q = {oz, oy, ox, 0, 0, 0, 0, 0};
                    long long nblocks = 0;
                    if (tr) {
                        Q.bz = (os[0] > 1) ? 4 : 1;
                        Q.by = (os[0] > 1) ? 4 * 8 : 4 * 4 * 8;
                    } else {
                        Q.bz = (os[0] > 1) ? 4 : 1;
                        Q.by = (os[0] > 1) ? 4 : 16;
                    }
                    const int brick_x = tr ? 256 : 64;
                    Q.nbz = (Q.oz + Q.bz - 1) / Q.bz;
                    Q.nby = (Q.oy + Q.by - 1) / Q.by;
                    Q.nbx = (Q.ox + brick_x - 1) / brick_x;
                    nblocks = (long long)Q.nbz * Q.nby * Q.nbx;
                    check("grid_is_the_drivers", g.bz == Q.bz && g.by == Q.by && g.nbz == Q.nbz && g.nby == Q.nby && g.nbx == Q.nbx && g.nblocks == nblocks &&
                                                     g.fits_one_launch() == !(nblocks > 0x7fffffffLL));
                }
    {   // 2048 x 2048 x 512 bricks of the generic kernel are 2^31 blocks: one too many; a brick less along x fits
        const int64_t big[3] = {8192, 8192, 32768}, less[3] = {8192, 8192, 32768 - 64};
        snprintf(where, sizeof(where), "8192 x 8192 x 32768");
        check("launch_limit_is_2_31_minus_1_blocks", P::brick_grid(P::kGenericBricks, big).nblocks == (1ll << 31) && !P::brick_grid(P::kGenericBricks, big).fits_one_launch());
        check("launch_limit_is_2_31_minus_1_blocks", P::brick_grid(P::kGenericBricks, less).fits_one_launch() && P::brick_grid(P::kTrBricks, big).fits_one_launch());
        P::BrickGrid g = P::brick_grid(P::kGenericBricks, less);
        g.nblocks = 0x7fffffffLL;
        check("launch_limit_is_2_31_minus_1_blocks", g.fits_one_launch());
        g.nblocks += 1;
        check("launch_limit_is_2_31_minus_1_blocks", !g.fits_one_launch());
    }
    {   // x-weight table: three views, one of them empty along x
        const int lo[3] = {0, 7, 30}, hi[3] = {19, 6, 300};
        size_t total = 0, xtab_total = 0;
        bool same = true;
        for (int i = 0; i < 3; ++i) {
            const int off = P::xtab_add(&total, lo[i], hi[i]);
            const int want = (int)xtab_total + 4;      // (the driver's lines, kXTabMargin = 4)
            xtab_total += (size_t)std::max(hi[i] - lo[i] + 1, 0) + 2 * 4;
            same = same && off == want && total == xtab_total;
        }
        snprintf(where, sizeof(where), "x-weight table");
        check("xtab_offsets_and_total_are_the_drivers", same && total == 20 + 0 + 271 + 24);
        check("xtab_scratch_is_the_drivers", P::xtab_bytes(total) == (xtab_total + 64) * sizeof(float) + 256 && P::xtab_overflow_at(total) == xtab_total + 64 &&
                                                 (P::xtab_overflow_at(total) + 1) * sizeof(float) <= P::xtab_bytes(total));
    }
}

// ---- f. chunk boxes -----------------------------------------------------------------------------------------------------------------
void boxes() {
    group = "boxes";
    const int n[3] = {9, 14, 11};
    const int64_t cs[3] = {24, 20, 28};
    for (int v = 0; v < 5; ++v) {
        const DevView d = tile_view(3, kOrigins[v], n);
        int lo[3], hi[3];
        P::view_chunk_box(d, cs, lo, hi);
        for (int k = 0; k < 3; ++k) {
            bool equal = true;
            for (int i = 0; i < cs[k]; ++i) {
                const double c = (double)i + d.off[k];
                equal = equal && (c >= 0.0 && c <= (double)(n[k] - 1)) == (i >= lo[k] && i <= hi[k]);
            }
            snprintf(where, sizeof(where), "view %d axis %d [%d, %d]", v, k, lo[k], hi[k]);
            check("identity_box_equals_the_walk", equal);
        }
    }
    const double c30 = cos(M_PI / 6.0), s30 = sin(M_PI / 6.0);
    const struct { const char* name; double m[9]; } turned[4] = {
        {"90 degrees about z", {1, 0, 0, 0, 0, -1, 0, 1, 0}},
        {"30 degrees about z", {1, 0, 0, 0, c30, -s30, 0, s30, c30}},
        {"mirror along x", {1, 0, 0, 0, 1, 0, 0, 0, -1}},
        {"anisotropic scale", {0.5, 0, 0, 0, 1.25, 0, 0, 0, 0.75}}};
    for (const auto& T : turned) {
        DevView d = tile_view(3, kOrigins[1], n);
        memcpy(d.m, T.m, sizeof(d.m));
        for (int k = 0; k < 3; ++k) {      // the chunk's centre lands on the slab's centre, a fraction off
            const double cc[3] = {(cs[0] - 1) / 2.0, (cs[1] - 1) / 2.0, (cs[2] - 1) / 2.0};
            d.off[k] = (n[k] - 1) / 2.0 + 0.3 - (cc[0] * d.m[3 * k] + cc[1] * d.m[3 * k + 1] + cc[2] * d.m[3 * k + 2]);
        }
        int lo[3], hi[3];
        P::view_chunk_box(d, cs, lo, hi);
        long long inside = 0, outside_box = 0;
        for (int z = 0; z < cs[0]; ++z)
            for (int y = 0; y < cs[1]; ++y)
                for (int x = 0; x < cs[2]; ++x) {
                    bool in = true;
                    for (int k = 0; k < 3; ++k) {
                        const double c = (((double)z * d.m[3 * k] + (double)y * d.m[3 * k + 1]) + (double)x * d.m[3 * k + 2]) + d.off[k];
                        in = in && !(c < 0.0 || c > (double)(n[k] - 1));
                    }
                    if (!in) continue;
                    ++inside;
                    if (z < lo[0] || z > hi[0] || y < lo[1] || y > hi[1] || x < lo[2] || x > hi[2]) ++outside_box;
                }
        snprintf(where, sizeof(where), "%s: %lld voxels in bounds, %lld of them outside [%d, %d] x [%d, %d] x [%d, %d]", T.name, inside, outside_box, lo[0], hi[0], lo[1],
                 hi[1], lo[2], hi[2]);
        check("turned_view_reaches_the_chunk", inside > 0);
        check("turned_box_holds_every_voxel_in_bounds", outside_box == 0);
    }
}

}  // namespace

int main() {
    valid_range();
    records();
    hand_views();
    routes();
    layouts();
    boxes();
    for (auto& kv : n_checked) printf("C %s %lld\n", kv.first.c_str(), kv.second);
    for (auto& kv : wrongs) printf("W %s %lld %s\n", kv.first.c_str(), kv.second.wrong, kv.second.wrong ? kv.second.first.c_str() : "-");
    for (auto& kv : n_routes) printf("R %s %lld\n", kv.first.c_str(), kv.second);
    for (auto& kv : n_named) printf("N %s %lld\n", kv.first.c_str(), kv.second);
    printf("done\n");
    return 0;
}
