// Host-side run of csrc/mvs_cb_plan.h (the plan of a content-based chunk: integers and small structs, no HIP call).
// tests/test_cb_plan_host.py builds this with hipcc (no GPU needed) and reads
//   C <group> <n checked>                         one per group of properties
//   W <property> <n wrong> <first wrong case>     one per property
// The properties are stated in terms of what the kernels need (powers of two, LDS bytes, disjoint ranges, who reads what), not as
// a second copy of the rules.  Two things ARE restated, once each, as specifications the plan must keep: the lines-per-workgroup
// decisions of the paired / split passes (spec_pair_T, spec_split_T) and the sizes the scratch requests had (spec_*_need).
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "mvs_cb_plan.h"

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
bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// ---- lines per workgroup ----
constexpr size_t kSpecBudget = 60 * 1024, kLdsLimit = 64 * 1024;
int spec_pair_T(int len, int radius, int axis) {
    const size_t span = (size_t)len + 2 * (size_t)radius;
    int T = (axis == 2) ? 8 : 16;
    while (T > 1 && span * (T + 1) * 8 > kSpecBudget) T >>= 1;
    if (span * (T + 1) * 8 > kSpecBudget || (axis != 2 && T < 4)) return 0;
    return T;
}
int spec_split_T(int len, int radius) {
    const size_t span = (size_t)len + 2 * (size_t)radius;
    int T = 32;
    while (T > 1 && span * (T + 1) * 4 > kSpecBudget) T >>= 1;
    return (span * (T + 1) * 4 > kSpecBudget || T < 8) ? 0 : T;
}
// one rule at one (len, radius, axis): its T, the range of T it may give, the bytes the launch asks for with a T, whether a T fits
void check_rule(const char* rule, int T, int tmin, int tmax, size_t lds_T, bool min_fits) {
    check("T_power_of_two_in_range", T == 0 || (pow2(T) && T >= tmin && T <= tmax));
    check("T_launch_within_64k", T == 0 || lds_T <= kLdsLimit);
    check("T_zero_iff_smallest_does_not_fit", (T == 0) == !min_fits);
    (void)rule;
}
void lines_per_workgroup() {
    group = "lines";
    const int radii[6] = {6, 8, 16, 20, 44, 127};
    for (int len = 1; len <= 9000; ++len)
        for (int r : radii)
            for (int axis = 1; axis <= 2; ++axis) {
                const bool x = axis == 2;
                snprintf(where, sizeof(where), "len %d radius %d axis %d", len, r, axis);
                int T = cb_pair_T(len, r, axis);
                check_rule("pair", T, x ? 1 : 4, x ? 8 : 16, cb_pair_lds(len, r, T, false), cb_pair_fits(len, r, x ? 1 : 4, false));
                check("pair_T_is_the_specified_decision", T == spec_pair_T(len, r, axis));
                T = cb_split_T(len, r);
                check_rule("split", T, 8, 32, cb_pair_lds(len, r, T, true), cb_pair_fits(len, r, 8, true));
                check("split_T_is_the_specified_decision", T == spec_split_T(len, r));
                T = cb_single_T(len, r, axis);
                check_rule("single", T, x ? 1 : 8, x ? 8 : 32, cb_single_lds(len, r, T), cb_single_lds(len, r, x ? 1 : 8) <= kCbLdsBudget);
                T = cb_fast_view_T(len, r, axis);
                check_rule("fast", T, x ? kCbXtLo : 32, x ? kCbXtHi : 64, cb_fast_lds(len, r, T, x), cb_fast_lds(len, r, x ? kCbXtLo : 32, x) <= kCbLdsBudget);
            }
}

// ---- boxes ----
// view i of a chunk `cs`: kind 0 touches the chunk's borders, 1 lies strictly inside, 2 is one voxel, 3 is empty (hi < lo on axis 1 + i % 2)
void make_reach(int kind, int i, int ndim, const int cs[3], int lo[3], int hi[3]) {
    for (int k = 0; k < 3; ++k) {
        if (k < 3 - ndim) { lo[k] = hi[k] = 0; continue; }
        if (kind == 0) { lo[k] = (i >> k) & 1 ? cs[k] / 2 : 0; hi[k] = (i >> k) & 1 ? cs[k] - 1 : cs[k] / 2 + 3; }
        else if (kind == 1) { lo[k] = 2 + i + k; hi[k] = cs[k] - 3 - k; }
        else if (kind == 2) { lo[k] = hi[k] = 5 + i; }
        else { lo[k] = 4; hi[k] = (k == 1 + i % 2) ? 3 - i : 9; }
    }
}
int make_boxes(int ndim, int nv, int shift, const int cs[3], CbPool* P, CbBox* boxes, int* row0, int* tab0, int* kinds) {
    *P = CbPool();
    for (int i = 0; i < nv; ++i) {
        int lo[3], hi[3];
        kinds[i] = (i + shift) % 4;
        make_reach(kinds[i], i, ndim, cs, lo, hi);
        cb_box_add(P, lo, hi, &boxes[i], &row0[i], &tab0[i]);
    }
    return nv;
}
void boxes() {
    group = "boxes";
    for (int ndim = 2; ndim <= 3; ++ndim)
        for (int nv = 1; nv <= 8; ++nv)
            for (int shift = 0; shift < 4; ++shift) {
                const int cs[3] = {ndim == 3 ? 40 : 1, 50, 60};
                snprintf(where, sizeof(where), "ndim %d views %d shift %d", ndim, nv, shift);
                CbPool P;
                CbBox B[8];
                int row0[8], tab0[8], kinds[8];
                make_boxes(ndim, nv, shift, cs, &P, B, row0, tab0, kinds);
                long long end = 0, max_box = 1, rows = 0, max_rows = 1, tab = 0;
                for (int i = 0; i < nv; ++i) {
                    const long long vol = (long long)B[i].n[0] * B[i].n[1] * B[i].n[2];
                    check("box_offset_multiple_of_64", B[i].off % 64 == 0);
                    check("box_ranges_disjoint_in_view_order", B[i].off >= end);
                    if (kinds[i] == 3) check("empty_box_is_zero_and_takes_no_pool", vol == 0 && B[i].n[0] + B[i].n[1] + B[i].n[2] == 0 && (i + 1 == nv ? P.floats : B[i + 1].off) == B[i].off);
                    else check("box_is_the_reach", vol > 0 && (kinds[i] != 2 || vol == 1));
                    check("row_and_table_running_sums", row0[i] == rows && tab0[i] == tab);
                    end = B[i].off + vol;
                    max_box = vol > max_box ? vol : max_box;
                    rows += (long long)B[i].n[0] * B[i].n[1];
                    max_rows = (long long)B[i].n[0] * B[i].n[1] > max_rows ? (long long)B[i].n[0] * B[i].n[1] : max_rows;
                    tab += 2ll * (B[i].n[0] + B[i].n[1] + B[i].n[2]);
                }
                check("pool_totals", P.used == end && P.floats >= end && P.floats % 64 == 0 && P.floats - end < 64 && P.max_box == max_box && P.rows == rows &&
                                         P.max_rows == max_rows && P.tab == tab);
            }
    // the 2^31 limit: `used` (the fast path's offsets) and `floats` (the rounded pool: small / mask_tables) flip exactly there
    struct { int n0, n2; bool used_fits, floats_fit; } big[3] = {{1, (int)((1ll << 31) - 64), true, true}, {1, (int)((1ll << 31) - 1), true, false}, {2, 1 << 30, false, false}};
    for (auto& b : big) {
        snprintf(where, sizeof(where), "box %d x 1 x %d", b.n0, b.n2);
        CbPool P;
        CbBox B;
        int r0, t0;
        const int lo[3] = {0, 0, 0}, hi[3] = {b.n0 - 1, 0, b.n2 - 1};
        cb_box_add(&P, lo, hi, &B, &r0, &t0);
        check("pool_verdict_flips_at_2_31", cb_pool_fits32(P.used) == b.used_fits && cb_pool_fits32(P.floats) == b.floats_fit && cb_small(8, P.floats) == b.floats_fit);
    }
}

// ---- scratch layouts ----
constexpr size_t kViewRec = 928;      // (any record size: the plan takes it as a number)
size_t spec_exact_need(const CbPool& P, int nv, bool paired, size_t n_taps, long long table_floats) {
    (void)n_taps;
    const size_t pool_b = (size_t)P.floats * 4, tmp_b = ((size_t)P.max_box * 4 + 255) / 256 * 256;
    return 3 * pool_b + (paired ? 5 : 6) * tmp_b + 64 * 1024 + (size_t)nv * (32 + kViewRec + 32 + 16) + 4096 + (size_t)table_floats * 4;
}
size_t spec_fast_need(const CbPool& P, int nv, size_t n_taps) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const long long g = (P.max_rows + 15) / 16;
    return 4 * up((size_t)P.floats * 4) + up((size_t)P.rows * 16) + up(n_taps * 8) + up(n_taps * 4) + up(nv * kViewRec) + up((size_t)nv * 64) + (size_t)nv * 512 * 16 +
           up((size_t)P.tab * 8) + up((size_t)nv * (size_t)(g < 1024 ? g : 1024) * 32) + 4096;
}
void check_sections(const size_t* off, const size_t* bytes, int n, size_t need, size_t spec) {
    for (int i = 0; i < n; ++i) {
        check("section_starts_on_256", off[i] % 256 == 0);
        check("sections_in_order_and_disjoint", off[i + 1] >= off[i] + bytes[i]);
    }
    check("request_covers_the_sections", need >= off[n]);
    check("request_not_below_the_specified_size", need >= spec);
}
void layouts() {
    group = "layouts";
    const int radii[3][2] = {{6, 8}, {20, 44}, {127, 127}};
    for (int ndim = 2; ndim <= 3; ++ndim)
        for (int nv = 1; nv <= 8; ++nv)
            for (auto& rr : radii)
                for (int variant = 0; variant < 4; ++variant) {
                    const int cs[3] = {ndim == 3 ? 40 : 1, 50, 60};
                    const bool paired = variant & 1;
                    const long long table_floats = (variant & 2) ? 64ll * (3 * nv + 1) : 0;
                    snprintf(where, sizeof(where), "ndim %d views %d radii %d %d variant %d", ndim, nv, rr[0], rr[1], variant);
                    CbPool P;
                    CbBox B[8];
                    int row0[8], tab0[8], kinds[8];
                    make_boxes(ndim, nv, variant, cs, &P, B, row0, tab0, kinds);
                    const size_t n_taps = 2 * (size_t)(rr[0] + rr[1]) + 2, unv = (size_t)nv, pool_b = (size_t)P.floats * 4;
                    // (the sections in the plan's order; the ones a path does not use are empty)
                    const CbLayout X = cb_layout(false, P, nv, paired, n_taps, kViewRec, table_floats);
                    const size_t xb[CS_N] = {pool_b, pool_b, pool_b, (paired ? 5 : 6) * (size_t)P.max_box * 4, 0, n_taps * 8, 0, unv * 32, unv * kViewRec, unv * 32, unv * 16, 0,
                                             (size_t)table_floats * 4, 0};
                    check_sections(X.off, xb, CS_N, X.need, spec_exact_need(P, nv, paired, n_taps, table_floats));
                    check("temporaries_hold_the_largest_box", X.tmp_b >= (size_t)P.max_box * 4 && X.tmp_b % 256 == 0);
                    const CbLayout F = cb_layout(true, P, nv, false, n_taps, kViewRec, 0);
                    const size_t fb[CS_N] = {pool_b, pool_b, pool_b, pool_b, (size_t)P.rows * 16, n_taps * 8, n_taps * 4, 0, unv * kViewRec, unv * 64, 0, unv * kCbMissCap * 16,
                                             (size_t)P.tab * 8, unv * cb_rows_grid(P.max_rows) * 32};
                    check_sections(F.off, fb, CS_N, F.need, spec_fast_need(P, nv, n_taps));
                    check("uploaded_block_is_contiguous", CS_UP0 == CS_TAPS64 && CS_UP1 == CS_MISS && CS_UP0 < CS_UP1);
                }
}

// ---- pass schedule of the exact paired path ----
void pair_schedule() {
    group = "pair_schedule";
    const int shapes[3][3] = {{50, 60, 70}, {300, 40, 48}, {20, 3000, 30}};      // (3000 + 2 * 44 rows: no split tile of 8 lines fits)
    for (int ndim = 2; ndim <= 3; ++ndim)
        for (auto& sh : shapes)
            for (int nosplit = 0; nosplit < 2; ++nosplit)
                for (int big = 0; big < 2; ++big) {
                    const int n[3] = {ndim == 3 ? sh[0] : 1, sh[1], sh[2]}, r1 = big ? 20 : 6, r2 = big ? 44 : 8;
                    snprintf(where, sizeof(where), "ndim %d box %d %d %d radii %d %d nosplit %d", ndim, n[0], n[1], n[2], r1, r2, nosplit);
                    CbPairPass p[6];
                    const int np = cb_pair_schedule(ndim, n, r1, r2, nosplit != 0, p);
                    check("pair_two_filters_of_ndim_passes", np == 2 * ndim);
                    for (int i = 0; i < np; ++i) {
                        const bool first = i % ndim == 0, last = i % ndim == ndim - 1;
                        const int radius = p[i].filt ? r2 : r1;
                        check("pair_filter_and_axis_order", p[i].filt == i / ndim && p[i].axis == 3 - ndim + i % ndim);
                        if (!first) check("pair_reads_what_the_previous_pass_wrote", p[i].src == SRC_AB && p[i].in_a == p[i - 1].out_a && p[i].in_b == p[i - 1].out_b && p[i].in_b >= 0);
                        else if (i == 0) check("pair_first_pass_reads_the_prepared_view", p[i].src == SRC_PREP && p[i].in_a == kCbBufView && p[i].in_b < 0);
                        else check("pair_second_filter_reads_the_squared_deviation", p[i].src == SRC_VMASK && p[i].in_a == kCbBufSq && p[i - 1].dst == DST_SQ && p[i - 1].out_a == kCbBufSq &&
                                                                                         p[i - 1].out_b < 0 && p[i].in_b < 0);
                        if (i == np - 1) check("pair_last_pass_writes_F", p[i].dst == DST_F && p[i].out_a == kCbBufF && p[i].out_b < 0);
                        if (!last) check("pair_middle_passes_hand_both_on", p[i].dst == DST_AB && p[i].out_a >= 0 && p[i].out_a < 4 && p[i].out_b >= 0 && p[i].out_b < 4 && p[i].out_a != p[i].out_b);
                        check("pair_writes_no_buffer_it_reads", p[i].out_a != p[i].in_a && p[i].out_a != p[i].in_b && (p[i].out_b < 0 || (p[i].out_b != p[i].in_a && p[i].out_b != p[i].in_b)));
                        const bool may_split = p[i].axis != 2 && p[i].dst == DST_AB && !nosplit;
                        check("pair_only_yz_passes_that_hand_both_on_are_split", p[i].split == (may_split && cb_split_T(n[p[i].axis], radius) > 0));
                        check("pair_launch_bytes", p[i].lds == cb_pair_lds(n[p[i].axis], radius, p[i].T, p[i].split) && (p[i].T == 0 || p[i].lds <= kLdsLimit));
                    }
                }
}

// ---- pass schedule of the fast path ----
void fast_schedule() {
    group = "fast_schedule";
    for (int ndim = 2; ndim <= 3; ++ndim)
        for (int nv = 1; nv <= 8; ++nv)
            for (int t = 0; t <= 22; t += 22) {
                const int cs[3] = {ndim == 3 ? 108 : 1, 120, 132}, r1 = 20, r2 = 44;
                const int64_t trim[3] = {ndim == 3 ? t : 0, t, t};
                snprintf(where, sizeof(where), "ndim %d views %d trim %d", ndim, nv, t);
                // tiles of a 2 x 2 x 2 grid that overlap in the middle; the LAST view is a sliver in the chunk's corner: wholly in the halo
                CbPool P;
                CbBox B[8];
                CbFastViews VS = CbFastViews();
                VS.nv = nv;
                for (int i = 0; i < nv; ++i) {
                    int lo[3], hi[3], row0, tab0;
                    for (int k = 0; k < 3; ++k) {
                        lo[k] = (i >> k) & 1 ? cs[k] / 2 - 15 : 0;
                        hi[k] = (i >> k) & 1 ? cs[k] - 1 : cs[k] / 2 + 15;
                        if (i == nv - 1 && nv > 1) { lo[k] = 0; hi[k] = cs[k] == 1 ? 0 : 9; }
                        if (cs[k] == 1) lo[k] = hi[k] = 0;
                    }
                    cb_box_add(&P, lo, hi, &B[i], &row0, &tab0);
                    VS.v[i] = CbFastView{(int)B[i].off, {B[i].n[0], B[i].n[1], B[i].n[2]}, {B[i].lo[0], B[i].lo[1], B[i].lo[2]}, row0, tab0, 0, 0, 0, 0, 0, 0};
                }
                int Tsel[3][2][8];
                check("fast_accepts_the_boxes", cb_fast_accepts_boxes(P, B, nv, ndim, r1, r2, Tsel) == kCbTaken);
                CbFastPass p[6];
                const int np = cb_fast_schedule(VS, ndim, cs, trim, r1, r2, Tsel, p);
                check("fast_two_filters_of_ndim_passes", np == 2 * ndim);
                for (int i = 0; i < np; ++i) {
                    const bool last_of_all = i == np - 1;
                    check("fast_pass_0_reads_I", (i == 0) == (p[i].src_buf == kCbBufI) && (i == 0) == (p[i].src == CBS_NAN0));
                    if (i) check("fast_reads_what_the_previous_pass_wrote", p[i].src_buf == p[i - 1].dst_buf);
                    check("fast_writes_no_pool_it_reads", p[i].dst_buf != p[i].src_buf && p[i].dst_buf != kCbBufI);
                    if (last_of_all) check("fast_last_pass_writes_F", p[i].dst_buf == kCbBufFast && p[i].dst == CBD_F);
                    check("fast_kinds", p[i].dst == (p[i].axis != 2 ? CBD_PLAIN : p[i].filt ? CBD_F : CBD_SQ) && p[i].radius == (p[i].filt ? r2 : r1));
                    int at = 0;
                    size_t lds = 0;
                    for (int v = 0; v < nv; ++v) {
                        const CbFastView& V = p[i].views.v[v];
                        bool reaches = (long long)V.n[0] * V.n[1] * V.n[2] > 0;
                        int w0[3], w1[3];      // the box inside the trimmed chunk, box-relative
                        for (int k = 0; k < 3; ++k) {
                            w0[k] = (V.lo[k] > trim[k] ? V.lo[k] : (int)trim[k]) - V.lo[k];
                            w1[k] = (V.lo[k] + V.n[k] < cs[k] - trim[k] ? V.lo[k] + V.n[k] : cs[k] - (int)trim[k]) - V.lo[k];
                            reaches = reaches && w1[k] > w0[k];
                        }
                        if (t && v == nv - 1 && nv > 1) check("fast_case_has_a_view_wholly_in_the_halo", !reaches);
                        if (!reaches) { check("fast_view_outside_the_trimmed_chunk_has_no_blocks", V.nzr == 0 && V.nyr == 0); continue; }
                        if (last_of_all) check("fast_last_pass_rows_are_the_trimmed_box", V.zr0 == w0[0] && V.nzr == w1[0] - w0[0] && V.yr0 == w0[1] && V.nyr == w1[1] - w0[1]);
                        else check("fast_other_passes_take_the_whole_box", V.zr0 == 0 && V.nzr == V.n[0] && V.yr0 == 0 && V.nyr == V.n[1]);
                        const long long lines = p[i].axis == 2 ? (long long)V.nzr * V.nyr : (long long)V.n[0] * V.n[1] * V.n[2] / V.n[p[i].axis];
                        check("fast_blocks_tile_the_launch_in_view_order", V.blk0 == at && pow2(V.T));
                        at += (int)((lines + V.T - 1) / V.T);
                        const size_t b = cb_fast_lds(V.n[p[i].axis], p[i].radius, V.T, p[i].axis == 2);
                        lds = b > lds ? b : lds;
                    }
                    check("fast_blocks_tile_the_launch_in_view_order", at == p[i].nb);
                    check("fast_launch_bytes_are_the_views_maximum", p[i].lds == lds && lds <= kLdsLimit);
                }
            }
}

// ---- which path a chunk takes, at the edges ----
void decisions() {
    group = "decisions";
    snprintf(where, sizeof(where), "edges");
    const int cs[3] = {200, 200, 200};
    const CbDecline by_views[4] = {kCbViewCount, kCbTaken, kCbTaken, kCbViewCount};
    const int counts[4] = {0, 1, 8, 9};
    for (int i = 0; i < 4; ++i) check("decline_view_count", cb_fast_accepts_chunk(counts[i], 3, cs, 20, 44, true) == by_views[i]);
    double m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    check("decline_matrix", cb_is_identity(m) && cb_fast_accepts_chunk(4, 3, cs, 20, 44, false) == kCbMatrix);
    for (int k = 0; k < 9; ++k) {
        m[k] += 1e-9;
        check("decline_matrix", !cb_is_identity(m));
        m[k] -= 1e-9;
    }
    for (int axis = 0; axis < 3; ++axis)
        for (int ndim = 2; ndim <= 3; ++ndim) {
            int c2[3] = {ndim == 3 ? 200 : 1, 200, 200};
            const bool counts_axis = axis >= 3 - ndim;
            c2[axis] = 43;
            check("decline_short_axis", cb_fast_accepts_chunk(4, ndim, c2, 20, 44, true) == (counts_axis ? kCbShortAxis : kCbTaken));
            check("decline_short_axis", cb_fast_accepts_chunk(4, ndim, c2, 44, 20, true) == (counts_axis ? kCbShortAxis : kCbTaken));
            c2[axis] = 44;
            check("decline_short_axis", cb_fast_accepts_chunk(4, ndim, c2, 20, 44, true) == kCbTaken);
        }
    check("decline_radius", cb_fast_accepts_chunk(4, 3, cs, 20, 127, true) == kCbTaken && cb_fast_accepts_chunk(4, 3, cs, 128, 20, true) == kCbRadius);
    // a view is a line along y that no tile of 32 lines holds; a pool of 2^31 floats
    CbPool P;
    CbBox B[2];
    int r0, t0, Tsel[3][2][8];
    const int lo[3] = {0, 0, 0}, hi_ok[3] = {9, 99, 9}, hi_long[3] = {9, 499, 9}, hi_big[3] = {1, 0, (1 << 30) - 1};
    cb_box_add(&P, lo, hi_ok, &B[0], &r0, &t0);
    check("decline_line", cb_fast_accepts_boxes(P, B, 1, 3, 20, 44, Tsel) == kCbTaken && Tsel[1][1][0] >= 32);
    cb_box_add(&P, lo, hi_long, &B[1], &r0, &t0);
    check("decline_line", cb_fast_view_T(500, 44, 1) == 0 && cb_fast_accepts_boxes(P, B, 2, 3, 20, 44, Tsel) == kCbLine);
    P = CbPool();
    cb_box_add(&P, lo, hi_big, &B[0], &r0, &t0);
    check("decline_pool", cb_fast_accepts_boxes(P, B, 1, 3, 20, 44, Tsel) == kCbPool);
    // the exact path's three
    P = CbPool();
    cb_box_add(&P, lo, hi_ok, &B[0], &r0, &t0);
    check("exact_decisions", cb_paired(B, 1, 3, 20, 44, false) && !cb_paired(B, 1, 3, 20, 44, true) && cb_small(8, P.floats) && !cb_small(9, P.floats) &&
                                 cb_mask_tables(true, 8, P.floats, true) && !cb_mask_tables(false, 8, P.floats, true) && !cb_mask_tables(true, 9, P.floats, true) &&
                                 !cb_mask_tables(true, 8, P.floats, false));
    const int hi_x[3] = {0, 9, 8199};      // x lines longer than any paired tile
    cb_box_add(&P, lo, hi_x, &B[1], &r0, &t0);
    check("exact_decisions", cb_pair_T(8200, 8, 2) == 0 && !cb_paired(B, 2, 2, 8, 16, false));
    // line geometry: every voxel of a box is position p of exactly one line
    group = "lines_geometry";
    const int n[3] = {3, 4, 5}, blo[3] = {7, 8, 9};
    for (int axis = 0; axis < 3; ++axis) {
        snprintf(where, sizeof(where), "axis %d", axis);
        const GaussLines L = cb_lines(n, blo, cs, axis);
        int seen[60] = {0};
        for (long long l = 0; l < L.n_lines; ++l)
            for (int p = 0; p < L.len; ++p) {
                const long long i = (l / L.inner) * L.outer_stride + (l % L.inner) + (long long)p * L.stride;
                if (i >= 0 && i < 60) ++seen[i];
            }
        bool once = L.n_lines * L.len == 60 && L.len == n[axis] && L.b0 == blo[axis] && L.full == cs[axis];
        for (int i = 0; i < 60; ++i) once = once && seen[i] == 1;
        check("lines_cover_the_box_once", once);
    }
}

}  // namespace

int main() {
    lines_per_workgroup();
    boxes();
    layouts();
    pair_schedule();
    fast_schedule();
    decisions();
    for (auto& g : n_checked) printf("C %s %lld\n", g.first.c_str(), g.second);
    for (auto& w : wrongs) printf("W %s %lld %s\n", w.first.c_str(), w.second.wrong, w.second.wrong ? w.second.first.c_str() : "-");
    printf("done\n");
    return 0;
}
