// Host-side run of csrc/mvs_phasecorr_plan.h (plain functions): the decisions, layouts and host arithmetic of mvs_phasecorr_multi.
// tests/test_phasecorr_plan_host.py builds this with hipcc (no GPU needed) and reads the lines:
//   P <checked> <kind> <lines_per_wg> <grid> <predictor> <capacity> <fuse_xp> <n_peak>     pass rule against the dispatch conditions and
//                                                       the predictor mvs_fft_reg_length that the driver used before the plan: wrong counts
//   R <route> <count>        S <stage-1 variant> <count>        F <forward variant> <count>        K <peak search> <count>
//   RW <checked> <wrong> ...   the plan against the conditions mvs_phasecorr_multi evaluated inline before the plan (`before`, below)
//   L <checked> <wrong> ...    layouts: regions apart, at the offsets of the formulas used before, totals equal, uploads of 16-byte units
//   Y <checked> <wrong>        the chunk partials of the merged stages 1 and 2 fit the stage-1 area, the chunks cover the rows
//   U / A / M / KV / TP / TS   host arithmetic (see main)
// Called with arguments it prints the plan of the cases they name instead (print_plans; tests/test_refine_cases_host.py).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mvs_phasecorr_plan.h"

namespace {
namespace pcp = mvs_phasecorr_plan;

// ---- the conditions as they stood in mvs_fft.hip, mvs_fft_slab.hip and mvs_reg.hip before the plan header ----------------------
namespace before {
size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
int grid_for(long long n) { return (int)std::min<long long>((n + 255) / 256, 256 * 8); }
// mvs_fft_reg_length: the driver's prediction of "this pass runs on the register kernels"
bool reg_length(int n) {
    if (n < 2) return false;
    if (mvs_dft_line_length(n)) return true;
    if ((n & (n - 1)) == 0) return n == 64 || n == 128 || n == 256;
    int M = 1;
    while (M < 2 * n - 1) M <<= 1;
    return M >= 64 && M <= 256;
}
// mvs_fft3_c2c: what a pass of length n over n_lines lines actually ran on
struct Dispatch { int kind; int lpw; long long grid; };      // kind: pcp::PassKind
Dispatch dispatch(int n, long long n_lines, bool axis2, bool fft_no_line) {
    const bool pow2n = (n & (n - 1)) == 0;
    if (n > 4096 || (!pow2n && n > 2048)) return {pcp::kFourStep, 0, 0};
    const bool bluestein = !pow2n;
    int M = 1;
    if (pow2n) M = n;
    else while (M < 2 * n - 1) M <<= 1;
    int lpb = std::max(1, std::min(8, 4096 / M));
    if (axis2) lpb = std::max(1, std::min(8, 2048 / M));
    const long long nblocks = (n_lines + lpb - 1) / lpb;
    const bool reg_pow2 = !bluestein && (n == 64 || n == 128 || n == 256);
    const bool reg_blue = bluestein && M <= 256 && M >= 64;
    const bool reg_line = mvs_dft_line_length(n) && !fft_no_line;
    if (reg_pow2 || reg_blue || reg_line) {
        const int lpw = reg_line ? 64 : ((reg_pow2 && n == 64) || (reg_blue && M == 64)) ? 32 : 16;
        return {reg_line ? pcp::kLine : reg_pow2 ? pcp::kRegPow2 : pcp::kRegBluestein, lpw, (n_lines + lpw - 1) / lpw};
    }
    return {pcp::kLds, lpb, nblocks};
}
long long pair_grid(const Dispatch& d, long long nz, long long ny) {
    const long long h = ny / 2 + 1, ncanon = h + ((nz - 1) / 2) * ny + ((nz % 2 == 0) ? h : 0);
    return (ncanon + d.lpw / 2 - 1) / (d.lpw / 2);
}
bool slab_long_length(int64_t n) { return n == 64 || n == 128 || n == 256; }
int slab_axis(const pcp::Switches& c, const int64_t shape[3]) {
    if (c.fft_no_slab || c.fft_no_line || c.reg_unfused) return -1;
    int as = -1;
    for (int k = 0; k < 3; ++k) {
        if (slab_long_length(shape[k])) continue;
        if (shape[k] > 64 || !mvs_dft_line_length((int)shape[k]) || as >= 0) return -1;
        as = k;
    }
    if (as >= 0 && !((c.fft_slab_axes >> as) & 1)) return -1;
    return as;
}
int slab_peaks(const int64_t shape[3], int short_axis) { return (int)(short_axis == 0 ? shape[1] : shape[0]); }

struct Decisions {
    int first_axis, last_axis, slab_axis, U, yx_chunks, rows_per_chunk, ga, gb;
    bool reads_crops, pack, packed, fuse_xp, fuse_yx, peak_ptrs;
    size_t mb_red, mb_z0, mb_res, mb_res_stride, mb_k, mb_kbytes, mb_total, up_kbytes, up_s1, up_s2, up_s3, up_bytes;
};
Decisions decide(int ndim, const int64_t shape[3], const int32_t* normalizations, int n_norm, int upsample_factor, const pcp::Switches& c) {
    Decisions d;
    const long long n = (long long)shape[0] * shape[1] * shape[2];
    const int nz = (int)shape[0], ny = (int)shape[1], nx = (int)shape[2];
    const int gb = grid_for(n);
    int first_axis = -1, last_axis = -1;
    for (int axis = 2; axis >= 0; --axis)
        if (shape[axis] > 1) { if (first_axis < 0) first_axis = axis; last_axis = axis; }
    const int slab_axis = (ndim == 3 && n_norm == 2 && (normalizations[0] != 0) != (normalizations[1] != 0) && !c.materialize_shifts &&
                           (int)ceilf((float)upsample_factor * 1.5f) <= 4)
                              ? before::slab_axis(c, shape) : -1;
    d.reads_crops = d.pack = false;
    if (slab_axis >= 0) {
    } else if (first_axis >= 0 && reg_length((int)shape[first_axis]) && !c.reg_unfused) {
        d.reads_crops = true;
    } else {
        d.pack = true;
    }
    const bool packed = n_norm == 2 && (normalizations[0] != 0) != (normalizations[1] != 0) && !c.materialize_shifts;
    const int up_U0 = (int)ceilf((float)upsample_factor * 1.5f);
    const size_t res_elems = upsample_factor > 1 ? (ndim == 3 ? (size_t)up_U0 * up_U0 * up_U0 : (size_t)up_U0 * up_U0) : 0;
    int ga = std::min(gb, 512);
    {
        int la = -1;
        for (int axis = 2; axis >= 0; --axis) if (shape[axis] > 1) la = axis;
        if (la >= 0 && reg_length((int)shape[la])) ga = std::max<long long>(ga, (n / shape[la] + 15) / 16);
        if (slab_axis >= 0) ga = std::max(ga, slab_peaks(shape, slab_axis));
    }
    const size_t mb_red = (size_t)ga * 32, mb_z0 = mb_red, mb_res = mb_red + 256, mb_res_stride = align_up(res_elems * sizeof(float2));
    const size_t mb_k = mb_res + mb_res_stride * (size_t)n_norm;
    const size_t mb_kbytes = upsample_factor > 1 ? align_up((size_t)up_U0 * (size_t)(nz + ny + nx) * sizeof(float2)) : 0;
    d.mb_total = mb_k + mb_kbytes * (size_t)n_norm;
    const bool fuse_xp = slab_axis >= 0 || (packed && first_axis == 2 && reg_length((int)nx) && up_U0 <= 4 && !c.reg_unfused);
    const bool fuse_yx = fuse_xp && ndim == 3 && up_U0 == 3 && nx <= 256 && ny >= 4;
    const int yx_chunks = fuse_yx ? std::max(1, std::min(pcp::kYxChunksMax, ((int)ny + pcp::kYxRows - 1) / pcp::kYxRows)) : 1;
    d.peak_ptrs = packed && slab_axis < 0 && last_axis >= 0 && reg_length((int)shape[last_axis]) && !c.reg_unfused;
    const int up_U = (int)ceilf((float)upsample_factor * 1.5f);
    const size_t up_kbytes = align_up((size_t)up_U * (size_t)(nz + ny + nx) * sizeof(float2));
    const size_t up_s1 = (size_t)nz * ny * up_U, up_s2 = (size_t)nz * up_U * up_U, up_s3 = (size_t)up_U * up_U * up_U;
    const size_t up_bytes = up_kbytes + (up_s1 + up_s2 + up_s3) * sizeof(float2) + 1024;
    d.first_axis = first_axis; d.last_axis = last_axis; d.slab_axis = slab_axis; d.U = up_U; d.yx_chunks = yx_chunks;
    d.rows_per_chunk = ((int)ny + yx_chunks - 1) / yx_chunks;
    d.ga = ga; d.gb = gb; d.packed = packed; d.fuse_xp = fuse_xp; d.fuse_yx = fuse_yx;
    d.mb_red = mb_red; d.mb_z0 = mb_z0; d.mb_res = mb_res; d.mb_res_stride = mb_res_stride; d.mb_k = mb_k; d.mb_kbytes = mb_kbytes;
    d.up_kbytes = up_kbytes; d.up_s1 = up_s1; d.up_s2 = up_s2; d.up_s3 = up_s3; d.up_bytes = up_bytes;
    return d;
}
}  // namespace before

struct Wrong {
    long long checked = 0, wrong = 0;
    char first[200] = "-";
    void note(const char* what, const int64_t shape[3], int n_norm, int uf) {
        if (!wrong) snprintf(first, sizeof first, "%s:%lldx%lldx%lld:n_norm=%d:uf=%d", what, (long long)shape[0], (long long)shape[1], (long long)shape[2], n_norm, uf);
        ++wrong;
    }
};

// ---- 1. prediction equals dispatch ---------------------------------------------------------------------------------------------
void check_passes() {
    long long checked = 0, w_kind = 0, w_lpw = 0, w_grid = 0, w_pred = 0, w_cap = 0, w_xp = 0, w_npeak = 0;
    const int32_t norms[2] = {1, 0};
    for (int n = 2; n <= 4200; ++n)
        for (int no_line = 0; no_line < 2; ++no_line)
            for (int no_pair = 0; no_pair < 2; ++no_pair)
                for (long long lines = 1; lines <= 70; ++lines) {
                    ++checked;
                    pcp::Switches sw;
                    sw.fft_no_line = no_line != 0; sw.fft_no_pair = no_pair != 0;
                    for (int axis2 = 0; axis2 < 2; ++axis2) {
                        const before::Dispatch d = before::dispatch(n, lines, axis2 != 0, sw.fft_no_line);
                        const pcp::Pass p = pcp::line_pass(n, lines, axis2 != 0, sw.fft_no_line);
                        const bool d_fused = d.kind == pcp::kLine || d.kind == pcp::kRegPow2 || d.kind == pcp::kRegBluestein;
                        if ((int)p.kind != d.kind || p.fused() != d_fused) ++w_kind;
                        if (p.lines_per_wg != d.lpw) ++w_lpw;
                        if (p.grid != d.grid) ++w_grid;
                        if (before::reg_length(n) != d_fused) ++w_pred;      // the predictor never saw fft_no_line
                    }
                    // the last inverse pass: along z of (n, lines, 1)
                    {
                        const int64_t shape[3] = {n, lines, 1};
                        const pcp::Plan pl = pcp::plan(3, shape, norms, 2, 2, sw);
                        const before::Dispatch d = before::dispatch(n, lines, false, sw.fft_no_line);
                        if (pl.last_pass_peaks) {
                            if (pl.ga < d.grid) ++w_cap;
                            if (pl.n_peak != d.grid) ++w_npeak;
                        }
                        if (pl.fuse_xp) ++w_xp;      // (the first pass does not run along x)
                    }
                    // the first inverse pass: along x of (1, lines, n); with one line it is the last pass as well
                    {
                        const int64_t shape[3] = {1, lines, n};
                        const pcp::Plan pl = pcp::plan(2, shape, norms, 2, 2, sw);
                        const before::Dispatch d = before::dispatch(n, lines, true, sw.fft_no_line);
                        const bool d_fused = d.kind != pcp::kLds && d.kind != pcp::kFourStep;
                        if (pl.fuse_xp && !d_fused) ++w_xp;
                        if (pl.last_pass_peaks && lines == 1) {
                            const bool pairs = pl.fuse_xp && d.kind == pcp::kRegPow2 && d.lpw % 2 == 0 && !sw.fft_no_pair;
                            const long long grid = pairs ? before::pair_grid(d, 1, lines) : d.grid;
                            if (pl.ga < grid) ++w_cap;
                            if (pl.n_peak != grid) ++w_npeak;
                        }
                    }
                }
    printf("P %lld %lld %lld %lld %lld %lld %lld %lld\n", checked, w_kind, w_lpw, w_grid, w_pred, w_cap, w_xp, w_npeak);
}

// ---- 2. route table, 3. layouts ------------------------------------------------------------------------------------------------
long long n_route[5], n_stage1[3], n_forward[3], n_peaks[3];
const char* route_name[5] = {"slab", "packed_fused_yx", "packed_fused_x", "packed_unfused", "per_norm"};
const char* stage1_name[3] = {"per_norm", "both", "stages_1_and_2_both"};
const char* forward_name[3] = {"inside_slab_passes", "reads_crops", "pack_kernel"};
const char* peaks_name[3] = {"slab_last_pass", "inverse_last_pass", "stand_alone_kernel"};
Wrong w_route, w_layout;

void check_case(int ndim, const int64_t shape[3], const int32_t* norms, int n_norm, int uf, const pcp::Switches& sw) {
    const before::Decisions b = before::decide(ndim, shape, norms, n_norm, uf, sw);
    const pcp::Plan p = pcp::plan(ndim, shape, norms, n_norm, uf, sw);
    ++w_route.checked;
    const pcp::Route want_route = b.slab_axis >= 0 ? pcp::kSlab : b.packed ? pcp::kPacked : pcp::kPerNorm;
    const bool same = p.route == want_route && p.first_axis == b.first_axis && p.last_axis == b.last_axis && p.short_axis == b.slab_axis && p.U == b.U &&
                      p.refine == (uf > 1) && p.forward_reads_crops == b.reads_crops && p.fuse_xp == b.fuse_xp && p.fuse_yx == b.fuse_yx &&
                      p.yx_chunks == b.yx_chunks && p.rows_per_chunk == b.rows_per_chunk && p.last_pass_peaks == b.peak_ptrs &&
                      p.ga == b.ga && p.gb == b.gb && (b.pack == (p.route != pcp::kSlab && !p.forward_reads_crops));
    if (!same) w_route.note("plan", shape, n_norm, uf);
    ++n_route[p.route == pcp::kSlab ? 0 : p.route == pcp::kPerNorm ? 4 : p.fuse_yx ? 1 : p.fuse_xp ? 2 : 3];
    if (p.refine) ++n_stage1[!p.fuse_xp ? 0 : p.fuse_yx ? 2 : 1];
    ++n_forward[p.route == pcp::kSlab ? 0 : p.forward_reads_crops ? 1 : 2];
    ++n_peaks[p.route == pcp::kSlab ? 0 : p.last_pass_peaks ? 1 : 2];

    ++w_layout.checked;
    const pcp::Mailbox m = pcp::mailbox(p, ndim, shape, n_norm);
    const pcp::Scratch s = pcp::scratch(p, shape, n_norm);
    const size_t ga = (size_t)p.ga, U = (size_t)p.U;
    // where the formulas used before put them, and the totals
    if (m.peak_val(0) != 0 || m.peak_idx(0) != ga * 8 || m.peak_val(1) != ga * 16 || m.peak_idx(1) != ga * 24 || m.z0 != b.mb_z0 || m.z0 != b.mb_red ||
        m.res != b.mb_res || m.res_stride != b.mb_res_stride || m.kvec != b.mb_k || m.kvec_stride != b.mb_kbytes || m.total != b.mb_total)
        w_layout.note("mailbox_offsets", shape, n_norm, uf);
    if (s.kvec_stride != b.up_kbytes || s.s1 != b.up_s1 || s.s2 != b.up_s2 || s.s3 != b.up_s3 || s.kvec_stride + s.stage_stride != b.up_bytes ||
        s.total != b.up_bytes * (size_t)n_norm)
        w_layout.note("scratch_offsets", shape, n_norm, uf);
    for (int i = 0; i < n_norm; ++i)
        if (s.kvec_of(i) != (size_t)i * b.up_kbytes || s.stage_of(i) != (size_t)n_norm * b.up_kbytes + (size_t)i * (b.up_bytes - b.up_kbytes))
            w_layout.note("scratch_offsets", shape, n_norm, uf);
    // regions apart: [peaks | z0 | results | kernel vectors], the four peak arrays, n_peak entries in ga
    const size_t res_bytes = p.refine ? (ndim == 3 ? U * U * U : U * U) * sizeof(float2) : 0;
    size_t kvec_bytes = 0;
    for (int k = ndim == 3 ? 0 : 1; k < 3; ++k) kvec_bytes += U * (size_t)shape[k] * sizeof(float2);
    if (!p.refine) kvec_bytes = 0;
    const bool apart = p.n_peak >= 1 && p.n_peak <= p.ga && m.peak_val(0) + ga * 4 <= m.peak_idx(0) && m.peak_idx(0) + ga * 8 <= m.peak_val(1) &&
                       m.peak_val(1) + ga * 4 <= m.peak_idx(1) && m.peak_idx(1) + ga * 8 <= m.z0 && m.z0 + sizeof(float2) <= m.res &&
                       res_bytes <= m.res_stride && m.res_of(n_norm - 1) + m.res_stride <= m.kvec && kvec_bytes <= m.kvec_stride &&
                       m.kvec_of(n_norm - 1) + m.kvec_stride <= m.total && m.res % 8 == 0 && m.kvec % 16 == 0;
    if (!apart) w_layout.note("mailbox_overlap", shape, n_norm, uf);
    const bool sapart = kvec_bytes <= s.kvec_stride && s.kvec_of(n_norm - 1) + s.kvec_stride <= s.stages && (s.s1 + s.s2 + s.s3) * sizeof(float2) <= s.stage_stride &&
                        s.stage_of(n_norm - 1) + s.stage_stride <= s.total && s.stages % 16 == 0 && s.stage_stride % 8 == 0;
    if (!sapart) w_layout.note("scratch_overlap", shape, n_norm, uf);
    // the kernel-vector stride is one number, and every upload is made of 16-byte units that stay inside the vectors' area
    if (p.refine) {
        const size_t one = pcp::upload_bytes(kvec_bytes), all = pcp::upload_bytes((size_t)(n_norm - 1) * s.kvec_stride + kvec_bytes);
        if (m.kvec_stride != s.kvec_stride || m.kvec_stride != pcp::kvec_stride(shape, p.U) || one % 16 || all % 16 || one > s.kvec_stride || all > s.stages ||
            m.kvec + all > m.total)
            w_layout.note("upload", shape, n_norm, uf);
    }
    if (p.fuse_yx && ((size_t)shape[0] * p.yx_chunks * U * U > s.s1 || (long long)p.rows_per_chunk * p.yx_chunks < shape[1]))
        w_layout.note("yx_partials", shape, n_norm, uf);
}

void check_routes_and_layouts() {
    const int64_t axes[] = {1, 2, 3, 4, 16, 18, 20, 51, 64, 65, 128, 130, 256, 300};
    const int na = (int)(sizeof axes / sizeof axes[0]);
    const int32_t norm_sets[6][2] = {{1, 0}, {0, 0}, {1, 0}, {0, 1}, {1, 1}, {0, 0}};      // two of n_norm = 1, four of n_norm = 2
    const int ufs[] = {1, 2, 3, 10};
    const int slab_masks[] = {4, 7, 2};
    for (int dims = 2; dims <= 3; ++dims)
        for (int iz = 0; iz < (dims == 3 ? na : 1); ++iz)
            for (int iy = 0; iy < na; ++iy)
                for (int ix = 0; ix < na; ++ix) {
                    const int64_t shape[3] = {dims == 3 ? axes[iz] : 1, axes[iy], axes[ix]};
                    for (int ns = 0; ns < 6; ++ns)
                        for (int uf : ufs)
                            for (int bits = 0; bits < 32; ++bits)
                                for (int mask : slab_masks) {
                                    pcp::Switches sw;
                                    sw.reg_unfused = bits & 1; sw.materialize_shifts = bits & 2; sw.fft_no_slab = bits & 4; sw.fft_no_line = bits & 8;
                                    sw.fft_no_pair = bits & 16; sw.fft_slab_axes = mask;
                                    check_case(dims, shape, norm_sets[ns], ns < 2 ? 1 : 2, uf, sw);
                                }
                }
    for (int r = 0; r < 5; ++r) printf("R %s %lld\n", route_name[r], n_route[r]);
    for (int r = 0; r < 3; ++r) printf("S %s %lld\n", stage1_name[r], n_stage1[r]);
    for (int r = 0; r < 3; ++r) printf("F %s %lld\n", forward_name[r], n_forward[r]);
    for (int r = 0; r < 3; ++r) printf("K %s %lld\n", peaks_name[r], n_peaks[r]);
    printf("RW %lld %lld %s\n", w_route.checked, w_route.wrong, w_route.first);
    printf("L %lld %lld %s\n", w_layout.checked, w_layout.wrong, w_layout.first);
    // merged stages 1 and 2: nz * yx_chunks * U * U <= nz * ny * U for every ny the route accepts
    long long checked = 0, wrong = 0;
    const int32_t norms[2] = {1, 0};
    for (int64_t ny = 4; ny <= 4096; ++ny)
        for (int64_t nz : {2, 7, 51})
            for (int64_t nx : {64, 51, 256}) {
                const int64_t shape[3] = {nz, ny, nx};
                const pcp::Plan p = pcp::plan(3, shape, norms, 2, 2, pcp::Switches());
                const pcp::Scratch s = pcp::scratch(p, shape, 2);
                ++checked;
                if (!p.fuse_yx || !p.fuse_xp || p.U != 3) { ++wrong; continue; }
                if ((size_t)nz * p.yx_chunks * p.U * p.U > (size_t)nz * ny * p.U || (size_t)nz * ny * p.U != s.s1) ++wrong;
                if ((long long)p.rows_per_chunk * p.yx_chunks < ny || p.yx_chunks > pcp::kYxChunksMax || p.yx_chunks < 1) ++wrong;
            }
    printf("Y %lld %lld\n", checked, wrong);
}

// ---- 4. host arithmetic ----------------------------------------------------------------------------------------------------------
unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

void print_arithmetic() {
    // U <flat> <nz> <ny> <nx> <pz> <py> <px>
    const int64_t shapes[][3] = {{5, 7, 9}, {1, 20, 64}, {4, 6, 64}, {51, 256, 256}};
    for (const auto& sh : shapes)
        for (long long flat : {0ll, 1ll, (long long)sh[2], (long long)(sh[1] * sh[2]), (long long)(sh[0] * sh[1] * sh[2] - 1), (long long)(sh[0] * sh[1] * sh[2] / 2 + 3)}) {
            if (flat >= sh[0] * sh[1] * sh[2]) continue;
            long long peak[3];
            pcp::unravel(flat, sh, peak);
            printf("U %lld %lld %lld %lld %lld %lld %lld\n", flat, (long long)sh[0], (long long)sh[1], (long long)sh[2], peak[0], peak[1], peak[2]);
        }
    // A <n> <uf> <peak> <U> <shift> <rounded shift> <offset>       float32 bit patterns, one axis (the three axes run the same code)
    // M <n> <uf> <peak> <m> <shift after the sub-pixel maximum m>   and, with "Z", the same on an axis of length 1 (zeroed)
    // KV <n> <uf> <peak> <U> then U * n pairs of bit patterns
    for (int n : {8, 9, 20, 51, 64, 301})
        for (int uf : {1, 2, 3, 10, 100}) {
            const int mid = n / 2;
            for (long long pk : {0ll, (long long)mid, (long long)mid - 1, (long long)mid + 1, (long long)n - 1}) {
                const int64_t shape[3] = {n, n, n};
                const long long peak[3] = {pk, pk, pk};
                float shift[3], offs[3];
                pcp::peak_to_shift(peak, shape, shift);
                const float s0 = shift[2];
                const int U = pcp::refine_samples(uf);
                pcp::round_to_grid(shift, uf, U, offs);
                printf("A %d %d %lld %d %u %u %u\n", n, uf, pk, U, bits(s0), bits(shift[2]), bits(offs[2]));
                for (int m = 0; m < U; m += (U > 8 ? U / 7 : 1)) {
                    float f3[3] = {shift[0], shift[1], shift[2]}, f2[3] = {shift[0], shift[1], shift[2]};
                    pcp::add_subpixel(f3, (size_t)m * U * U + (size_t)m * U + m, U, 3, uf);
                    pcp::add_subpixel(f2, (size_t)m * U + m, U, 2, uf);
                    const int64_t unit[3] = {1, n, n};
                    pcp::zero_unit_axes(f2, unit);
                    printf("M %d %d %lld %d %u %u %u %u %u %u\n", n, uf, pk, m, bits(f3[0]), bits(f3[1]), bits(f3[2]), bits(f2[0]), bits(f2[1]), bits(f2[2]));
                }
                if (n <= 51) {
                    std::vector<float2> k((size_t)U * n);
                    const size_t nk = pcp::fill_kernel(k.data(), n, U, offs[2], uf);
                    printf("KV %d %d %lld %d", n, uf, pk, U);
                    for (size_t i = 0; i < nk; ++i) printf(" %u %u", bits(k[i].x), bits(k[i].y));
                    printf("\n");
                }
            }
        }
    // TP <n> <values...> <indices...> <best> <index>: arg max over partials with planted ties (the lowest INDEX wins, wherever it stands)
    {
        const float v[][6] = {{1, 5, 5, 2, 5, 0}, {7, 7, 7, 7, 7, 7}, {0, 1, 2, 3, 4, 9}, {9, 1, 2, 3, 4, 9}, {-1, -1, -1, -1, -1, -1}};
        const long long ix[][6] = {{10, 40, 30, 5, 35, 1}, {6, 5, 4, 3, 2, 1}, {1, 2, 3, 4, 5, 6}, {60, 2, 3, 4, 5, 6}, {3, 2, 1, 4, 5, 6}};
        for (int t = 0; t < 5; ++t) {
            float best;
            long long bi;
            pcp::argmax_partials(v[t], ix[t], 6, &best, &bi);
            printf("TP 6");
            for (int i = 0; i < 6; ++i) printf(" %g", v[t][i]);
            for (int i = 0; i < 6; ++i) printf(" %lld", ix[t][i]);
            printf(" %g %lld\n", best, bi);
        }
    }
    // TS <n> <re im ...> <index>: sub-pixel arg max of |.| with ties (3 + 4i, 5, 5i, 4 - 3i all have modulus 5 exactly)
    {
        const float2 r[][5] = {{{0, 0}, {3, 4}, {5, 0}, {0, 5}, {4, -3}}, {{5, 0}, {3, 4}, {1, 1}, {0, -5}, {0, 0}}, {{1, 0}, {0, 2}, {-3, 0}, {0, -3}, {3, 0}},
                               {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}}};
        for (int t = 0; t < 4; ++t) {
            printf("TS 5");
            for (int i = 0; i < 5; ++i) printf(" %g %g", r[t][i].x, r[t][i].y);
            printf(" %zu\n", pcp::subpixel_argmax(r[t], 5));
        }
    }
    // X <z0.re> <z0.im> <n> <scale_phase> <scale_plain>: the channel scales the host takes from the DC term
    for (float re : {0.f, 3.5f, 1000.f, 1e30f})
        for (float im : {2.f, 4096.f, 1e30f})
            for (long long n : {1ll, 1000ll, 3342336ll}) {
                float sp, sl;
                mvs_xpower_scales(make_float2(re, im), n, &sp, &sl);
                printf("X %u %u %lld %u %u\n", bits(re), bits(im), n, bits(sp), bits(sl));
            }
}

// ---- 5. the plan of given cases (tests/test_refine_cases_host.py) ------------------------------------------------------------------
// every argument "ndim,nz,ny,nx,n_norm,norm0,norm1,upsample,switch bits" (bits as in check_routes_and_layouts: 1 reg_unfused,
// 2 materialize_shifts, 4 fft_no_slab, 8 fft_no_line, 16 fft_no_pair) gives one line
//   PL <argument> <route> <fuse_xp> <fuse_yx> <yx_chunks> <rows_per_chunk> <forward_reads_crops> <last_pass_peaks> <n_peak>
int print_plans(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        long long v[9];
        if (sscanf(argv[i], "%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) != 9) return 2;
        const int64_t shape[3] = {v[1], v[2], v[3]};
        const int32_t norms[2] = {(int32_t)v[5], (int32_t)v[6]};
        pcp::Switches sw;
        sw.reg_unfused = v[8] & 1; sw.materialize_shifts = v[8] & 2; sw.fft_no_slab = v[8] & 4; sw.fft_no_line = v[8] & 8; sw.fft_no_pair = v[8] & 16;
        const pcp::Plan p = pcp::plan((int)v[0], shape, norms, (int)v[4], (int)v[7], sw);
        printf("PL %s %s %d %d %d %d %d %d %d\n", argv[i], p.route == pcp::kSlab ? "slab" : p.route == pcp::kPacked ? "packed" : "per_norm", (int)p.fuse_xp,
               (int)p.fuse_yx, p.yx_chunks, p.rows_per_chunk, (int)p.forward_reads_crops, (int)p.last_pass_peaks, p.n_peak);
    }
    printf("done\n");
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) return print_plans(argc, argv);
    check_passes();
    check_routes_and_layouts();
    print_arithmetic();
    printf("done\n");
    return 0;
}
