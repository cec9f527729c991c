// mvs_cb_plan.h -- the one definition of the host plan of a content-based chunk (mvs_gauss.hip, mvs_gauss_fast.inc): the structs the
// kernels share with the drivers, the views' boxes and their pool, the lines of a box, the lines a workgroup takes (each rule next to the
// LDS bytes of the launch it sizes), which path a chunk takes, the scratch layout and the pass schedules of both paths.  Integers and
// small structs only: no context, no HIP call; tests/native/cb_plan_host_test.cpp compiles it for the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

namespace {      // (anonymous, as the kernels of mvs_gauss.hip that take these structs are: the header leaves their symbols as they were)

constexpr int kGaussK = 8;            // outputs per thread of the LDS line filters
constexpr int kCbNearCap = 256;       // listed voxels one workgroup of a last pass handles in its compact form
constexpr int kCbMissCap = 512;       // listed voxels per view; more -> flag, exact path
constexpr int kCbMaxRadius = 127;     // radii of the fast path (sigma <= 31): the weights of a last pass sit in static LDS
constexpr int kCbRun = 4;             // consecutive voxels of a row per thread of the fast path's normalise / fuse kernels
constexpr size_t kCbLdsBudget = 60 * 1024;      // dynamic LDS a line launch may plan with, of the 64 KiB a workgroup can have
constexpr int kCbXtLo = 8, kCbXtHi = 32;        // lines per workgroup of the fast path's x passes (measured range)
constexpr long long kCbPoolLimit = 1ll << 31;   // floats of a pool that 32-bit indices reach

struct CbBox { int lo[3], n[3]; long long off; };      // box of a view inside the chunk; off: its first float in the I / BW / F pools
static_assert(sizeof(CbBox) == 32, "CbBox layout");
struct CbBox32 { int lo[3], n[3], off; };
struct CbBoxes8 { CbBox32 b[8]; };
// zr0 / nzr / yr0 / nyr: the rows (z, y) of the box a pass along x works on (the last pass of the second filter: only the rows
// inside the trimmed chunk are ever read); nzr == 0: the view takes no part in the launch
struct CbFastView { int off; int n[3]; int lo[3]; int row0; int tab0; int T; int blk0; int zr0, nzr, yr0, nyr; };
struct CbFastViews { CbFastView v[8]; int nv; };
struct GaussLines { long long n_lines; int len; long long stride; long long inner; long long outer_stride; int T; int b0, full; };

__host__ __device__ inline size_t cb_align(size_t v) { return (v + 255) / 256 * 256; }

// scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius), radius = int(truncate * sigma + 0.5)
inline void gaussian_taps(double sigma, int* radius_out, std::vector<double>* w) {
    const int radius = (int)(4.0 * sigma + 0.5);
    w->resize(2 * radius + 1);
    const double sigma2 = sigma * sigma;
    double sum = 0.0;
    for (int k = -radius; k <= radius; ++k) {
        const double v = exp(-0.5 / sigma2 * (double)k * (double)k);
        (*w)[k + radius] = v;
        sum += v;
    }
    for (auto& v : *w) v /= sum;
    *radius_out = radius;
}

// ---- boxes: view after view from its reach (lo, hi) inside the chunk to its box and the pools' running sums.  An empty reach
// (hi < lo on an axis) is the all-zero box and takes no pool; a box starts on a multiple of 64 floats. ----
// floats: pool size (rounded); used: end of the last box (the fast path's 32-bit offsets need used < 2^31); largest box; (z, y) rows, table doubles
struct CbPool { long long floats = 0, used = 0, max_box = 1, rows = 0, max_rows = 1, tab = 0; };
inline void cb_box_add(CbPool* P, const int lo[3], const int hi[3], CbBox* B, int* row0, int* tab0) {
    long long bv = 1;
    for (int k = 0; k < 3; ++k) {
        B->lo[k] = lo[k];
        B->n[k] = hi[k] - lo[k] + 1 > 0 ? hi[k] - lo[k] + 1 : 0;
        bv *= B->n[k];
    }
    if (bv == 0) B->n[0] = B->n[1] = B->n[2] = 0;
    const long long rows = (long long)B->n[0] * B->n[1];
    B->off = P->floats; *row0 = (int)P->rows; *tab0 = (int)P->tab;
    P->used = P->floats + bv;
    P->floats += (bv + 63) / 64 * 64;
    P->rows += rows;
    P->tab += 2ll * (B->n[0] + B->n[1] + B->n[2]);
    P->max_box = bv > P->max_box ? bv : P->max_box;
    P->max_rows = rows > P->max_rows ? rows : P->max_rows;
}
inline bool cb_pool_fits32(long long floats) { return floats < kCbPoolLimit; }
inline void cb_boxes8(const CbBox* boxes, int n_views, CbBoxes8* bx8) {      // (pool below 2^31 floats, <= 8 views)
    *bx8 = CbBoxes8{};
    for (int i = 0; i < n_views; ++i) {
        for (int k = 0; k < 3; ++k) { bx8->b[i].lo[k] = boxes[i].lo[k]; bx8->b[i].n[k] = boxes[i].n[k]; }
        bx8->b[i].off = (int)boxes[i].off;
    }
}

// ---- the lines of a box along `axis` (scipy filters axis 0, 1, 2 in turn): `full` = the chunk's extents (reflection), T is the rule's ----
inline GaussLines cb_lines(const int n[3], const int lo[3], const int full[3], int axis) {
    GaussLines L;
    const long long nz = n[0], ny = n[1], nx = n[2];
    if (axis == 2) { L.len = n[2]; L.stride = 1; L.n_lines = nz * ny; L.inner = 1; L.outer_stride = nx; }
    else if (axis == 1) { L.len = n[1]; L.stride = nx; L.n_lines = nz * nx; L.inner = nx; L.outer_stride = ny * nx; }
    else { L.len = n[0]; L.stride = ny * nx; L.n_lines = ny * nx; L.inner = ny * nx; L.outer_stride = 0; }
    L.T = 0;
    L.b0 = lo[axis];
    L.full = full[axis];
    return L;
}

// ---- lines per workgroup (T, a power of two; 0: no admissible T fits), each rule under the LDS bytes of the launch it sizes ----
// gauss1d_pair_kernel: len + 2 radius staged rows + kGaussK spare ones, pitch T + 1, two quantities (split: one) of 4 bytes
inline size_t cb_pair_lds(int len, int radius, int T, bool split) { return (size_t)(len + 2 * radius + kGaussK) * (T + 1) * (split ? 4 : 8); }
// The rules budget the STAGED rows (the decisions of round 4, measured with them): the launch minus its spare rows (= the launch of an
// empty line); those come out of the 4 KiB between the budget and the 64 KiB a workgroup can have
inline bool cb_pair_fits(int len, int radius, int T, bool split) { return cb_pair_lds(len, radius, T, split) - cb_pair_lds(-2 * radius, radius, T, split) <= kCbLdsBudget; }
static_assert(kCbLdsBudget + kGaussK * (32 + 1) * 8 <= 64 * 1024, "spare rows of the largest T fit above the budget");
inline int cb_pair_T(int len, int radius, int axis) {      // paired pass: 8 along x, 16 along y / z (at least 4)
    int T = (axis == 2) ? 8 : 16;
    while (T > 1 && !cb_pair_fits(len, radius, T, false)) T >>= 1;
    return (!cb_pair_fits(len, radius, T, false) || (axis != 2 && T < 4)) ? 0 : T;
}
inline int cb_split_T(int len, int radius) {      // split pass, y / z only (8 / 16 / 32 measured: 30.9 / 28.5 / 28.1 ms per probe call)
    int T = 32;
    while (T > 1 && !cb_pair_fits(len, radius, T, true)) T >>= 1;
    return (!cb_pair_fits(len, radius, T, true) || T < 8) ? 0 : T;
}
// gauss1d_lds_kernel (separate passes): len + 2 radius rows of one quantity; 0: the tap-by-tap kernel
inline size_t cb_single_lds(int len, int radius, int T) { return (size_t)(len + 2 * radius) * (T + 1) * 4; }
inline int cb_single_T(int len, int radius, int axis) {
    int T = (axis == 2) ? 8 : 32;
    while (T > 1 && cb_single_lds(len, radius, T) > kCbLdsBudget) T >>= 1;
    return (cb_single_lds(len, radius, T) <= kCbLdsBudget && (axis == 2 || T >= 8)) ? T : 0;
}

// LDS layouts of cb_line_kernel.  Lines along z / y (PF = false): [position][line], pitch T + 1 -- a wavefront's lanes are adjacent
// LINES (adjacent x in memory), staging, filter reads and stores are all conflict-free / coalesced.  Lines along x (PF = true): a
// wavefront's lanes must be adjacent 8-sample BLOCKS of one line, or every 32-byte piece of the pass's global reads and writes lands
// in another row; their window samples are 8 positions apart, so a line is stored de-interleaved by 8 -- position p at
// (p & 7) * S8 + (p >> 3), S8 = 4 mod 8 -- which makes both the staging (lanes = consecutive positions) and the filter reads (lanes =
// consecutive blocks) conflict-free.
__host__ __device__ __forceinline__ int cb_pf_S8(int rows) { int s = (rows + 7) / 8 + 1; s += (12 - (s & 7)) & 7; return s; }      // rows = len + 2 radius + K
__host__ __device__ __forceinline__ int cb_pf_LP(int rows) { return 8 * cb_pf_S8(rows) + 11; }
inline size_t cb_fast_lds(int len, int radius, int T, bool pf) {      // (x passes: + the [kCbNearCap][T] weights of the listed voxels)
    const int rows = len + 2 * radius + kGaussK;
    return pf ? (size_t)T * cb_pf_LP(rows) * 4 + (size_t)kCbNearCap * T * 4 : (size_t)rows * (T + 1) * 4;
}
// cb_line_kernel: the power of two (from `lo` to `hi`) that leaves the fewest idle thread slots in the filter loop (T * ceil(len / K)
// items on 256 threads) and fits the LDS budget
inline int cb_fast_T(int len, int radius, int lo, int hi, bool pf) {
    const int nblk = (len + kGaussK - 1) / kGaussK;
    int best = 0;
    double best_eff = -1.0;
    for (int T = lo; T <= hi; T <<= 1) {
        if (cb_fast_lds(len, radius, T, pf) > kCbLdsBudget) break;
        const int items = T * nblk;
        const double eff = (double)items / (double)(((items + 255) / 256) * 256);
        // ties: lines along z / y take the larger T (longer contiguous pieces per row), lines along x the smaller one (less LDS per
        // workgroup, more of them per CU: 16.4 -> 13.5 ms per probe call)
        if (pf ? eff > best_eff + 1e-9 : eff >= best_eff - 1e-9) { best_eff = eff; best = T; }
    }
    return best;
}
inline int cb_fast_view_T(int len, int radius, int axis) {      // (a view without voxels takes no part: any T)
    return len > 0 ? cb_fast_T(len, radius, axis == 2 ? kCbXtLo : 32, axis == 2 ? kCbXtHi : 64, axis == 2) : 8;
}

// ---- which path a chunk takes ----
// why the fast path declines a chunk, in the order the checks are made (further images of a voxel under the reflection would be in
// reach on a chunk axis shorter than a radius; kCbPool: see CbPool::used)
enum CbDecline { kCbTaken = 0, kCbViewCount, kCbShortAxis, kCbMatrix, kCbRadius, kCbPool, kCbLine };
inline bool cb_is_identity(const double m[9]) {
    for (int k = 0; k < 9; ++k) if (m[k] != ((k % 4 == 0) ? 1.0 : 0.0)) return false;
    return true;
}
inline CbDecline cb_fast_accepts_chunk(int n_views, int ndim, const int cs[3], int r1, int r2, bool identity) {      // what needs no boxes
    const int rmax = r1 > r2 ? r1 : r2;
    if (n_views > 8 || n_views < 1) return kCbViewCount;
    for (int axis = 3 - ndim; axis < 3; ++axis)
        if (cs[axis] < rmax) return kCbShortAxis;
    if (!identity) return kCbMatrix;
    return rmax > kCbMaxRadius ? kCbRadius : kCbTaken;
}
// ... and what needs them: Tsel[axis][filter][view] = lines per workgroup of every line launch
inline CbDecline cb_fast_accepts_boxes(const CbPool& P, const CbBox* boxes, int n_views, int ndim, int r1, int r2, int Tsel[3][2][8]) {
    if (!cb_pool_fits32(P.used)) return kCbPool;
    for (int axis = 3 - ndim; axis < 3; ++axis)
        for (int f = 0; f < 2; ++f)
            for (int i = 0; i < n_views; ++i)
                if (!(Tsel[axis][f][i] = cb_fast_view_T(boxes[i].n[axis], f ? r2 : r1, axis))) return kCbLine;
    return kCbTaken;
}
// exact path.  small: boxes as a kernel argument, 32-bit indices kept in registers; paired: every line set of every view can be
// staged twice in LDS (else the separate value / mask passes); mask_tables: the masks that are boxes come from tables
inline bool cb_small(int n_views, long long pool) { return n_views <= 8 && cb_pool_fits32(pool); }
inline bool cb_paired(const CbBox* boxes, int n_views, int ndim, int r1, int r2, bool unpaired) {
    for (int i = 0; i < n_views && !unpaired; ++i)
        for (int axis = 3 - ndim; axis < 3; ++axis)
            if (boxes[i].n[axis] > 0 && (!cb_pair_T(boxes[i].n[axis], r1, axis) || !cb_pair_T(boxes[i].n[axis], r2, axis))) return false;
    return !unpaired;
}
inline bool cb_mask_tables(bool paired, int n_views, long long pool, bool closed_form) { return paired && cb_small(n_views, pool) && closed_form; }

// ---- scratch layout (slot 6) of both paths: the sections in order, each on a multiple of 256 bytes; a section a path does not use is
// empty.  The request is the sections' end plus the path's headroom (the slack terms the requests always carried).
//   pools I, BW, F; temporaries (exact: 5 paired / 6 separate ones of the largest box, fast: the pool T0); fast: row records;
//   [CS_UP0, CS_UP1) ONE uploaded block: taps float64, fast: taps float32, exact: boxes, view records, empty mask records (exact 32,
//   fast 64 bytes), exact: table offsets;
//   fast: lists; mask tables (exact: B(z, y) of every view and filter, floats; fast: doubles); fast: partial records of the row scan
enum { CS_I, CS_BW, CS_F, CS_TMP, CS_ROWS, CS_TAPS64, CS_TAPS32, CS_BOXES, CS_VIEWS, CS_RECS, CS_TOFF, CS_MISS, CS_TABLES, CS_PART, CS_N,
       CS_UP0 = CS_TAPS64, CS_UP1 = CS_MISS };
constexpr size_t kCbExactHeadroom = 64 * 1024 + 4096, kCbFastHeadroom = 4096;
inline unsigned cb_rows_grid(long long max_rows) { const long long g = (max_rows + 15) / 16; return (unsigned)(g < 1024 ? g : 1024); }      // a workgroup: 4 wavefronts x 4 rows per sweep
struct CbLayout { size_t off[CS_N + 1], tmp_b, need; };
inline CbLayout cb_layout(bool fast, const CbPool& P, int n_views, bool paired, size_t n_taps, size_t view_rec_bytes, long long table_floats) {
    CbLayout Y;
    const size_t nv = (size_t)n_views, pool_b = (size_t)P.floats * 4, f = fast ? 1 : 0, x = 1 - f;
    Y.tmp_b = cb_align((size_t)P.max_box * 4);
    const size_t bytes[CS_N] = {pool_b, pool_b, pool_b, fast ? pool_b : (paired ? 5 : 6) * Y.tmp_b, f * P.rows * 16, n_taps * 8, f * n_taps * 4, x * nv * sizeof(CbBox),
                                nv * view_rec_bytes, nv * (fast ? 64 : 32), x * nv * 16, f * nv * kCbMissCap * 16,
                                fast ? (size_t)P.tab * 8 : (size_t)table_floats * 4, f * nv * cb_rows_grid(P.max_rows) * 32};
    Y.off[0] = 0;
    for (int i = 0; i < CS_N; ++i) Y.off[i + 1] = Y.off[i] + cb_align(bytes[i]);
    Y.need = Y.off[CS_N] + (fast ? kCbFastHeadroom : kCbExactHeadroom);
    return Y;
}

// ---- pass schedule of the exact paired path: per filter the axes 3 - ndim .. 2 in turn ----
enum { SRC_AB = 0, SRC_PREP = 1, SRC_VMASK = 2, DST_AB = 0, DST_SQ = 1, DST_F = 2 };
// buffers: 0..4 = the five temporaries (4: the squared deviation between the filters), kCbBufView = the resampled view with its
// blending weight, kCbBufF = the view's box in the F pool, -1 = none
enum { kCbBufSq = 4, kCbBufView = 5, kCbBufF = 6 };
struct CbPairPass { int filt, axis, src, dst, in_a, in_b, out_a, out_b, T; bool split; size_t lds; };
// the passes of a view with box extents n (returns their number); split: passes along y / z that only hand both quantities on take one
// quantity per workgroup and twice the lines (128-byte pieces)
inline int cb_pair_schedule(int ndim, const int n[3], int r1, int r2, bool nosplit, CbPairPass out[6]) {
    int np = 0;
    for (int f = 0; f < 2; ++f) {
        const int radius = f ? r2 : r1;
        for (int axis = 3 - ndim, pass = 0; axis < 3; ++axis, ++pass, ++np) {
            const bool firstp = axis == 3 - ndim, lastp = axis == 2;
            CbPairPass& p = out[np];
            p.filt = f; p.axis = axis;
            p.src = firstp ? (f ? SRC_VMASK : SRC_PREP) : SRC_AB;
            p.dst = lastp ? (f ? DST_F : DST_SQ) : DST_AB;
            p.in_a = firstp ? (f ? kCbBufSq : kCbBufView) : out[np - 1].out_a;
            p.in_b = firstp ? -1 : out[np - 1].out_b;
            p.out_a = lastp ? (f ? kCbBufF : kCbBufSq) : 2 * (pass & 1);
            p.out_b = lastp ? -1 : 2 * (pass & 1) + 1;
            const int Ts = (p.dst == DST_AB && axis != 2 && !nosplit) ? cb_split_T(n[axis], radius) : 0;
            p.split = Ts > 0;
            p.T = p.split ? Ts : cb_pair_T(n[axis], radius, axis);
            p.lds = cb_pair_lds(n[axis], radius, p.T, p.split);
        }
    }
    return np;
}

// ---- pass schedule of the fast path: 2 * ndim line passes, each ONE launch over all views: I -> T0 -> F -> (squared deviation) T0 -> F
// -> T0 -> F (3D) ----
enum { CBS_PLAIN = 0, CBS_NAN0 = 1, CBD_PLAIN = 0, CBD_SQ = 1, CBD_F = 2 };
enum { kCbBufI = 0, kCbBufT0 = 1, kCbBufFast = 2 };      // pools of the fast path (kCbBufFast: F)
struct CbFastPass { int filt, axis, radius, src_buf, dst_buf, src, dst, nb; size_t lds; CbFastViews views; };      // nb == 0: no launch
inline int cb_fast_schedule(const CbFastViews& VS, int ndim, const int cs[3], const int64_t trim[3], int r1, int r2, const int Tsel[3][2][8],
                            CbFastPass out[6]) {
    int np = 0;
    for (int f = 0; f < 2; ++f)
        for (int axis = 3 - ndim; axis < 3; ++axis, ++np) {
            CbFastPass& p = out[np];
            const bool lastp = axis == 2;
            p.filt = f; p.axis = axis; p.radius = f ? r2 : r1;
            p.src_buf = (np == 0) ? kCbBufI : ((np & 1) ? kCbBufT0 : kCbBufFast);
            p.dst_buf = (np & 1) ? kCbBufFast : kCbBufT0;
            p.src = (np == 0) ? CBS_NAN0 : CBS_PLAIN;
            p.dst = lastp ? (f ? CBD_F : CBD_SQ) : CBD_PLAIN;
            p.views = VS; p.nb = 0; p.lds = 0;
            for (int i = 0; i < VS.nv; ++i) {
                CbFastView& V = p.views.v[i];
                V.T = Tsel[axis][f][i];
                V.blk0 = p.nb;
                V.zr0 = 0; V.nzr = V.n[0]; V.yr0 = 0; V.nyr = V.n[1];
                long long bn = (long long)V.n[0] * V.n[1] * V.n[2];
                // the weight F of a view is read on the TRIMMED chunk only: a view that does not reach it (a sliver of a neighbour in the
                // halo) is not filtered at all, and the last pass works on the rows inside it
                int tl[3], th[3];
                bool reaches = bn > 0;
                for (int k = 0; k < 3; ++k) {
                    tl[k] = (V.lo[k] > (int)trim[k] ? V.lo[k] : (int)trim[k]) - V.lo[k];
                    th[k] = (V.lo[k] + V.n[k] < cs[k] - (int)trim[k] ? V.lo[k] + V.n[k] : cs[k] - (int)trim[k]) - V.lo[k];
                    if (th[k] <= tl[k]) reaches = false;
                }
                if (!reaches) { V.nzr = V.nyr = 0; continue; }
                if (lastp && f == 1) {
                    V.zr0 = tl[0]; V.nzr = th[0] - tl[0]; V.yr0 = tl[1]; V.nyr = th[1] - tl[1];
                    bn = (long long)V.nzr * V.nyr * V.n[2];
                }
                const long long n_lines = bn / V.n[axis];
                p.nb += (int)((n_lines + V.T - 1) / V.T);
                const size_t lds = cb_fast_lds(V.n[axis], p.radius, V.T, axis == 2);
                p.lds = lds > p.lds ? lds : p.lds;
            }
        }
    return np;
}

}  // namespace
