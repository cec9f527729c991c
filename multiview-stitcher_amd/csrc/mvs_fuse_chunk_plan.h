// mvs_fuse_chunk_plan.h -- the one definition of everything the chunk entries (mvs_fuse_chunk_impl in mvs_fuse.hip, the content-based
// and DCT drivers) decide without the device: the brick constants the kernels of mvs_fuse.hip share with the grid, the host arithmetic
// that turns a view into its device records (exact in-bounds ranges, translation-path constants, chunk frame, chunk box), the route of
// a chunk through the four kernel families, and the layouts of the parameter block, the brick grid and the x-weight table.  Plain
// functions: no context, no HIP call, no mvs_fail; tests/native/fuse_chunk_plan_host_test.cpp compiles them for the host
// (tests/test_fuse_chunk_plan_host.py).  The library is built with -ffp-contract=off and so is the test: the bits of the double
// arithmetic below are scipy's.
#pragma once
#include "mvs_fuse_dev.h"
#include "mvs_fuse_tr.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace mvs_fuse_chunk_plan {

// ---- brick constants: the kernels walk what the grid below counts ----------------------------------------------------------------
constexpr int kBrickX = 64;      // generic kernel: voxels along x per brick (16 lanes x 4 voxels)
constexpr int kTrBrickX = 256;   // column kernel: voxels along x per wavefront (64 lanes x 4)
constexpr int kTrRows = 4;       // consecutive y rows per wavefront
constexpr int kTrPlanes = 4;     // z planes per workgroup (one per wavefront)
constexpr int kTrGroups = 8;     // row groups (of kTrRows rows) a wavefront walks with one culled view list
constexpr int kXTabMargin = 4;   // table entries kept on either side of [lo_x, hi_x] (a lane reads 4 consecutive ones)

// ---- view geometry -----------------------------------------------------------------------------------------------------------
// c(i) = fl(i + off) is what the generic kernel (and scipy) test against [0, n-1] for an identity
// matrix; it is monotone in i, so the in-bounds set is an integer interval found exactly here.
// Index frame (mvs_fuse_opts_t.index_origin): `off` refers to frame index i = chunk index + org and to the whole view's pixel
// grid, in which the slab starts at pixel `ioff`: in bounds iff ioff <= fl(i + off) <= ioff + n - 1.
inline void exact_valid_range(double off, int n, int n_out, int* lo_out, int* hi_out, long long org = 0, long long ioff = 0) {
    auto c = [off](long long i) { return (double)i + off; };
    const double cmin = (double)ioff, cmax = (double)(ioff + n - 1);
    long long lo = (long long)ceil(cmin - off);
    while (c(lo - 1) >= cmin) --lo;
    while (c(lo) < cmin) ++lo;
    long long hi = (long long)floor(cmax - off);
    while (c(hi + 1) <= cmax) ++hi;
    while (c(hi) > cmax) --hi;
    lo -= org;
    hi -= org;
    if (lo < 0) lo = 0;
    if (hi > n_out - 1) hi = n_out - 1;
    *lo_out = (int)std::min<long long>(lo, 0x7fffffff);
    *hi_out = (int)std::max<long long>(hi, -1);   // lo > hi: the view never contributes
}

// Decide whether a view qualifies for the translation fast path and derive its constants.
inline void prepare_translation_view(DevView* d, int order, int fusion, const int64_t chunk_shape[3], size_t elem_size,
                                     const int64_t* org = nullptr, const int64_t* ioff = nullptr) {
    static const int64_t zero3[3] = {0, 0, 0};
    if (!org) org = zero3;
    if (!ioff) ioff = zero3;
    d->tr_ok = 0;
    static const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k)
        if (d->m[k] != I9[k]) return;
    const int n[3] = {d->nz, d->ny, d->nx};
    for (int k = 0; k < 3; ++k) {
        if (!(fabs(d->off[k]) < 1048576.0) || n[k] > 65536 || chunk_shape[k] > 65536) return;
        if (std::llabs(org[k]) > (1 << 24) || std::llabs(ioff[k]) > (1 << 24)) return;
        if (!(fabs(d->off[k] + (double)(org[k] - ioff[k])) < 65536.0)) return;
    }
    if (fusion == MVS_FUSE_WEIGHTED_AVERAGE) {
        const int offd[6] = {1, 2, 3, 5, 6, 7};
        for (int k : offd)
            if (d->wm[k] != 0.0) return;
        // closed-form check of the support table: edt == min_d(ws_d * tent(i_d))
        const int nz = d->wnz;
        float sz = INFINITY, sy, sx;
        if (nz == 5) {
            sz = d->edt[(1 * 5 + 2) * 5 + 2];
            sy = d->edt[(2 * 5 + 1) * 5 + 2];
            sx = d->edt[(2 * 5 + 2) * 5 + 1];
        } else {
            sy = d->edt[1 * 5 + 2];
            sx = d->edt[2 * 5 + 1];
        }
        for (int i = 0; i < nz; ++i)
            for (int j = 0; j < 5; ++j)
                for (int k = 0; k < 5; ++k) {
                    float t = fminf(sy * (float)std::min(j, 4 - j), sx * (float)std::min(k, 4 - k));
                    if (nz == 5) t = fminf(t, sz * (float)std::min(i, 4 - i));
                    if (t != d->edt[(i * 5 + j) * 5 + k]) return;
                }
        d->ws[0] = (nz == 5) ? sz : 0.f;
        d->ws[1] = sy;
        d->ws[2] = sx;
        for (int k = 0; k < 3; ++k) {
            d->sup_k[k] = 0.f;
            d->sup_ilo[k] = d->sup_ihi[k] = 0;
            d->sup_flo[k] = d->sup_fhi[k] = 0.f;
            if (k == 0 && nz == 1) continue;
            const double wm = d->wm[k * 4], wo = d->woff[k];
            if (!(wm > 0.0)) return;
            const double lo = -wo / wm;          // frame index where the support coordinate is 0
            const double hi = (4.0 - wo) / wm;   // ... and 4
            if (!(fabs(lo) < 1e6) || !(fabs(hi) < 1e6)) return;
            d->sup_k[k] = (float)wm;
            d->sup_ilo[k] = (int)((long long)floor(lo) - org[k]);     // chunk index = frame index - org (integers: exact)
            d->sup_flo[k] = (float)(lo - floor(lo));
            d->sup_ihi[k] = (int)((long long)ceil(hi) - org[k]);
            d->sup_fhi[k] = (float)(ceil(hi) - hi);
        }
    }
    d->span = (long long)(d->nz - 1) * d->stride_z + (long long)(d->ny - 1) * d->stride_y + d->nx;
    if (d->stride_z > 0x7fffffffLL || d->stride_y > 0x7fffffffLL || d->stride_z < 0 || d->stride_y < 0) return;
    // 32-bit signed byte offsets in the buffer loads; windows may start up to a few rows before / after the slab
    if ((long long)d->span * (long long)elem_size >= (1ll << 31) - (1ll << 27) || (long long)d->stride_z * (long long)elem_size >= (1ll << 26)) return;
    for (int k = 0; k < 3; ++k) {
        const double off = d->off[k];
        // slab pixel = chunk index + org + off - ioff: the integer parts are combined as integers, so the fraction (and with
        // it every interpolation weight) does not depend on which chunk / slab the voxel is seen through
        if (order == 0) {
            d->io[k] = (int)((long long)floor(off + 0.5) + org[k] - ioff[k]);
            d->fw[k] = 0.f;
        } else {
            const double f = floor(off);
            d->io[k] = (int)((long long)f + org[k] - ioff[k]);
            d->fw[k] = (float)(off - f);
        }
        exact_valid_range(off, n[k], (int)chunk_shape[k], &d->lo[k], &d->hi[k], org[k], ioff[k]);
    }
    d->pad[0] = (order == 0) ? 0.f : 1.f;   // carried into TrView.linear
    d->tr_ok = 1;
}

inline void fill_tr_view(const DevView& d, TrView* t) {
    memset(t, 0, sizeof(*t));
    for (int k = 0; k < 3; ++k) {
        t->lo[k] = d.lo[k];
        t->hi[k] = d.hi[k];
        t->io[k] = d.io[k];
        t->fw[k] = d.fw[k];
        t->sup_ilo[k] = d.sup_ilo[k];
        t->sup_ihi[k] = d.sup_ihi[k];
        t->sup_flo[k] = d.sup_flo[k];
        t->sup_fhi[k] = d.sup_fhi[k];
        t->sup_k[k] = d.sup_k[k];
        t->ws[k] = d.ws[k];
    }
    t->wnz = d.wnz;
    t->n[0] = d.nz; t->n[1] = d.ny; t->n[2] = d.nx;
    t->linear = d.pad[0] != 0.f ? 1 : 0;
    t->data = (unsigned long long)d.data;
    t->span = d.span;
    t->stride_y = (int)d.stride_y;
    t->stride_z = (int)d.stride_z;
    t->xtab_off = 0;
}

// Index frame -> chunk frame for the kernels that evaluate the full affine map per voxel (generic fuse kernel, resample,
// blend): c = M (p + org) + off - ioff = M p + (off + M org - ioff).  (The translation fast path keeps the integer parts apart,
// see prepare_translation_view; here the last bit of a coordinate may depend on the chunk, as it does in the reference.)
inline void view_to_chunk_frame(DevView* d, const int64_t org[3], const int64_t ioff[3]) {
    if (!(org[0] | org[1] | org[2] | ioff[0] | ioff[1] | ioff[2])) return;
    const double o[3] = {(double)org[0], (double)org[1], (double)org[2]};
    for (int k = 0; k < 3; ++k) {
        d->off[k] = (((o[0] * d->m[3 * k] + o[1] * d->m[3 * k + 1]) + o[2] * d->m[3 * k + 2]) + d->off[k]) - (double)ioff[k];
        d->woff[k] = ((o[0] * d->wm[3 * k] + o[1] * d->wm[3 * k + 1]) + o[2] * d->wm[3 * k + 2]) + d->woff[k];
    }
}

// Chunk-index box [lo, hi] (inclusive; lo > hi: empty) outside of which view `d` is certainly out of bounds: exact for
// translations (the interval scipy's in-bounds test yields, as in the fast path), the bounding box of the slab's corners mapped
// into the chunk (+- 2 voxels) otherwise.
inline void view_chunk_box(const DevView& d, const int64_t shape[3], int lo[3], int hi[3]) {
    static const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    bool ident = true;
    for (int k = 0; k < 9; ++k) ident = ident && d.m[k] == I9[k];
    const int n[3] = {d.nz, d.ny, d.nx};
    if (ident) {
        for (int k = 0; k < 3; ++k) {
            if (!(fabs(d.off[k]) < 1e9)) { lo[k] = 0; hi[k] = (int)shape[k] - 1; continue; }
            exact_valid_range(d.off[k], n[k], (int)shape[k], &lo[k], &hi[k]);
        }
        return;
    }
    const double* m = d.m;
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    for (int k = 0; k < 3; ++k) { lo[k] = 0; hi[k] = (int)shape[k] - 1; }
    if (!(fabs(det) > 1e-12)) return;
    const double inv[9] = {(m[4] * m[8] - m[5] * m[7]) / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
                           (m[5] * m[6] - m[3] * m[8]) / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
                           (m[3] * m[7] - m[4] * m[6]) / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det};
    double bl[3] = {1e300, 1e300, 1e300}, bh[3] = {-1e300, -1e300, -1e300};
    for (int q = 0; q < 8; ++q) {
        const double in[3] = {(q & 4) ? (double)(n[0] - 1) - d.off[0] : -d.off[0], (q & 2) ? (double)(n[1] - 1) - d.off[1] : -d.off[1],
                              (q & 1) ? (double)(n[2] - 1) - d.off[2] : -d.off[2]};
        for (int k = 0; k < 3; ++k) {
            const double o = inv[3 * k] * in[0] + inv[3 * k + 1] * in[1] + inv[3 * k + 2] * in[2];
            bl[k] = std::min(bl[k], o);
            bh[k] = std::max(bh[k], o);
        }
    }
    for (int k = 0; k < 3; ++k) {
        lo[k] = (int)std::max(0.0, std::floor(bl[k]) - 2.0);
        hi[k] = (int)std::min((double)shape[k] - 1.0, std::ceil(bh[k]) + 2.0);
    }
}

// Device record of a view whose x stride and shape mvs_fill_dev_view (mvs_fuse.hip) has checked; the translation path is not set
inline void fill_dev_view(const mvs_view_t& v, int ndim, const void* dev_data, DevView* d) {
    d->data = dev_data;
    d->stride_z = v.stride[0];
    d->stride_y = v.stride[1];
    d->nz = (int)v.shape[0];
    d->ny = (int)v.shape[1];
    d->nx = (int)v.shape[2];
    d->wnz = (ndim == 3) ? 5 : 1;
    memcpy(d->m, v.matrix, sizeof(d->m));
    memcpy(d->off, v.offset, sizeof(d->off));
    memcpy(d->wm, v.w_matrix, sizeof(d->wm));
    memcpy(d->woff, v.w_offset, sizeof(d->woff));
    memcpy(d->edt, v.edt, sizeof(d->edt));
    d->pad[0] = d->pad[1] = d->pad[2] = 0.f;
}

// The record of a weight tile that reads its data at dev_data (NULL: no weights), in the chunk frame: the tile is whole
// (index_offset 0), so c = M (p + org) + off with the operation order of view_to_chunk_frame.
inline void fill_weight_view(const mvs_view_t& v, const void* dev_data, const int64_t org[3], WeightView* d) {
    memset(d, 0, sizeof(*d));
    d->data = (const unsigned char*)dev_data;
    if (!dev_data) return;
    d->stride_z = v.stride[0];
    d->stride_y = v.stride[1];
    d->nz = (int)v.shape[0];
    d->ny = (int)v.shape[1];
    d->nx = (int)v.shape[2];
    memcpy(d->m, v.matrix, sizeof(d->m));
    memcpy(d->off, v.offset, sizeof(d->off));
    if (!(org[0] | org[1] | org[2])) return;
    const double o[3] = {(double)org[0], (double)org[1], (double)org[2]};
    for (int k = 0; k < 3; ++k) d->off[k] = ((o[0] * d->m[3 * k] + o[1] * d->m[3 * k + 1]) + o[2] * d->m[3 * k + 2]) + d->off[k];
}

// A filled view as the chunk sees it: its translation-path constants in the index frame, then the chunk frame for the kernels that
// evaluate the affine map, then -- when the view qualifies (returns true; not rotated / scaled views, nor, under weighted average, a
// support table that is not the closed form) -- its translation-path record.
inline bool tr_view_in_chunk(DevView* d, int order, int fusion, const int64_t chunk_shape[3], size_t elem_size, const int64_t org[3],
                             const int64_t ioff[3], TrView* out) {
    prepare_translation_view(d, order, fusion, chunk_shape, elem_size, org, ioff);
    view_to_chunk_frame(d, org, ioff);
    if (!d->tr_ok) return false;
    fill_tr_view(*d, out);
    return true;
}

// ---- the route of a chunk ---------------------------------------------------------------------------------------------------
//   use_tr  = !force_generic && !dct && every view tr_ok, and for float32 at order 1 only under weighted average (WA)
//   float32 at order 1 (use_tr): rows, else generic           -- scipy multiplies the second tap of every axis by its (possibly zero)
//                                                                weight, so a NaN there poisons the sample; only the row kernels and
//                                                                the generic kernel read all taps
//   WA, rows_v1 (use_tr):        rows, else regions unless no_regions, else column
//   WA (use_tr):                 regions unless no_regions, else column
//   max / simple average (use_tr): column
//   !use_tr:                     generic
// The column kernel lists at most 64 views per column: with more views in the chunk its overflow word is read back, and a raised
// word sends the chunk through the generic kernel once more.
enum Family { kRows, kRegions, kColumn, kGeneric };
enum GridKind { kGenericBricks, kTrBricks };
inline GridKind family_grid(Family f) { return f == kColumn ? kTrBricks : kGenericBricks; }      // (rows and regions plan bricks of their own)
struct RouteInputs {
    int dtype, order, fusion;      // MVS_U8 / MVS_U16 / MVS_F32, 0 / 1, MVS_FUSE_*
    bool dct;                      // DCT-entropy quality grids multiply the weights (mvs_fuse_chunk_dct)
    bool all_tr_ok;                // every view qualifies for the translation path
    bool force_generic, rows_v1, no_regions;      // switches of the context
    int n_views;
};
struct Route {
    bool use_tr;                   // the views' cull boxes, translation records and x-table offsets are built
    bool try_rows, try_regions;    // families asked in turn; each may decline the chunk
    Family fallback;               // kColumn or kGeneric: takes the chunk when no family before it did
    GridKind grid;                 // the fallback's brick grid
    GridKind first_grid;           // the grid whose block count is checked before anything is timed (the translation path's when use_tr)
    bool read_overflow;            // the column kernel's overflow word is read back
};
inline Route route(const RouteInputs& in) {
    Route r;
    const bool wa = in.fusion == MVS_FUSE_WEIGHTED_AVERAGE, nan_exact = in.dtype == MVS_F32 && in.order == 1;
    r.use_tr = !in.force_generic && !in.dct && in.all_tr_ok && !(nan_exact && !wa);
    r.try_rows = r.use_tr && wa && (in.rows_v1 || nan_exact);
    r.try_regions = r.use_tr && wa && !nan_exact && !in.no_regions;
    r.fallback = (r.use_tr && !nan_exact) ? kColumn : kGeneric;
    r.grid = family_grid(r.fallback);
    r.first_grid = r.use_tr ? kTrBricks : kGenericBricks;
    r.read_overflow = r.fallback == kColumn && in.n_views > 64;
    return r;
}

// ---- layouts ---------------------------------------------------------------------------------------------------------------------
// the parameter block of a chunk, in the pinned staging slot and in scratch slot 2: DevView[n] | cull[6][n] (SoA: zlo, zhi, ylo, yhi,
// xlo, xhi) | TrView[n], each part on a multiple of 256 bytes
struct ParamBlock { size_t views, cull, tr, total; };
inline ParamBlock param_block(int n_views) {
    ParamBlock b;
    b.views = 0;
    b.cull = align_up(sizeof(DevView) * (size_t)n_views);
    b.tr = b.cull + align_up(sizeof(int) * 6 * (size_t)n_views);
    b.total = b.tr + sizeof(TrView) * (size_t)n_views;
    return b;
}

// bricks of the trimmed result `os`: generic kernel 4 x 4 x 64 (2-D: 1 x 16 x 64), column kernel kTrPlanes x (kTrRows kTrGroups) x
// kTrBrickX (2-D: one plane, four wavefronts side by side along y)
struct BrickGrid {
    int bz, by;            // brick extent along z and y
    int nbz, nby, nbx;
    long long nblocks;
    bool fits_one_launch() const { return nblocks <= 0x7fffffffLL; }
};
inline BrickGrid brick_grid(GridKind kind, const int64_t os[3]) {
    BrickGrid g;
    const bool tr = kind == kTrBricks;
    const int oz = (int)os[0], oy = (int)os[1], ox = (int)os[2];
    if (tr) {
        g.bz = (os[0] > 1) ? kTrPlanes : 1;
        g.by = (os[0] > 1) ? kTrRows * kTrGroups : 4 * kTrRows * kTrGroups;
    } else {
        g.bz = (os[0] > 1) ? 4 : 1;
        g.by = (os[0] > 1) ? 4 : 16;
    }
    const int brick_x = tr ? kTrBrickX : kBrickX;
    g.nbz = (oz + g.bz - 1) / g.bz;
    g.nby = (oy + g.by - 1) / g.by;
    g.nbx = (ox + brick_x - 1) / brick_x;
    g.nblocks = (long long)g.nbz * g.nby * g.nbx;
    return g;
}

// x-weight table of the column kernel (xweight_table_kernel): per view its chunk x range [lo, hi] with kXTabMargin entries on
// either side, view after view.  xtab_add gives TrView.xtab_off -- the entry of x = lo -- and advances the running total; the
// scratch holds the table, 64 spare floats and, behind them, the overflow word.
inline int xtab_add(size_t* total, int lo_x, int hi_x) {
    const int off = (int)*total + kXTabMargin;
    *total += (size_t)std::max(hi_x - lo_x + 1, 0) + 2 * kXTabMargin;
    return off;
}
inline size_t xtab_overflow_at(size_t total) { return total + 64; }      // index of the overflow word, in floats
inline size_t xtab_bytes(size_t total) { return (total + 64) * sizeof(float) + 256; }

}  // namespace mvs_fuse_chunk_plan
