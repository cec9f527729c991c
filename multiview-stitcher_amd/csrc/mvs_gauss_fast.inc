// mvs_gauss_fast.inc -- round 6: the FAST content-based path (included by mvs_gauss.hip inside its anonymous namespace).
//
// The bit-faithful passes of mvs_gauss.hip (option "cb_exact" = 1) reproduce scipy's float64 accumulators and filter the valid
// mask of every view through all three axes of both Gaussians.  The bar of north_star is the ORACLE at 1e-4 relative on the fused
// voxels, not the bits of scipy's intermediates, so the default path spends its HBM traffic and its issue slots differently:
//
//  * the valid mask is the box of the view minus a short list of voxels (weights.py:54-55 sets I to NaN where the normalised
//    blending weight is < 1e-7: the outermost layer of a tile and a few dozen voxels next to its corners, where two or three cosine
//    ramps are small at once).  cb_rows_kernel / cb_missing_kernel find the box and the list on the device (nothing is assumed:
//    a list that does not fit raises a flag and the caller redoes the call on the exact path); gaussian(mask) is then
//        WW(z, y, x) = Gz(z) Gy(y) Gx(x)  -  sum over the listed voxels s of  wz(z, s) wy(y, s) wx(x, s)
//    with 1-D tables G of the box indicator (cb_tables_kernel, reflect at the chunk's ends like the filters) and the listed voxels'
//    separable bumps evaluated only on the lines they reach.  NO mask array is filtered: every pass carries ONE quantity.
//  * mask_normalize8_kernel stores NaN into the resampled view where the weight falls below 1e-7, so "valid" is "finite" and the
//    passes never read the blending weights;
//  * the taps accumulate in float32 (far taps first, the centre last: partial sums grow with the terms), option "cb_taps_f64"
//    switches to float64 accumulators for A/B;
//  * ONE launch per pass for all views of the chunk (view v owns the workgroups [blk0[v], blk0[v + 1])): 2 * ndim line launches per
//    chunk instead of 2 * ndim per view.
//
// Reference: weights.py:22-74 (content_based), :293-322 (nan_gaussian_filter), :325-345 (normalize_weights); fusion/_core.py:1199-1220.

struct CbFastRec { unsigned long long cnt; int lo[3]; int hi[3]; int nmiss; int pad[7]; };      // lo / hi: box-local bounding box of the valid voxels
static_assert(sizeof(CbFastRec) == 64, "CbFastRec layout");

// ---- valid voxels per row (one wavefront per group of 4 rows, their loads in flight together), per-workgroup partial records of
// the view's count and bounding box (no atomics: a few thousand of them on one cache line cost more than the scan itself);
// cb_rec_reduce_kernel folds the partials into the view's record ----
struct CbPartial { unsigned long long cnt; int lo[3]; int hi[3]; };
static_assert(sizeof(CbPartial) == 32, "CbPartial layout");
__global__ __launch_bounds__(256) void cb_rows_kernel(const float* __restrict__ I, CbFastViews VS, int4* __restrict__ rows, CbPartial* __restrict__ partials) {
    const CbFastView V = VS.v[blockIdx.y];
    const int nrows = V.n[0] * V.n[1], nx = V.n[2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long cnt = 0;
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
    for (int row0 = (blockIdx.x * 4 + wave) * 4; row0 < nrows; row0 += gridDim.x * 16) {
        int rc[4] = {0, 0, 0, 0}, first[4] = {-1, -1, -1, -1}, last[4] = {-1, -1, -1, -1};
        for (int x0 = 0; x0 < nx; x0 += 256) {
            float val[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int x = x0 + q * 64 + lane;
                    const int row = min(row0 + r, nrows - 1);
                    val[r][q] = I[V.off + (long long)row * nx + min(x, nx - 1)];
                }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int xq = x0 + q * 64;
                    const bool ok = (xq + lane < nx) && (val[r][q] == val[r][q]);
                    const unsigned long long b = __ballot(ok);
                    if (b) {
                        rc[r] += __popcll(b);
                        if (first[r] < 0) first[r] = xq + __ffsll((long long)b) - 1;
                        last[r] = xq + 63 - __clzll((long long)b);
                    }
                }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + r;
            if (row >= nrows) break;
            if (lane == 0) rows[V.row0 + row] = make_int4(rc[r], first[r], last[r], 0);
            if (rc[r]) {
                const int bz = row / V.n[1], by = row - bz * V.n[1];
                cnt += rc[r];
                lo[0] = min(lo[0], bz); hi[0] = max(hi[0], bz);
                lo[1] = min(lo[1], by); hi[1] = max(hi[1], by);
                lo[2] = min(lo[2], first[r]); hi[2] = max(hi[2], last[r]);
            }
        }
    }
    __shared__ unsigned long long s_cnt[4];
    __shared__ int s_lo[4][3], s_hi[4][3];
    if (lane == 0) {
        s_cnt[wave] = cnt;
        for (int k = 0; k < 3; ++k) { s_lo[wave][k] = lo[k]; s_hi[wave][k] = hi[k]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) {
            cnt += s_cnt[q];
            for (int k = 0; k < 3; ++k) { lo[k] = min(lo[k], s_lo[q][k]); hi[k] = max(hi[k], s_hi[q][k]); }
        }
        CbPartial P;
        P.cnt = cnt;
        for (int k = 0; k < 3; ++k) { P.lo[k] = lo[k]; P.hi[k] = hi[k]; }
        partials[blockIdx.y * gridDim.x + blockIdx.x] = P;
    }
}
__global__ __launch_bounds__(256) void cb_rec_reduce_kernel(const CbPartial* __restrict__ partials, int per_view, CbFastRec* __restrict__ recs) {
    mvs_fold::CountBox<unsigned long long> a = {0, {0x7fffffff, 0x7fffffff, 0x7fffffff}, {-1, -1, -1}};
    for (int i = threadIdx.x; i < per_view; i += blockDim.x) {
        const CbPartial P = partials[blockIdx.x * per_view + i];
        a.merge({P.cnt, {P.lo[0], P.lo[1], P.lo[2]}, {P.hi[0], P.hi[1], P.hi[2]}});
    }
    a = mvs_fold::block_fold<4>(a);
    if (threadIdx.x == 0) {
        CbFastRec R;
        R.cnt = a.n;
        for (int k = 0; k < 3; ++k) { R.lo[k] = a.lo[k]; R.hi[k] = a.hi[k]; }
        R.nmiss = 0;
        for (int k = 0; k < 7; ++k) R.pad[k] = 0;
        recs[blockIdx.x] = R;
    }
}

// ---- the invalid voxels inside the bounding box: rows of the box that are not full are scanned (one thread per row) ----
__global__ __launch_bounds__(256) void cb_missing_kernel(const float* __restrict__ I, CbFastViews VS, const int4* __restrict__ rows, CbFastRec* __restrict__ recs,
                                                         int4* __restrict__ miss, int* __restrict__ flag) {
    const CbFastView V = VS.v[blockIdx.y];
    CbFastRec* R = recs + blockIdx.y;
    if (R->cnt == 0ull) return;
    const int lo0 = R->lo[0], hi0 = R->hi[0], lo1 = R->lo[1], hi1 = R->hi[1], lo2 = R->lo[2], hi2 = R->hi[2];
    const int nrows = V.n[0] * V.n[1], W = hi2 - lo2 + 1;
    for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < nrows; row += gridDim.x * blockDim.x) {
        const int bz = row / V.n[1], by = row - bz * V.n[1];
        if (bz < lo0 || bz > hi0 || by < lo1 || by > hi1) continue;
        if (rows[V.row0 + row].x == W) continue;
        const float* p = I + V.off + (long long)row * V.n[2];
        for (int x = lo2; x <= hi2; ++x) {
            const float val = p[x];
            if (val == val) continue;
            const int k = atomicAdd(&R->nmiss, 1);
            if (k < kCbMissCap) miss[blockIdx.y * kCbMissCap + k] = make_int4(bz, by, x, 0);
            else *flag = 1;
        }
    }
}

// ---- the list in a fixed order (atomics filled it in the order the rows were scheduled): bitonic sort of <= 512 keys ----
__global__ __launch_bounds__(512) void cb_sort_missing_kernel(CbFastRec* __restrict__ recs, int4* __restrict__ miss) {
    __shared__ unsigned long long key[kCbMissCap];
    int4* M = miss + blockIdx.x * kCbMissCap;
    const int nm = min(recs[blockIdx.x].nmiss, kCbMissCap);
    if (nm <= 1) return;      // (uniform)
    const int t = threadIdx.x;
    unsigned long long k = ~0ull;
    if (t < nm) { const int4 m = M[t]; k = ((unsigned long long)m.x << 40) | ((unsigned long long)m.y << 20) | (unsigned long long)m.z; }
    key[t] = k;
    __syncthreads();
    for (int size = 2; size <= kCbMissCap; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int partner = t ^ stride;
            if (partner > t) {
                const bool up = (t & size) == 0;
                const unsigned long long a = key[t], b = key[partner];
                if ((a > b) == up) { key[t] = b; key[partner] = a; }
            }
            __syncthreads();
        }
    if (t < nm) { const unsigned long long q = key[t]; M[t] = make_int4((int)(q >> 40), (int)((q >> 20) & 0xfffff), (int)(q & 0xfffff), 0); }
}

// ---- 1-D tables of the box indicator under the line filter: G_axis[p] = sum_j w_j [reflect(p + j) in [lo_axis, hi_axis]] (float64).
// grid = (3 axes, views, 2 filters).  Layout per view: filter f at tab0 + f * (n0 + n1 + n2): Gz[n0], Gy[n1], Gx[n2]. ----
__global__ __launch_bounds__(256) void cb_tables_kernel(CbFastViews VS, const CbFastRec* __restrict__ recs, Shape3 S, int ndim, int r1,
                                                        const double* __restrict__ fw1, int r2, const double* __restrict__ fw2, double* __restrict__ tabs) {
    const int axis = blockIdx.x, v = blockIdx.y, f = blockIdx.z;
    const CbFastView V = VS.v[v];
    const CbFastRec R = recs[v];
    const int radius = f ? r2 : r1;
    const double* fw = f ? fw2 : fw1;
    const int len = V.n[axis], b0 = V.lo[axis], full = (&S.nz)[axis];
    double* out = tabs + V.tab0 + (long long)f * (V.n[0] + V.n[1] + V.n[2]) + (axis > 0 ? V.n[0] : 0) + (axis > 1 ? V.n[1] : 0);
    const int lo = R.lo[axis], hi = R.hi[axis];
    const bool filtered = axis >= 3 - ndim;      // a 2D chunk has no z pass
    for (int p = threadIdx.x; p < len; p += blockDim.x) {
        double acc = 0.0;
        if (R.cnt) {
            if (!filtered) acc = (p >= lo && p <= hi) ? 1.0 : 0.0;
            else
                for (int j = -radius; j <= radius; ++j) {
                    int q = p + j;
                    if ((unsigned)q >= (unsigned)len) q = box_reflect(q, b0, len, full);
                    if (q >= lo && q <= hi) acc += fw[radius + j];
                }
        }
        out[p] = acc;
    }
}

// weight with which the line filter at box position p picks up the voxel at box position s: sum over the images of s under the
// reflection at the chunk's ends (s, -1 - s, 2 full - 1 - s in chunk coordinates; radius <= full: no further image in reach)
__device__ __forceinline__ double cb_axis_weight(int p, int s, int b0, int full, int radius, const double* __restrict__ fw, bool filtered) {
    if (!filtered) return p == s ? 1.0 : 0.0;
    const int q = p + b0, t = s + b0;
    double w = 0.0;
    const int d0 = t - q, d1 = -1 - t - q, d2 = 2 * full - 1 - t - q;
    if (d0 >= -radius && d0 <= radius) w += fw[radius + d0];
    if (d1 >= -radius && d1 <= radius) w += fw[radius + d1];
    if (d2 >= -radius && d2 <= radius) w += fw[radius + d2];
    return w;
}
__device__ __forceinline__ bool cb_axis_reach(int a, int b, int s, int b0, int full, int radius, bool filtered) {      // any of p in [a, b] reaches s
    if (!filtered) return s >= a && s <= b;
    const int qa = a + b0 - radius, qb = b + b0 + radius, t = s + b0;
    const int i1 = -1 - t, i2 = 2 * full - 1 - t;
    return (t >= qa && t <= qb) || (i1 >= qa && i1 <= qb) || (i2 >= qa && i2 <= qb);
}

// the same from a float32 copy of the weights in LDS, without branches (the last pass evaluates it per output sample inside a serial
// walk over the listed voxels: from global memory every step of that walk was a memory round trip)
__device__ __forceinline__ float cb_axis_weight_lds(int p, int s, int b0, int full, int radius, const float* __restrict__ sfw) {
    const int q = p + b0, t = s + b0;
    const int d0 = t - q, d1 = -1 - t - q, d2 = 2 * full - 1 - t - q;
    const int a0 = abs(d0), a1 = abs(d1), a2 = abs(d2);
    float w = (a0 <= radius) ? sfw[radius - min(a0, radius)] : 0.f;      // (symmetric kernel: index radius - |d|)
    w += (a1 <= radius) ? sfw[radius - min(a1, radius)] : 0.f;
    w += (a2 <= radius) ? sfw[radius - min(a2, radius)] : 0.f;
    return w;
}

// ---- the line filter of ONE quantity, all views of the chunk in one launch ----
typedef float cb_f4u_t __attribute__((ext_vector_type(4), aligned(4)));      // 16-byte access at 4-byte alignment (rows of odd length)
struct CbLineArgs {
    const float* src; float* dst; const float* I;      // pools (a view's box at + off)
    int axis, radius, ndim, filt;
    Shape3 S;                                          // the chunk (reflection)
    const float* fwf; const double* fwd;               // the filter's 2 radius + 1 weights
    const double* tabs; const CbFastRec* recs; const int4* miss;
};
#ifndef MVS_CBF_PREFETCH
#define MVS_CBF_PREFETCH 1      // the view's 8 samples of the last pass are requested before the taps, not after them
#endif
#ifndef MVS_CBF_NACC
#define MVS_CBF_NACC 2
#endif
#ifndef MVS_CBF_NB
#define MVS_CBF_NB 8
#endif

template <int SRC, int DST, typename ACC, bool PF>
__global__ __launch_bounds__(256) void cb_line_kernel(CbLineArgs A, CbFastViews B) {
    static_assert(PF || DST == CBD_PLAIN, "the last pass of a filter runs along x");
    extern __shared__ float sl[];
    int v = 0;
    while (v + 1 < B.nv && (int)blockIdx.x >= B.v[v + 1].blk0) ++v;
    const CbFastView& V = B.v[v];
    const int axis = PF ? 2 : A.axis, radius = A.radius;
    const int nz = V.n[0], ny = V.n[1], nx = V.n[2];
    int len;
    long long stride, n_lines, inner, outer_stride;
    if (axis == 2) { len = nx; stride = 1; n_lines = (long long)V.nzr * V.nyr; inner = 1; outer_stride = nx; }
    else if (axis == 1) { len = ny; stride = nx; n_lines = (long long)nz * nx; inner = nx; outer_stride = (long long)ny * nx; }
    else { len = nz; stride = (long long)ny * nx; n_lines = (long long)ny * nx; inner = (long long)ny * nx; outer_stride = 0; }
    constexpr int K = kGaussK;
    const int T = V.T, TP = T + 1, lt = 31 - __clz(T);
    const int S8 = cb_pf_S8(len + 2 * radius + K), LP = 8 * S8 + 11;
    // LDS index of row r (= position + radius) of line `line`
    auto lidx = [&](int line, int r) { return PF ? line * LP + (r & 7) * S8 + (r >> 3) : r * TP + line; };
    const int b0 = V.lo[axis], full = (&A.S.nz)[axis];
    const long long l0 = (long long)((int)blockIdx.x - V.blk0) * T;
    const int nl = (int)min((long long)T, n_lines - l0);
    const float* src = A.src + V.off;
    float* dst = A.dst + V.off;
    __shared__ long long lbase[64];
    if ((int)threadIdx.x < T) {
        const long long l = min(l0 + threadIdx.x, n_lines - 1);
        if (PF) { const int rz = (int)(l / V.nyr); lbase[threadIdx.x] = ((long long)(V.zr0 + rz) * ny + V.yr0 + (int)(l - (long long)rz * V.nyr)) * nx; }
        else lbase[threadIdx.x] = (l / inner) * outer_stride + (l % inner);
    }
    // ---- the listed voxels this workgroup's lines can see (last pass of a filter only), in list order ----
    __shared__ unsigned s_nearmask[kCbMissCap / 32];
    // ... compacted in list order (<= kCbNear of them; more: the items walk the mask themselves), with the weight wz * wy of every
    // (voxel, line) worked out once per workgroup instead of once per 8-sample block
    constexpr int kCbNear = kCbNearCap;
    __shared__ int s_nn, s_mz[kCbNear], s_my[kCbNear], s_mx[kCbNear];
    float* s_wzy = sl + (PF ? T * LP : 0);      // [kCbNear][T] behind the lines (the host sizes the dynamic LDS for it)
    // bit r of s_lmask[line]: compacted voxel r reaches the line (wz * wy != 0); of s_emask[blk]: it reaches the block along x.  An item
    // walks the intersection -- for nearly all items of a workgroup near a tile corner that is no voxel at all
    constexpr int kCbBlkMax = 128;
    constexpr int NW = kCbNear / 64;
    __shared__ unsigned long long s_lmask[(DST != CBD_PLAIN) ? 32 * NW : 1], s_emask[(DST != CBD_PLAIN) ? kCbBlkMax * NW : 1];
    int nm = 0;
    // (the list's entries are requested here, unconditionally, and looked at after the lines are staged: a workgroup is a short
    // dependent chain, and two more memory round trips in front of its staging loads cost it a third of its time)
    static_assert(kCbMissCap == 512, "two list entries per thread of a 256-thread workgroup");
    int4 mym = make_int4(0, 0, 0, 0);
    __shared__ float s_fwx[(DST != CBD_PLAIN) ? kCbMaxRadius + 1 : 1];      // weights radius .. 0 taps from the centre: s_fwx[radius - |d|]
    if constexpr (DST != CBD_PLAIN) {
        if ((int)threadIdx.x <= radius) s_fwx[threadIdx.x] = A.fwf[threadIdx.x];
        nm = A.recs[v].nmiss;
        mym = A.miss[v * kCbMissCap + threadIdx.x];
        if (threadIdx.x < kCbMissCap / 32) s_nearmask[threadIdx.x] = 0u;
        if (threadIdx.x == 0) s_nn = 0;
    }
    __syncthreads();
    // ---- stage the lines: the loads of NB samples are requested back to back before the first of them is written to LDS ----
    constexpr int NB = MVS_CBF_NB;
    const int per_line = PF ? (int)blockDim.x : ((int)blockDim.x >> lt);
    const int my_line = PF ? 0 : (int)(threadIdx.x & (T - 1));
    const int my_pos0 = PF ? (int)threadIdx.x : (int)(threadIdx.x >> lt);
    const int sweeps = (len + per_line - 1) / per_line;
    const int n_my = PF ? sweeps * T : sweeps;
    for (int e0 = 0; e0 < n_my; e0 += NB) {
        float q[NB];
        int bl[NB], bp[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int e = e0 + u;
            const int line = PF ? e / sweeps : my_line;
            const int sweep = PF ? e - line * sweeps : e;
            const int pos = my_pos0 + sweep * per_line;
            bl[u] = line; bp[u] = pos;
            q[u] = src[lbase[min(line, nl - 1)] + (long long)min(pos, len - 1) * stride];
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int e = e0 + u;
            if (e < n_my && bp[u] < len && bl[u] < T) {
                float val = bl[u] < nl ? q[u] : 0.f;
                if constexpr (SRC == CBS_NAN0) val = (val == val) ? val : 0.f;
                sl[lidx(bl[u], bp[u] + radius)] = val;
            }
        }
    }
    if constexpr (DST != CBD_PLAIN) {
        nm = min(nm, kCbMissCap);
        if (nm > 0) {
            const int ra = (int)(l0 / V.nyr), rb = (int)((l0 + nl - 1) / V.nyr);
            const int za = V.zr0 + ra, zb = V.zr0 + rb;
            const int ya = V.yr0 + (ra == rb ? (int)(l0 - (long long)ra * V.nyr) : 0), yb = V.yr0 + (ra == rb ? (int)(l0 + nl - 1 - (long long)ra * V.nyr) : V.nyr - 1);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int e = h * 256 + (int)threadIdx.x;
                if (e >= nm) break;
                const int4 m = h ? A.miss[v * kCbMissCap + e] : mym;      // (lists beyond 256 voxels are rare)
                if ( cb_axis_reach(za, zb, m.x, V.lo[0], A.S.nz, radius, A.ndim == 3) && cb_axis_reach(ya, yb, m.y, V.lo[1], A.S.ny, radius, true))
                    atomicOr(&s_nearmask[e >> 5], 1u << (e & 31));
            }
        }
    }
    __syncthreads();
    if constexpr (DST != CBD_PLAIN) {
        if (nm > 0) {
            const int nw = (nm + 31) / 32;
            for (int e = threadIdx.x; e < nm; e += blockDim.x) {
                const unsigned wbits = s_nearmask[e >> 5];
                if ((wbits >> (e & 31)) & 1u) {
                    int rank = __popc(wbits & ((1u << (e & 31)) - 1u));
                    for (int wd = 0; wd < (e >> 5); ++wd) rank += __popc(s_nearmask[wd]);
                    if (rank < kCbNear) {
                        const int4 m = e < 256 ? mym : A.miss[v * kCbMissCap + e];
                        s_mz[rank] = m.x; s_my[rank] = m.y; s_mx[rank] = m.z;
                    }
                }
            }
            if (threadIdx.x == 0) {
                int tot = 0;
                for (int wd = 0; wd < nw; ++wd) tot += __popc(s_nearmask[wd]);
                s_nn = (tot > kCbNear || (len + K - 1) / K > kCbBlkMax) ? kCbNear + 1 : tot;
            }
            if (threadIdx.x < 32 * NW) s_lmask[threadIdx.x] = 0ull;
            for (int i = threadIdx.x; i < ((len + K - 1) / K) * NW && i < kCbBlkMax * NW; i += blockDim.x) s_emask[i] = 0ull;
        }
    }
    // ---- halo: the chunk line reflected at the chunk's ends, zeros where that leaves the box ----
    for (int idx = threadIdx.x; idx < 2 * radius * T; idx += blockDim.x) {
        int h, line;
        if (PF) { line = idx / (2 * radius); h = idx - line * 2 * radius; }
        else { h = idx >> lt; line = idx & (T - 1); }
        const int p = (h < radius) ? (h - radius) : (len + h - radius);
        const int q = box_reflect(p, b0, len, full);
        sl[lidx(line, p + radius)] = (q >= 0) ? sl[lidx(line, q + radius)] : 0.f;
    }
    __syncthreads();
    if constexpr (DST != CBD_PLAIN) {
        const int nn = s_nn;
        if (nn > 0 && nn <= kCbNear) {
            for (int i = threadIdx.x; i < nn * T; i += blockDim.x) {
                const int r = i >> lt, line = i & (T - 1);
                float w = 0.f;
                if (line < nl) {
                    const long long l = l0 + line;
                    const int rz = (int)(l / V.nyr);
                    const int bz = V.zr0 + rz, by = V.yr0 + (int)(l - (long long)rz * V.nyr);
                    const float wz = A.ndim == 3 ? cb_axis_weight_lds(bz, s_mz[r], V.lo[0], A.S.nz, radius, s_fwx) : (bz == s_mz[r] ? 1.f : 0.f);
                    w = wz * cb_axis_weight_lds(by, s_my[r], V.lo[1], A.S.ny, radius, s_fwx);
                }
                s_wzy[i] = w;
                if (w != 0.f) atomicOr(&s_lmask[line * NW + (r >> 6)], 1ull << (r & 63));
            }
            const int nblk_ = (len + K - 1) / K;
            for (int i = threadIdx.x; i < nn * nblk_; i += blockDim.x) {
                const int r = i / nblk_, blk = i - r * nblk_;
                const int mx = s_mx[r];
                if (cb_axis_reach(blk * K, blk * K + K - 1, mx, V.lo[2], A.S.nx, radius, true)) atomicOr(&s_emask[blk * NW + (r >> 6)], 1ull << (r & 63));
            }
        }
        __syncthreads();
    }
    // ---- filter: K consecutive outputs of one line per thread; pair j of output k needs the samples k - j and k + j, two windows
    // of K samples that slide by one in opposite directions as j falls (rotating registers, one new LDS sample per window and pair).
    // Row m (relative to the thread's first row p0 = K * blk; m is uniform over the workgroup) sits at base + off(m). ----
    const ACC* fw;
    if constexpr (std::is_same<ACC, float>::value) fw = A.fwf; else fw = A.fwd;
    const int nblk = (len + K - 1) / K;
    auto off = [&](int m) { return PF ? (m & 7) * S8 + (m >> 3) : m * TP; };
    for (int idx = threadIdx.x; idx < T * nblk; idx += blockDim.x) {
        int blk, line;
        if (PF) { line = idx / nblk; blk = idx - line * nblk; }
        else { blk = idx >> lt; line = idx & (T - 1); }
        if (line >= nl) continue;
        const int p0 = blk * K;
        const float* c = sl + (PF ? line * LP + blk : line + p0 * TP);      // row p0 + m: c[off(m)]
        // (last pass of a filter: what the quotient needs from memory -- the view at the 8 outputs, the tables -- is requested
        // before the taps, not after them)
        float av[K];
        if constexpr (DST != CBD_PLAIN && MVS_CBF_PREFETCH) {
            const float* Iv = A.I + V.off + lbase[line] + p0;
            if (p0 + K <= len) {
                const cb_f4u_t a0 = reinterpret_cast<const cb_f4u_t*>(Iv)[0], a1 = reinterpret_cast<const cb_f4u_t*>(Iv)[1];
                av[0] = a0.x; av[1] = a0.y; av[2] = a0.z; av[3] = a0.w; av[4] = a1.x; av[5] = a1.y; av[6] = a1.z; av[7] = a1.w;
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k) av[k] = (p0 + k < len) ? Iv[k] : NAN;
            }
        }
        // (float32: NA independent accumulators -- pair j goes to accumulator j mod NA -- so that a sum is NA chains of radius / NA
        // roundings instead of one of radius; C3 at size: one-count flips 0.24 % with one chain)
        constexpr int NA = std::is_same<ACC, float>::value ? MVS_CBF_NACC : 1;
        ACC PA[K], PB[K], accs[NA][K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            PA[k] = (ACC)c[off(k)];
            PB[k] = (ACC)c[off(k + 2 * radius)];
#pragma unroll
            for (int a = 0; a < NA; ++a) accs[a][k] = (ACC)0;
        }
        int ma = K, mb = 2 * radius - 1;      // next rows of the two windows
        int jb = radius;
        for (; jb >= K; jb -= K) {
            ACC w[K];
#pragma unroll
            for (int s = 0; s < K; ++s) w[s] = fw[radius - jb + s];
#pragma unroll
            for (int s = 0; s < K; ++s) {
#pragma unroll
                for (int k = 0; k < K; ++k) accs[s % NA][k] = fma(PA[(k + s) % K] + PB[(k - s + K) % K], w[s], accs[s % NA][k]);
                PA[s] = (ACC)c[off(ma + s)];
                PB[K - 1 - s] = (ACC)c[off(mb - s)];
            }
            ma += K;
            mb -= K;
        }
#pragma unroll
        for (int s = 0; s < K - 1; ++s) {                // the remaining jb < K pairs
            if (s >= jb) break;
            const ACC w = fw[radius - jb + s];
#pragma unroll
            for (int k = 0; k < K; ++k) accs[s % NA][k] = fma(PA[(k + s) % K] + PB[(k - s + K) % K], w, accs[s % NA][k]);
            PA[s] = (ACC)c[off(ma + s)];
            PB[K - 1 - s] = (ACC)c[off(mb - s)];
        }
        const ACC wc = fw[radius];
        float res[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            ACC acc = accs[0][k];
            if constexpr (NA == 2) acc += accs[1][k];
            if constexpr (NA == 4) acc = (acc + accs[1][k]) + (accs[2][k] + accs[3][k]);
            res[k] = (float)fma((ACC)c[off(k + radius)], wc, acc);
        }
        const long long obase = lbase[line] + (long long)p0 * stride;
        if constexpr (DST == CBD_PLAIN) {
            if (PF && p0 + K <= len) {
                cb_f4u_t* o4 = reinterpret_cast<cb_f4u_t*>(dst + obase);
                cb_f4u_t r0, r1;
                r0.x = res[0]; r0.y = res[1]; r0.z = res[2]; r0.w = res[3];
                r1.x = res[4]; r1.y = res[5]; r1.z = res[6]; r1.w = res[7];
                o4[0] = r0;
                o4[1] = r1;
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (p0 + k < len) dst[obase + (long long)k * stride] = res[k];
            }
        } else {
            // (x pass: line = (z, y) of the box)  WW = gaussian(mask) from the tables minus the listed voxels; Z = VV / WW where the
            // view is valid (weights.py:314-320); CBD_SQ: (A - Z)^2 with NaN -> 0; CBD_F: Z, NaN where A is NaN
            const long long l = l0 + line;
            const int rz = (int)(l / V.nyr);
            const int bz = V.zr0 + rz, by = V.yr0 + (int)(l - (long long)rz * V.nyr);
            const double* G = A.tabs + V.tab0 + (long long)A.filt * (nz + ny + nx);
            const double gzy = G[bz] * G[nz + by];
            float corr[K];      // (the bumps are <= 1e-2 of WW: their float32 sum is exact to 1e-9 of it)
#pragma unroll
            for (int k = 0; k < K; ++k) corr[k] = 0.f;
            const int nn = s_nn;
            if (nn > 0 && nn <= kCbNear) {
                for (int half = 0; half < NW; ++half) {
                unsigned long long bits = s_lmask[line * NW + half] & s_emask[blk * NW + half];
                while (bits) {
                    const int r = half * 64 + __ffsll((long long)bits) - 1;
                    bits &= bits - 1;
                    const float w = s_wzy[(r << lt) + line];
                    const int mx = s_mx[r];
#pragma unroll
                    for (int k = 0; k < K; ++k) corr[k] += w * cb_axis_weight_lds(p0 + k, mx, V.lo[2], A.S.nx, radius, s_fwx);
                }
                }
            } else if (nn > kCbNear) {
                for (int wd = 0; wd < (nm + 31) / 32; ++wd) {
                    unsigned bits = s_nearmask[wd];
                    while (bits) {
                        const int e = wd * 32 + __ffs((int)bits) - 1;
                        bits &= bits - 1;
                        const int4 m = A.miss[v * kCbMissCap + e];
                        // (most blocks of a line the voxel reaches in z and y are out of its reach along x)
                        if (!cb_axis_reach(p0, p0 + K - 1, m.z, V.lo[2], A.S.nx, radius, true)) continue;
                        const double wzy = cb_axis_weight(bz, m.x, V.lo[0], A.S.nz, radius, A.fwd, A.ndim == 3) *
                                           cb_axis_weight(by, m.y, V.lo[1], A.S.ny, radius, A.fwd, true);
                        if (wzy != 0.0) {
#pragma unroll
                            for (int k = 0; k < K; ++k) corr[k] += (float)(wzy * cb_axis_weight(p0 + k, m.z, V.lo[2], A.S.nx, radius, A.fwd, true));
                        }
                    }
                }
            }
            const bool whole = p0 + K <= len;
            if constexpr (!MVS_CBF_PREFETCH) {
                const float* Iv = A.I + V.off + obase;
                if (whole) {
                    const cb_f4u_t a0 = reinterpret_cast<const cb_f4u_t*>(Iv)[0], a1 = reinterpret_cast<const cb_f4u_t*>(Iv)[1];
                    av[0] = a0.x; av[1] = a0.y; av[2] = a0.z; av[3] = a0.w; av[4] = a1.x; av[5] = a1.y; av[6] = a1.z; av[7] = a1.w;
                } else {
#pragma unroll
                    for (int k = 0; k < K; ++k) av[k] = (p0 + k < len) ? Iv[k] : NAN;
                }
            }
            float ov[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float a = av[k];
                const float WW = (float)(gzy * G[nz + ny + min(p0 + k, len - 1)] - (double)corr[k]);
                float o;
                if constexpr (DST == CBD_SQ) {
                    o = 0.f;
                    if (a == a) {
                        const float d = a - res[k] / WW;      // (IEEE division: the quotient is subtracted from the view)
                        const float qd = d * d;
                        o = (qd == qd) ? qd : 0.f;
                    }
                } else {
                    o = (a == a) ? res[k] / WW : NAN;
                }
                ov[k] = o;
            }
            if (whole) {
                cb_f4u_t r0, r1;
                r0.x = ov[0]; r0.y = ov[1]; r0.z = ov[2]; r0.w = ov[3];
                r1.x = ov[4]; r1.y = ov[5]; r1.z = ov[6]; r1.w = ov[7];
                reinterpret_cast<cb_f4u_t*>(dst + obase)[0] = r0;
                reinterpret_cast<cb_f4u_t*>(dst + obase)[1] = r1;
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (p0 + k < len) dst[obase + k] = ov[k];
            }
        }
    }
}

// ---- mask_normalize8_kernel / cb_fuse8_kernel of the exact path spend their time testing 8 boxes per voxel (~150 instructions for 12
// bytes); here a thread owns R consecutive voxels of a row: the z / y tests and the row's index are worked out once per view and run ----
__global__ __launch_bounds__(256) void cb_normalize8_runs_kernel(float* __restrict__ bw, float* __restrict__ im, CbBoxes8 BX, int nviews, Shape3 S) {
    const int runs_x = (S.nx + kCbRun - 1) / kCbRun;
    const long long nruns = (long long)S.nz * S.ny * runs_x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nruns; i += (long long)gridDim.x * blockDim.x) {
        const int x0 = (int)(i % runs_x) * kCbRun;
        const long long t = i / runs_x;
        const int y = (int)(t % S.ny), z = (int)(t / S.ny);
        float w[8][kCbRun];
        int base[8];
        float wsum[kCbRun];
#pragma unroll
        for (int r = 0; r < kCbRun; ++r) wsum[r] = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            base[v] = -1;
#pragma unroll
            for (int r = 0; r < kCbRun; ++r) w[v][r] = 0.f;
            if (v >= nviews) continue;
            const CbBox32& B = BX.b[v];
            const int bz = z - B.lo[0], by = y - B.lo[1], bx0 = x0 - B.lo[2];
            if ((unsigned)bz >= (unsigned)B.n[0] || (unsigned)by >= (unsigned)B.n[1] || bx0 + kCbRun <= 0 || bx0 >= B.n[2]) continue;
            base[v] = B.off + (bz * B.n[1] + by) * B.n[2] + bx0;      // (may point before the row's first voxel: only in-range r are touched)
#pragma unroll
            for (int r = 0; r < kCbRun; ++r) {
                if ((unsigned)(bx0 + r) < (unsigned)B.n[2] && x0 + r < S.nx) {
                    float ww = bw[base[v] + r];
                    const float xv = im[base[v] + r];
                    if (xv != xv) ww = 0.f;
                    w[v][r] = ww;
                    wsum[r] += ww;      // (view order, float32: np.nansum over axis 0)
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kCbRun; ++r)
            if (wsum[r] == 0.f) wsum[r] = 1.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            if (base[v] == -1) continue;
            const CbBox32& B = BX.b[v];
            const int bx0 = x0 - B.lo[2];
#pragma unroll
            for (int r = 0; r < kCbRun; ++r)
                if ((unsigned)(bx0 + r) < (unsigned)B.n[2] && x0 + r < S.nx) {
                    const float wn = w[v][r] / wsum[r];
                    bw[base[v] + r] = wn;
                    if (wn < 1e-7f) im[base[v] + r] = NAN;
                }
        }
    }
}

template <typename TOut>
__global__ __launch_bounds__(256) void cb_fuse8_runs_kernel(const float* __restrict__ im, const float* __restrict__ bw, const float* __restrict__ F,
                                                            CbBoxes8 BX, int nviews, int tz, int ty, int tx, Shape3 O, TOut* __restrict__ out) {
    const int runs_x = (O.nx + kCbRun - 1) / kCbRun;
    const long long nruns = (long long)O.nz * O.ny * runs_x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nruns; i += (long long)gridDim.x * blockDim.x) {
        const int x0 = (int)(i % runs_x) * kCbRun;
        const long long t = i / runs_x;
        const int y = (int)(t % O.ny), z = (int)(t / O.ny);
        float f[8][kCbRun], a[8][kCbRun];
        int base[8];
        float fsum[kCbRun], asum[kCbRun], acc[kCbRun];
#pragma unroll
        for (int r = 0; r < kCbRun; ++r) { fsum[r] = 0.f; asum[r] = 0.f; acc[r] = 0.f; }
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            base[v] = -1;
#pragma unroll
            for (int r = 0; r < kCbRun; ++r) { f[v][r] = NAN; a[v][r] = 0.f; }
            if (v >= nviews) continue;
            const CbBox32& B = BX.b[v];
            const int bz = z + tz - B.lo[0], by = y + ty - B.lo[1], bx0 = x0 + tx - B.lo[2];
            if ((unsigned)bz >= (unsigned)B.n[0] || (unsigned)by >= (unsigned)B.n[1] || bx0 + kCbRun <= 0 || bx0 >= B.n[2]) continue;
            base[v] = B.off + (bz * B.n[1] + by) * B.n[2] + bx0;
#pragma unroll
            for (int r = 0; r < kCbRun; ++r)
                if ((unsigned)(bx0 + r) < (unsigned)B.n[2]) {
                    f[v][r] = F[base[v] + r];
                    if (f[v][r] == f[v][r]) fsum[r] += f[v][r];
                }
        }
#pragma unroll
        for (int r = 0; r < kCbRun; ++r)
            if (fsum[r] == 0.f) fsum[r] = 1.f;
        // (a view that does not hold the voxel is NaN there: f NaN -> every term it would add is skipped, like the reference's nansum)
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            if (base[v] == -1) continue;
            const int bx0 = x0 + tx - BX.b[v].lo[2];
#pragma unroll
            for (int r = 0; r < kCbRun; ++r)
                if ((unsigned)(bx0 + r) < (unsigned)BX.b[v].n[2]) {
                    a[v][r] = bw[base[v] + r] * (f[v][r] / fsum[r]);
                    if (a[v][r] == a[v][r]) asum[r] += a[v][r];
                }
        }
#pragma unroll
        for (int r = 0; r < kCbRun; ++r)
            if (asum[r] == 0.f) asum[r] = 1.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            if (base[v] == -1) continue;
            const int bx0 = x0 + tx - BX.b[v].lo[2];
#pragma unroll
            for (int r = 0; r < kCbRun; ++r)
                if ((unsigned)(bx0 + r) < (unsigned)BX.b[v].n[2]) {
                    const float p = im[base[v] + r] * (a[v][r] / asum[r]);
                    if (p == p) acc[r] += p;
                }
        }
        const long long o = ((long long)z * O.ny + y) * O.nx + x0;
#pragma unroll
        for (int r = 0; r < kCbRun; ++r)
            if (x0 + r < O.nx) {
                float q = acc[r];
                if (!(fabsf(q) <= 3.4028234e38f)) q = 0.f;
                out[o + r] = cast_cb<TOut>(q);
            }
    }
}
