// mvs_masks.hip -- sample masks and mask-driven pair selection (masks.py) on gfx950: the histogram of a whole acquisition for its one
// Otsu threshold (mvs_tile_histogram), the thresholded and box-dilated uint8 mask of a tile (mvs_mask_threshold), the fusion of the
// label images mask_i * (i + 1) by their minimum at order 0 (mvs_label_fuse) and the count of touching label pairs
// (mvs_label_contacts).  They replace registration.get_pairs_from_sample_masks (registration.py:3256-3292) and
// mv_graph.get_connected_labels (mv_graph.py:895-931) of the reference.  Every result is an integer or a selection: integer atomics
// only, equal inputs give equal bits.  Limits and launch geometry: mvs_masks_plan.h.
#include "mvs_internal.h"
#include "mvs_fold_dev.h"
#include "mvs_fuse_dev.h"
#include "mvs_masks_plan.h"
#include "mvs_sample_dev.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

namespace {

using namespace mvs_masks_plan;
static_assert(kMaxBins == MVS_HIST_MAX_BINS && kMaxDilate == MVS_MASK_MAX_DILATE && kMaxLabels == MVS_LABEL_MAX, "limits of mvs_hip.h and mvs_masks_plan.h differ");

// ---- shared device pieces -----------------------------------------------------------------------------------------------------------
// Sum of `v` over the workgroup, added to *dst (if any) by one integer atomic.
__device__ __forceinline__ void block_add_u64(unsigned long long v, unsigned long long* dst) {
    const unsigned long long sum = mvs_fold::block_fold<kWaves>(mvs_fold::Sums<unsigned long long>{{v}}).v[0];
    if (threadIdx.x == 0 && dst && sum) atomicAdd(dst, sum);
}

// The nx elements of a row at p, shared among the 64 lanes of a wave: 16-byte loads from the row's first 16-byte aligned element on,
// a scalar head before it and a scalar tail.  (p is aligned to its element type: checked by the entry points.)
template <typename T, typename F>
__device__ __forceinline__ void visit_row(const T* p, int nx, int lane, F&& f) {
    constexpr int V = 16 / (int)sizeof(T);
    struct alignas(16) Word { T v[V]; };
    int head = (int)(((16u - (unsigned)((unsigned long long)p & 15u)) & 15u) / (unsigned)sizeof(T));
    if (head > nx) head = nx;
    const int nvec = (nx - head) / V, tail = head + nvec * V;
    for (int x = lane; x < head; x += 64) f(p[x]);
    for (int j = lane; j < nvec; j += 64) {
        const Word w = *(const Word*)(p + head + j * V);
#pragma unroll
        for (int k = 0; k < V; ++k) f(w.v[k]);
    }
    for (int x = tail + lane; x < nx; x += 64) f(p[x]);
}

// ---- histogram ------------------------------------------------------------------------------------------------------------------------
struct HistTile {
    const char* data;
    long long sz, sy;           // bytes
    long long row0;             // rows (z, y) of the tiles before this one
    int ny, nx;
};

struct HistArgs {
    const HistTile* tiles;
    int n_tiles;
    long long total_rows;
};

typedef mvs_fold::Range<long long> RangePartial;

// row r of the stack of all tiles: its tile (binary search over row0) and its address
template <typename T>
__device__ __forceinline__ const T* hist_row(const HistArgs& P, long long r, int* nx) {
    int lo = 0, hi = P.n_tiles;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (P.tiles[mid].row0 <= r) lo = mid;
        else hi = mid;
    }
    const HistTile t = P.tiles[lo];
    const long long lr = r - t.row0;
    *nx = t.nx;
    return (const T*)(t.data + (lr / t.ny) * t.sz + (lr % t.ny) * t.sy);
}

// minimum, maximum and number of the non-NaN voxels a workgroup sees: one partial per workgroup ...
template <typename T>
__global__ __launch_bounds__(kThreads) void hist_range_kernel(HistArgs P, RangePartial* partials) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    RangePartial a{INFINITY, -INFINITY, 0};
    for (long long r = (long long)blockIdx.x * kWaves + wave; r < P.total_rows; r += (long long)gridDim.x * kWaves) {
        int nx;
        const T* p = hist_row<T>(P, r, &nx);
        visit_row<T>(p, nx, lane, [&](T raw) {
            const float v = (float)raw;
            if (v == v) a.merge({v, v, 1});
        });
    }
    a = mvs_fold::block_fold<kWaves>(a);
    if (threadIdx.x == 0) partials[blockIdx.x] = a;
}

// ... and one small launch that folds the partials
__global__ __launch_bounds__(kThreads) void hist_range_final_kernel(const RangePartial* partials, int n, RangePartial* out) {
    RangePartial a{INFINITY, -INFINITY, 0};
    for (int i = threadIdx.x; i < n; i += kThreads) a.merge(partials[i]);
    a = mvs_fold::block_fold<kWaves>(a);
    if (threadIdx.x == 0) *out = a;
}

// numpy's bin of v among n_bins equal bins over [edges[0], edges[n_bins]] (numpy/lib/_histograms_impl.py, the equal-bin path): the
// truncated (v - lo) / (hi - lo) * n_bins, n_bins folded into the last bin, then one step down or up against the edges themselves.
// -1: not counted (NaN, outside the range).
__device__ __forceinline__ int numpy_bin(double v, const double* __restrict__ edges, int n_bins, double lo, double hi) {
    if (!(v >= lo && v <= hi)) return -1;
    int k = (int)(((v - lo) / (hi - lo)) * (double)n_bins);
    k = min(max(k, 0), n_bins - 1);
    if (v < edges[k]) --k;
    else if (v >= edges[k + 1] && k != n_bins - 1) ++k;
    return min(max(k, 0), n_bins - 1);
}

// The counts of one workgroup's rows in uint32 bins in LDS (LDS integer atomics), flushed once with global uint64 integer atomics.
// (hist_blocks keeps the voxels of a workgroup below 2^32.)
template <typename T>
__global__ __launch_bounds__(kThreads) void hist_count_kernel(HistArgs P, const double* __restrict__ edges, int n_bins, unsigned long long* counts) {
    __shared__ unsigned int bins[kMaxBins];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = threadIdx.x; b < n_bins; b += kThreads) bins[b] = 0u;
    __syncthreads();
    const double lo = edges[0], hi = edges[n_bins];
    for (long long r = (long long)blockIdx.x * kWaves + wave; r < P.total_rows; r += (long long)gridDim.x * kWaves) {
        int nx;
        const T* p = hist_row<T>(P, r, &nx);
        visit_row<T>(p, nx, lane, [&](T raw) {
            const int k = numpy_bin((double)raw, edges, n_bins, lo, hi);
            if (k >= 0) atomicAdd(&bins[k], 1u);
        });
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_bins; b += kThreads)
        if (bins[b]) atomicAdd(&counts[b], (unsigned long long)bins[b]);
}

// ---- threshold and dilation ---------------------------------------------------------------------------------------------------------
struct MaskDims {
    int nz, ny, nx;
    long long groups;           // groups of kGroup voxels per row
    long long pitch;            // bytes per row of the work volumes: groups * kGroup
};

// where a pass writes: a work volume (rows of `pitch` bytes, always whole 16-byte stores, zeros past the row) or the result (rows of
// nx bytes)
struct MaskOut {
    unsigned char* data;
    long long pitch;
    int padded;
};

template <typename T> __device__ __forceinline__ bool above(T v, double thr, float thr_f) { return (double)v > thr; }
template <> __device__ __forceinline__ bool above<float>(float v, double thr, float thr_f) { return v > thr_f; }      // (a NaN is not)

// the first nvalid bytes of a group
__device__ __forceinline__ uint4 clip_group(uint4 m, int nvalid) {
    unsigned int w[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int nb = min(max(nvalid - 4 * d, 0), 4);
        w[d] &= nb == 4 ? 0xffffffffu : ((1u << (8 * nb)) - 1u);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// 16 mask bytes (0 / 1) <-> 16 bits
__device__ __forceinline__ unsigned int pack4(unsigned int d) { return (d & 1u) | ((d >> 7) & 2u) | ((d >> 14) & 4u) | ((d >> 21) & 8u); }
__device__ __forceinline__ unsigned int unpack4(unsigned int n) { return (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21); }
__device__ __forceinline__ unsigned int pack16(uint4 m) { return pack4(m.x) | (pack4(m.y) << 4) | (pack4(m.z) << 8) | (pack4(m.w) << 12); }
__device__ __forceinline__ uint4 unpack16(unsigned int b) { return make_uint4(unpack4(b), unpack4(b >> 4), unpack4(b >> 8), unpack4(b >> 12)); }

// Store the group at x0 of a row (m clipped to its nvalid voxels); returns the number of set voxels.
__device__ __forceinline__ int emit_group(uint4 m, const MaskOut& O, long long row, long long x0, int nvalid) {
    unsigned char* q = O.data + row * O.pitch + x0;
    if (O.padded || (nvalid == kGroup && ((unsigned long long)q & 15u) == 0)) {
        *(uint4*)q = m;
    } else {
        const unsigned int w[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
        for (int j = 0; j < kGroup; ++j)
            if (j < nvalid) q[j] = (unsigned char)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
    }
    return __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
}

// mask = v > threshold, one group of 16 voxels per lane: 16-byte loads where the group is whole and aligned, element by element otherwise
template <typename T>
__global__ __launch_bounds__(kThreads) void mask_threshold_kernel(const T* __restrict__ in, long long sz, long long sy, MaskDims D, double thr, MaskOut O,
                                                                  unsigned long long* count) {
    constexpr int V = 16 / (int)sizeof(T);
    struct alignas(16) Word { T v[V]; };
    const float thr_f = (float)thr;
    const long long items = (long long)D.nz * D.ny * D.groups;
    unsigned long long cnt = 0;
    for (long long item = (long long)blockIdx.x * kThreads + threadIdx.x; item < items; item += (long long)gridDim.x * kThreads) {
        const long long row = item / D.groups, x0 = (item % D.groups) * kGroup;
        const int nvalid = (int)min((long long)kGroup, D.nx - x0);
        const T* p = in + (row / D.ny) * sz + (row % D.ny) * sy + x0;
        unsigned int w[4] = {0u, 0u, 0u, 0u};
        if (nvalid == kGroup && ((unsigned long long)p & 15u) == 0) {
#pragma unroll
            for (int u = 0; u < kGroup / V; ++u) {
                const Word word = *(const Word*)(p + u * V);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int j = u * V + k;
                    if (above<T>(word.v[k], thr, thr_f)) w[j >> 2] |= 1u << (8 * (j & 3));
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < kGroup; ++j)
                if (j < nvalid && above<T>(p[j], thr, thr_f)) w[j >> 2] |= 1u << (8 * (j & 3));
        }
        cnt += (unsigned long long)emit_group(make_uint4(w[0], w[1], w[2], w[3]), O, row, x0, nvalid);
    }
    block_add_u64(cnt, count);
}

// 128 bits, of which the x pass uses 80
struct Bits128 {
    unsigned long long lo, hi;
};
__device__ __forceinline__ Bits128 bits_shr(Bits128 b, int s) {      // 0 <= s < 64
    if (s == 0) return b;
    return Bits128{(b.lo >> s) | (b.hi << (64 - s)), b.hi >> s};
}

// Running maximum of a flat box of 2 r + 1 voxels along x, 1 <= r <= kMaxDilate, zeros outside the row.  A lane takes one group of
// 16 voxels: the 16-byte groups g - 2 .. g + 2 of the work row as the bits of the positions x0 - 32 .. x0 + 47, the OR over a window
// of 2 r + 1 bits by doubling, and the 16 bits of its own group out of it.
__global__ __launch_bounds__(kThreads) void mask_dilate_x_kernel(const unsigned char* __restrict__ in, MaskDims D, int r, MaskOut O, unsigned long long* count) {
    const long long items = (long long)D.nz * D.ny * D.groups;
    const int L = 2 * r + 1;
    unsigned long long cnt = 0;
    for (long long item = (long long)blockIdx.x * kThreads + threadIdx.x; item < items; item += (long long)gridDim.x * kThreads) {
        const long long row = item / D.groups, g = item % D.groups;
        const unsigned char* line = in + row * D.pitch;
        unsigned long long part[5];
#pragma unroll
        for (int k = -2; k <= 2; ++k) {
            const long long gg = g + k;
            const bool need = gg >= 0 && gg < D.groups && ((k >= -1 && k <= 1) || r > kGroup);      // r <= 16 stays within g - 1 .. g + 1
            part[k + 2] = need ? (unsigned long long)pack16(*(const uint4*)(line + gg * kGroup)) : 0ull;
        }
        Bits128 w{part[0] | (part[1] << 16) | (part[2] << 32) | (part[3] << 48), part[4]};      // w(i) = OR of the bits i .. i + len - 1
        int len = 1;
        for (; len * 2 <= L; len *= 2) {
            const Bits128 s = bits_shr(w, len);
            w.lo |= s.lo;
            w.hi |= s.hi;
        }
        if (len < L) {
            const Bits128 s = bits_shr(w, L - len);
            w.lo |= s.lo;
            w.hi |= s.hi;
        }
        const unsigned int bits = (unsigned int)(bits_shr(w, 2 * kGroup - r).lo & 0xffffull);      // voxel x0 + j: window from bit 32 + j - r
        const long long x0 = g * kGroup;
        const int nvalid = (int)min((long long)kGroup, D.nx - x0);
        cnt += (unsigned long long)emit_group(clip_group(unpack16(bits), nvalid), O, row, x0, nvalid);
    }
    block_add_u64(cnt, count);
}

// The same along y (axis 1) or z (axis 0): the OR of the 16-byte groups of the 2 r + 1 rows or planes around a lane's own.
__global__ __launch_bounds__(kThreads) void mask_dilate_lines_kernel(const unsigned char* __restrict__ in, MaskDims D, int r, int axis, MaskOut O,
                                                                     unsigned long long* count) {
    const long long items = (long long)D.nz * D.ny * D.groups;
    const int n = axis ? D.ny : D.nz;
    const long long step = (axis ? 1LL : (long long)D.ny) * D.pitch;
    unsigned long long cnt = 0;
    for (long long item = (long long)blockIdx.x * kThreads + threadIdx.x; item < items; item += (long long)gridDim.x * kThreads) {
        const long long row = item / D.groups, x0 = (item % D.groups) * kGroup;
        const int at = axis ? (int)(row % D.ny) : (int)(row / D.ny);
        const unsigned char* p = in + row * D.pitch + x0;
        uint4 m = make_uint4(0u, 0u, 0u, 0u);
        for (int t = max(-r, -at); t <= min(r, n - 1 - at); ++t) {
            const uint4 v = *(const uint4*)(p + t * step);
            m.x |= v.x;
            m.y |= v.y;
            m.z |= v.z;
            m.w |= v.w;
        }
        const int nvalid = (int)min((long long)kGroup, D.nx - x0);
        cnt += (unsigned long long)emit_group(clip_group(m, nvalid), O, row, x0, nvalid);
    }
    block_add_u64(cnt, count);
}

// ---- label fuse ---------------------------------------------------------------------------------------------------------------------
constexpr int kBrickX = 64;      // voxels along x per brick (16 lanes x 4 voxels): the brick of the generic fuse kernel
constexpr int kVPT = 4;

struct LabelParams {
    const DevView* views;
    int nviews;
    int* out;
    int oz, oy, ox;
    int nbz, nby, nbx;     // brick grid
    int bz, by;            // brick extent along z and y: 4 x 4 (3D) or 1 x 16 (2D)
};

// out(p) = min over the views v whose order-0 sample at p is in bounds of (mask_v ? v + 1 : 0); 0 where there is none.  Bricks and
// the culling of views per brick are those of fuse_kernel (mvs_fuse.hip), coordinates and sample those of mvs_resample.
__global__ __launch_bounds__(kThreads) void label_fuse_kernel(LabelParams P) {
    __shared__ int s_act[64];
    __shared__ int s_nact;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.x;
    const int bx = b % P.nbx;
    b /= P.nbx;
    const int byi = b % P.nby, bzi = b / P.nby;
    const int lx = lane & 15, ly = lane >> 4;
    int z, y;
    if (P.bz == 4) {
        z = bzi * 4 + wave;
        y = byi * 4 + ly;
    } else {
        z = bzi;
        y = byi * 16 + wave * 4 + ly;
    }
    const int x0 = bx * kBrickX + lx * kVPT;
    const bool row_ok = (z < P.oz) && (y < P.oy) && (x0 < P.ox);
    const int lo[3] = {bzi * P.bz, byi * P.by, bx * kBrickX};
    const int hi[3] = {min(bzi * P.bz + P.bz, P.oz) - 1, min(byi * P.by + P.by, P.oy) - 1, min(bx * kBrickX + kBrickX, P.ox) - 1};
    const double pz = (double)z, py = (double)y, px0 = (double)x0;

    int best[kVPT];
#pragma unroll
    for (int j = 0; j < kVPT; ++j) best[j] = INT_MAX;

    for (int base = 0; base < P.nviews; base += 64) {
        __syncthreads();
        if (wave == 0) {
            const int v = base + lane;
            bool act = false;
            if (v < P.nviews) act = brick_hits_view(P.views[v], lo, hi);
            const unsigned long long mask = __ballot(act);
            if (act) s_act[__popcll(mask & ((1ull << lane) - 1ull))] = v;
            if (lane == 0) s_nact = __popcll(mask);
        }
        __syncthreads();
        const int nact = s_nact;
        if (!row_ok) continue;
        for (int a = 0; a < nact; ++a) {
            const int vi = __builtin_amdgcn_readfirstlane(s_act[a]);
            const DevView& V = P.views[vi];
            const double rz = pz * V.m[0] + py * V.m[1];
            const double ry = pz * V.m[3] + py * V.m[4];
            const double rx = pz * V.m[6] + py * V.m[7];
#pragma unroll
            for (int j = 0; j < kVPT; ++j) {
                const double px = px0 + (double)j;
                const double cz = (rz + px * V.m[2]) + V.off[0];
                const double cy = (ry + px * V.m[5]) + V.off[1];
                const double cx = (rx + px * V.m[8]) + V.off[2];
                if (!view_in_bounds(V, cz, cy, cx)) continue;
                const int label = sample_view<unsigned char, 0>(V, cz, cy, cx) != 0.f ? vi + 1 : 0;
                best[j] = min(best[j], label);
            }
        }
    }
    if (!row_ok) return;
#pragma unroll
    for (int j = 0; j < kVPT; ++j)
        if (best[j] == INT_MAX) best[j] = 0;
    int* q = P.out + ((long long)z * P.oy + y) * (long long)P.ox + x0;
    if (x0 + kVPT <= P.ox && ((unsigned long long)q & 15u) == 0) {
        *(int4*)q = make_int4(best[0], best[1], best[2], best[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kVPT; ++j)
            if (x0 + j < P.ox) q[j] = best[j];
    }
}

// ---- label contacts -----------------------------------------------------------------------------------------------------------------
struct ContactArgs {
    const int* labels;
    int nz, ny, nx;
    int n_labels, n_off;
    Offset off[kMaxOffsets];
    unsigned long long* counts;      // n_labels x n_labels
    long long chunks;                // chunks of 64 voxels per row
};

// A wave takes 64 consecutive voxels of a row; per offset of the half neighbourhood every lane forms the key of its pair
// (a, b) = (label(p), label(p + o)), both in 1 .. n_labels and different, as (min - 1) * n_labels + (max - 1) + 1, or 0.  Equal keys
// of consecutive lanes -- a run along the face between two tiles -- are combined: the first lane of a run adds its length.
__global__ __launch_bounds__(kThreads) void label_contacts_kernel(ContactArgs P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long items = (long long)P.nz * P.ny * P.chunks;
    for (long long item = (long long)blockIdx.x * kWaves + wave; item < items; item += (long long)gridDim.x * kWaves) {
        const long long row = item / P.chunks;
        const int z = (int)(row / P.ny), y = (int)(row % P.ny), x = (int)(item % P.chunks) * 64 + lane;
        int a = x < P.nx ? P.labels[row * P.nx + x] : 0;
        if (a < 0 || a > P.n_labels) a = 0;
        for (int k = 0; k < P.n_off; ++k) {
            const int qz = z + P.off[k].dz, qy = y + P.off[k].dy, qx = x + P.off[k].dx;
            const bool ok = a > 0 && qz >= 0 && qz < P.nz && qy >= 0 && qy < P.ny && qx >= 0 && qx < P.nx;
            int bl = ok ? P.labels[((long long)qz * P.ny + qy) * P.nx + qx] : 0;
            if (bl < 0 || bl > P.n_labels) bl = 0;
            const unsigned int key = (bl > 0 && bl != a) ? (unsigned int)(min(a, bl) - 1) * (unsigned int)P.n_labels + (unsigned int)(max(a, bl) - 1) + 1u : 0u;
            const unsigned int prev = __shfl_up(key, 1);
            const bool head = lane == 0 || key != prev;
            const unsigned long long heads = __ballot(head);
            if (head && key) {
                const unsigned long long next = lane == 63 ? 0ull : heads >> (lane + 1);
                const int len = next ? __ffsll((long long)next) : 64 - lane;
                atomicAdd(&P.counts[key - 1u], (unsigned long long)len);
            }
        }
    }
}

// ---- host pieces --------------------------------------------------------------------------------------------------------------------
// What the entries require of a tile beyond mvs_check_tile_view: a shape in range, rows contiguous, the data aligned to its type.
int check_tile_layout(MvsContext* c, const char* what, const mvs_view_t& v, int i) {
    for (int k = 0; k < 3; ++k)
        if (v.shape[k] < 1 || v.shape[k] > 0x7fffffffLL) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: tile %d: shape[%d] out of range", what, i, k);
    if (v.stride[2] != 1) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: tile %d: the stride along x must be 1", what, i);
    if ((unsigned long long)v.data % mvs_dtype_size(v.dtype)) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: tile %d: data not aligned to its type", what, i);
    if (v.mem == MVS_MEM_HOST && (v.stride[1] != v.shape[2] || v.stride[0] != v.shape[1] * v.shape[2]))
        return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: tile %d: host tiles must be C-contiguous", what, i);
    return MVS_OK;
}

}  // namespace

extern "C" int mvs_tile_histogram(int device, const mvs_view_t* tiles, int32_t n_tiles, int32_t n_bins, const double* edges, uint64_t* counts_out,
                                  double* min_out, double* max_out, int64_t* n_valid_out) {
    const char* what = "mvs_tile_histogram";
    MvsContext* c0 = mvs_ctx(device);
    if (n_bins < 0) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: n_bins < 0", what);
    if (n_bins > MVS_HIST_MAX_BINS) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: n_bins %d exceeds %d", what, n_bins, MVS_HIST_MAX_BINS);
    if (!tiles || n_tiles < 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL/empty argument", what);
    if (n_bins == 0 && (!min_out || !max_out || !n_valid_out)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: n_bins == 0 needs min_out, max_out, n_valid_out", what);
    if (n_bins > 0 && (!edges || !counts_out)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: n_bins > 0 needs edges and counts_out", what);
    if (n_bins > 0 && !(edges[n_bins] > edges[0])) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: the range of the edges is empty", what);
    const int dtype = tiles[0].dtype;
    const size_t es = mvs_dtype_size(dtype);
    long long total_rows = 0, max_nx = 1;
    size_t host_bytes = 0;
    for (int i = 0; i < n_tiles; ++i) {
        const mvs_view_t& v = tiles[i];
        int rc = mvs_check_tile_view(c0, what, &v, 3);
        if (rc) return rc;
        if (v.dtype != dtype) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: the tiles must share one dtype (%d and %d given)", what, dtype, v.dtype);
        rc = check_tile_layout(c0, what, v, i);
        if (rc) return rc;
        if (v.shape[2] > (1LL << 29)) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: tile %d: rows of more than 2^29 voxels", what, i);
        total_rows += v.shape[0] * v.shape[1];
        max_nx = std::max<long long>(max_nx, v.shape[2]);
        if (v.mem == MVS_MEM_HOST) host_bytes += align_up((size_t)v.shape[0] * v.shape[1] * v.shape[2] * es);
    }
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    // host tiles are packed into one block for the duration of the call
    MvsWorkArea area(c);
    if (host_bytes) {
        rc = area.alloc(host_bytes);
        if (rc) return rc;
    }
    std::vector<HistTile> table((size_t)n_tiles);
    size_t cursor = 0;
    long long row0 = 0;
    for (int i = 0; i < n_tiles; ++i) {
        const mvs_view_t& v = tiles[i];
        HistTile& t = table[i];
        const void* dptr;
        rc = mvs_stage_view(c, v, es, (char*)area.ptr, &cursor, &dptr);
        if (rc) return rc;
        t.data = (const char*)dptr;
        t.sz = (v.mem == MVS_MEM_HOST ? v.shape[1] * v.shape[2] : v.stride[0]) * (long long)es;
        t.sy = (v.mem == MVS_MEM_HOST ? v.shape[2] : v.stride[1]) * (long long)es;
        t.row0 = row0;
        t.ny = (int)v.shape[1];
        t.nx = (int)v.shape[2];
        row0 += v.shape[0] * v.shape[1];
    }
    const long long nblocks_ll = hist_blocks(total_rows, max_nx);
    if (nblocks_ll > 0x7fffffffLL) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: too many voxels", what);
    const int nblocks = (int)nblocks_ll;
    const size_t table_bytes = align_up(sizeof(HistTile) * (size_t)n_tiles);
    const size_t edge_bytes = align_up(sizeof(double) * (size_t)(n_bins + 1));
    const size_t result_bytes = n_bins ? sizeof(unsigned long long) * (size_t)n_bins : sizeof(RangePartial) * (size_t)nblocks;
    char* small = (char*)mvs_scratch(c, 2, table_bytes + edge_bytes + result_bytes);
    if (!small) return mvs_alloc_failed(c);
    // (pageable sources: the copies have left the host buffers when they return)
    MVS_HIP_TRY(c, hipMemcpyAsync(small, table.data(), sizeof(HistTile) * (size_t)n_tiles, hipMemcpyHostToDevice, c->stream));
    HistArgs P{(const HistTile*)small, n_tiles, total_rows};
    double* d_edges = (double*)(small + table_bytes);
    char* d_result = small + table_bytes + edge_bytes;

    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    if (n_bins == 0) {
        void *mh, *md;
        rc = mvs_mailbox(c, sizeof(RangePartial), &mh, &md);
        if (rc) return rc;
        mvs_dispatch_dtype(dtype, [&](auto tag) {
            hipLaunchKernelGGL((hist_range_kernel<decltype(tag)>), dim3(nblocks), dim3(kThreads), 0, c->stream, P, (RangePartial*)d_result);
        });
        MVS_HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(hist_range_final_kernel, dim3(1), dim3(kThreads), 0, c->stream, (const RangePartial*)d_result, nblocks, (RangePartial*)md);
        MVS_HIP_TRY(c, hipGetLastError());
        MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
        c->timing_valid = true;
        MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
        const RangePartial r = *(const RangePartial*)mh;
        *n_valid_out = r.n;
        *min_out = r.n ? (double)r.mn : NAN;
        *max_out = r.n ? (double)r.mx : NAN;
    } else {
        MVS_HIP_TRY(c, hipMemcpyAsync(d_edges, edges, sizeof(double) * (size_t)(n_bins + 1), hipMemcpyHostToDevice, c->stream));
        MVS_HIP_TRY(c, hipMemsetAsync(d_result, 0, result_bytes, c->stream));
        mvs_dispatch_dtype(dtype, [&](auto tag) {
            hipLaunchKernelGGL((hist_count_kernel<decltype(tag)>), dim3(nblocks), dim3(kThreads), 0, c->stream, P, (const double*)d_edges, (int)n_bins,
                               (unsigned long long*)d_result);
        });
        MVS_HIP_TRY(c, hipGetLastError());
        MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
        c->timing_valid = true;
        MVS_HIP_TRY(c, hipMemcpyAsync(counts_out, d_result, result_bytes, hipMemcpyDeviceToHost, c->stream));
        MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return host_bytes ? area.release() : MVS_OK;
}

extern "C" int mvs_mask_threshold(int device, const mvs_view_t* tile, int32_t ndim, double threshold, const int32_t radius[3], void* mask_out,
                                  int64_t* n_set_out) {
    const char* what = "mvs_mask_threshold";
    MvsContext* c0 = mvs_ctx(device);
    if (!tile || !radius || !mask_out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", what);
    for (int k = 0; k < 3; ++k) {
        if (radius[k] < 0) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: radius[%d] < 0", what, k);
        if (radius[k] > MVS_MASK_MAX_DILATE) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: radius[%d] = %d exceeds %d", what, k, radius[k], MVS_MASK_MAX_DILATE);
    }
    int rc = mvs_check_tile_view(c0, what, tile, ndim);
    if (rc) return rc;
    if (tile->mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: the tile must be in device memory", what);
    rc = check_tile_layout(c0, what, *tile, 0);
    if (rc) return rc;
    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    MaskDims D;
    D.nz = (int)tile->shape[0]; D.ny = (int)tile->shape[1]; D.nx = (int)tile->shape[2];
    D.groups = row_groups(D.nx);
    D.pitch = padded_pitch(D.nx);
    const long long rows = (long long)D.nz * D.ny;
    const int extent[3] = {D.nz, D.ny, D.nx};
    // the passes after the threshold, x first: a box along an axis of one voxel changes nothing
    int pass_axis[3], n_pass = 0;
    for (int k = 2; k >= 0; --k)
        if (radius[k] > 0 && extent[k] > 1) pass_axis[n_pass++] = k;
    MvsWorkArea area(c);
    const size_t work_bytes = align_up((size_t)rows * (size_t)D.pitch);
    if (n_pass) {
        rc = area.alloc(work_bytes * (n_pass > 1 ? 2 : 1));
        if (rc) return rc;
    }
    unsigned long long* d_count = (unsigned long long*)mvs_scratch(c, 2, sizeof(unsigned long long));
    if (!d_count) return mvs_alloc_failed(c);
    MVS_HIP_TRY(c, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), c->stream));
    const MaskOut result{(unsigned char*)mask_out, (long long)D.nx, 0};
    const MaskOut work[2] = {MaskOut{(unsigned char*)area.ptr, D.pitch, 1}, MaskOut{(unsigned char*)area.ptr + work_bytes, D.pitch, 1}};
    const int nblocks = grid_blocks(rows * D.groups, kThreads);

    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    {
        const MaskOut O = n_pass ? work[0] : result;
        unsigned long long* cnt = n_pass ? nullptr : d_count;
        mvs_dispatch_dtype(tile->dtype, [&](auto tag) {
            using T = decltype(tag);
            hipLaunchKernelGGL((mask_threshold_kernel<T>), dim3(nblocks), dim3(kThreads), 0, c->stream, (const T*)tile->data, (long long)tile->stride[0],
                               (long long)tile->stride[1], D, threshold, O, cnt);
        });
        MVS_HIP_TRY(c, hipGetLastError());
    }
    for (int i = 0; i < n_pass; ++i) {
        const bool last = i == n_pass - 1;
        const unsigned char* src = work[i & 1].data;
        const MaskOut O = last ? result : work[(i + 1) & 1];
        unsigned long long* cnt = last ? d_count : nullptr;
        const int k = pass_axis[i];
        if (k == 2) hipLaunchKernelGGL(mask_dilate_x_kernel, dim3(nblocks), dim3(kThreads), 0, c->stream, src, D, (int)radius[2], O, cnt);
        else hipLaunchKernelGGL(mask_dilate_lines_kernel, dim3(nblocks), dim3(kThreads), 0, c->stream, src, D, (int)radius[k], k, O, cnt);
        MVS_HIP_TRY(c, hipGetLastError());
    }
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    unsigned long long n_set = 0;
    MVS_HIP_TRY(c, hipMemcpyAsync(&n_set, d_count, sizeof(n_set), hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n_set_out) *n_set_out = (int64_t)n_set;
    return n_pass ? area.release() : MVS_OK;
}

extern "C" int mvs_label_fuse(int device, const mvs_view_t* views, int32_t n_views, int32_t ndim, const int64_t out_shape[3], int32_t* out,
                              int32_t out_mem) {
    const char* what = "mvs_label_fuse";
    MvsContext* c0 = mvs_ctx(device);
    if (!views || n_views < 1 || !out_shape || !out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL/empty argument", what);
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", what);
    if (out_mem != MVS_MEM_HOST && out_mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: bad out_mem", what);
    for (int k = 0; k < 3; ++k)
        if (out_shape[k] < 1 || out_shape[k] > 0x7fffffffLL) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: out_shape[%d] out of range", what, k);
    if (ndim == 2 && out_shape[0] != 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: 2D grids have out_shape[0] == 1", what);
    for (int i = 0; i < n_views; ++i) {
        const int rc = mvs_check_tile_view(c0, what, &views[i], ndim);
        if (rc) return rc;
        if (views[i].dtype != MVS_U8) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: view %d: masks are uint8", what, i);
    }
    LabelParams P;
    P.nviews = n_views;
    P.oz = (int)out_shape[0]; P.oy = (int)out_shape[1]; P.ox = (int)out_shape[2];
    P.bz = ndim == 3 ? 4 : 1;
    P.by = ndim == 3 ? 4 : 16;
    P.nbz = (P.oz + P.bz - 1) / P.bz;
    P.nby = (P.oy + P.by - 1) / P.by;
    P.nbx = (P.ox + kBrickX - 1) / kBrickX;
    const long long nblocks = (long long)P.nbz * P.nby * P.nbx;
    if (nblocks > 0x7fffffffLL) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 bricks", what);
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    // one block: the view records, the host masks, a host result
    size_t mask_bytes = 0;
    rc = mvs_stage_views_bytes(c, views, n_views, 1, &mask_bytes);
    if (rc) return rc;
    const size_t rec_bytes = align_up(sizeof(DevView) * (size_t)n_views);
    const size_t out_bytes = sizeof(int32_t) * (size_t)out_shape[0] * (size_t)out_shape[1] * (size_t)out_shape[2];
    MvsWorkArea area(c);
    rc = area.alloc(rec_bytes + mask_bytes + (out_mem == MVS_MEM_HOST ? out_bytes : 0));
    if (rc) return rc;
    char* base = (char*)area.ptr;
    std::vector<DevView> recs((size_t)n_views);
    size_t cursor = 0;
    for (int i = 0; i < n_views; ++i) {
        const void* dptr;
        rc = mvs_stage_view(c, views[i], 1, base + rec_bytes, &cursor, &dptr);
        if (rc) return rc;
        rc = mvs_fill_dev_view(c, views[i], ndim, dptr, &recs[i]);
        if (rc) return rc;
        recs[i].tr_ok = 0;
    }
    MVS_HIP_TRY(c, hipMemcpyAsync(base, recs.data(), sizeof(DevView) * (size_t)n_views, hipMemcpyHostToDevice, c->stream));
    P.views = (const DevView*)base;
    P.out = out_mem == MVS_MEM_HOST ? (int*)(base + rec_bytes + mask_bytes) : (int*)out;

    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    hipLaunchKernelGGL(label_fuse_kernel, dim3((unsigned)nblocks), dim3(kThreads), 0, c->stream, P);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    if (out_mem == MVS_MEM_HOST) MVS_HIP_TRY(c, hipMemcpyAsync(out, P.out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the records and host masks were copied from pageable memory of this call)
    return area.release();
}

extern "C" int mvs_label_contacts(int device, const int32_t* labels, int32_t ndim, const int64_t shape[3], int32_t n_labels, int32_t connectivity,
                                  uint64_t* counts_out) {
    const char* what = "mvs_label_contacts";
    MvsContext* c0 = mvs_ctx(device);
    if (!labels || !shape || !counts_out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", what);
    if (n_labels < 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: n_labels < 1", what);
    if (n_labels > MVS_LABEL_MAX) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: n_labels %d exceeds %d", what, n_labels, MVS_LABEL_MAX);
    if (connectivity < 1 || connectivity > ndim) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: connectivity must be 1..ndim", what);
    for (int k = 0; k < 3; ++k)
        if (shape[k] < 1 || shape[k] > 0x7fffffffLL) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: shape[%d] out of range", what, k);
    if (ndim == 2 && shape[0] != 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: 2D volumes have shape[0] == 1", what);
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    ContactArgs P;
    P.labels = labels;
    P.nz = (int)shape[0]; P.ny = (int)shape[1]; P.nx = (int)shape[2];
    P.n_labels = n_labels;
    P.n_off = half_neighbourhood(ndim, connectivity, P.off);
    P.chunks = (P.nx + 63) / 64;
    const size_t bytes = sizeof(unsigned long long) * (size_t)n_labels * (size_t)n_labels;
    P.counts = (unsigned long long*)mvs_scratch(c, 1, bytes);
    if (!P.counts) return mvs_alloc_failed(c);
    MVS_HIP_TRY(c, hipMemsetAsync(P.counts, 0, bytes, c->stream));
    const int nblocks = grid_blocks((long long)P.nz * P.ny * P.chunks, kWaves);
    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    hipLaunchKernelGGL(label_contacts_kernel, dim3(nblocks), dim3(kThreads), 0, c->stream, P);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    MVS_HIP_TRY(c, hipMemcpyAsync(counts_out, P.counts, bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MVS_OK;
}
