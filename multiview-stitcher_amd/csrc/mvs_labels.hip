// mvs_labels.hip -- stitching per-tile segmentations (labels.py) on gfx950: the voxel count of every label of a tile
// (mvs_label_counts), the co-occurrence table of the labels of two overlapping tiles (mvs_label_pair_overlaps) and the fusion of
// int32 label tiles through per-view look-up tables, the interior-most view deciding (mvs_label_tiles_fuse).  The tiles are int32 by
// contract: mvs_view_t.dtype is not read.  Coordinates and the in-bounds rule are those of mvs_resample / mvs_label_fuse at order 0.
// Every result is an integer: integer atomics only, equal inputs give equal results (the triples of a table after sorting).  Limits,
// the table's key / hash / probe sequence and the launch geometry: mvs_labels_plan.h.
#include "mvs_internal.h"
#include "mvs_fold_dev.h"
#include "mvs_fuse_dev.h"
#include "mvs_labels_plan.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

using namespace mvs_labels_plan;
static_assert(kMaxCountCapacity == MVS_LABEL_COUNT_MAX_CAPACITY && kMaxPairCapacity == MVS_LABEL_PAIR_MAX_CAPACITY,
              "limits of mvs_hip.h and mvs_labels_plan.h differ");

// An int32 label tile as the kernels read it; m / off map an index of the walked grid to a pixel of the tile.
struct LabelTile {
    const int* data;
    long long sz, sy;      // elements
    int nz, ny, nx;
    int lut_len;           // fuse: entries of lut (lut == NULL: the identity)
    const int* lut;
    double m[9];
    double off[3];
};

// ---- shared device pieces -----------------------------------------------------------------------------------------------------------
// c = M p + off in the operation order of the sampler (mvs_sample_dev.h): ((M_k0 p_z + M_k1 p_y) + M_k2 p_x) + o_k, in float64; the
// file is compiled without contraction.
__device__ __forceinline__ void tile_coord(const LabelTile& V, double pz, double py, double px, double c[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = ((pz * V.m[3 * k] + py * V.m[3 * k + 1]) + px * V.m[3 * k + 2]) + V.off[k];
}

// the in-bounds rule of mvs_resample: 0 <= c <= n - 1 on every axis
__device__ __forceinline__ bool tile_in_bounds(const LabelTile& V, const double c[3]) {
    return !(c[0] < 0.0 || c[0] > (double)(V.nz - 1) || c[1] < 0.0 || c[1] > (double)(V.ny - 1) || c[2] < 0.0 || c[2] > (double)(V.nx - 1));
}

// the voxel of an in-bounds coordinate at order 0: floor(c + 0.5)
__device__ __forceinline__ int tile_label(const LabelTile& V, const double c[3]) {
    const int iz = (int)floor(c[0] + 0.5), iy = (int)floor(c[1] + 0.5), ix = (int)floor(c[2] + 0.5);
    return V.data[iz * V.sz + iy * V.sy + ix];
}

// Conservative: can any voxel of the index box lo .. hi (inclusive) land inside the tile?  (brick_hits_view of mvs_sample_dev.h on
// this file's record.)
__device__ __forceinline__ bool brick_hits_tile(const LabelTile& V, const int lo[3], const int hi[3]) {
    const int n[3] = {V.nz, V.ny, V.nx};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double cmin = V.off[d], cmax = V.off[d];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double a = V.m[d * 3 + k] * (double)lo[k], b = V.m[d * 3 + k] * (double)hi[k];
            cmin += fmin(a, b);
            cmax += fmax(a, b);
        }
        if (cmax < -1e-3 || cmin > (double)(n[d] - 1) + 1e-3) return false;
    }
    return true;
}

// Counting the keys of the 64 lanes of a wave, chunk after chunk.  Equal keys of consecutive lanes are a run: one shuffle and one
// ballot find the first lane of every run and its length (the scheme of mvs_label_contacts), and that lane alone calls add(key,
// length).  A chunk that is ONE run is not added at all: the wave carries its key and length in registers and goes on adding to
// them while the next chunks bring the same key -- background, or the inside of a large object -- so a uniform region costs one
// atomic per wave, not one per chunk.  `none` is the key of a lane that counts nothing.  Every lane of the wave calls count() and
// flush() together; carry_key / carry_n hold the same value in every lane.
template <typename K>
struct WaveCounter {
    K none, carry_key;
    unsigned long long carry_n = 0;
    int lane;
    __device__ __forceinline__ WaveCounter(K none_, int lane_) : none(none_), carry_key(none_), lane(lane_) {}

    template <typename Add>
    __device__ __forceinline__ void flush(Add&& add) {
        if (carry_n && lane == 0 && carry_key != none) add(carry_key, carry_n);
        carry_n = 0;
    }

    template <typename Add>
    __device__ __forceinline__ void count(K key, Add&& add) {
        const K prev = __shfl_up(key, 1);
        const bool head = lane == 0 || key != prev;
        const unsigned long long heads = __ballot(head);
        if (heads == 1ull) {      // the whole chunk is one run
            if (carry_n && carry_key == key) {
                carry_n += 64ull;
                return;
            }
            flush(add);
            carry_key = key;
            carry_n = 64ull;
            return;
        }
        flush(add);
        if (head && key != none) {
            const unsigned long long next = lane == 63 ? 0ull : heads >> (lane + 1);
            add(key, (unsigned long long)(next ? __ffsll((long long)next) : 64 - lane));
        }
    }
};

// ---- label counts -------------------------------------------------------------------------------------------------------------------
struct CountArgs {
    LabelTile T;
    long long chunks, items;         // chunks of 64 voxels per row; rows * chunks
    long long capacity;
    unsigned long long* counts;      // capacity
    int* max_label;
};

// The 64 voxels at p, one per lane (lanes >= n: 0).  A whole chunk on a 16-byte boundary is read by 16 lanes with one 16-byte load
// each and handed out by shuffles; the branch is the same for all lanes of the wave.
__device__ __forceinline__ int load_chunk(const int* p, int n, int lane) {
    if (n == 64 && ((unsigned long long)p & 15u) == 0) {
        int4 w = make_int4(0, 0, 0, 0);
        if (lane < 16) w = *(const int4*)(p + 4 * lane);
        const int src = lane >> 2, k = lane & 3;
        const int a = __shfl(w.x, src), b = __shfl(w.y, src), c = __shfl(w.z, src), d = __shfl(w.w, src);
        return k == 0 ? a : (k == 1 ? b : (k == 2 ? c : d));
    }
    return lane < n ? p[lane] : 0;
}

// n[l] of one tile: a wave takes 64 consecutive voxels of a row at a time, a contiguous range of such chunks in all.  A negative
// label counts as 0; a label >= capacity is not counted; the largest label seen goes to *max_label by one integer atomic per wave.
__global__ __launch_bounds__(kThreads) void label_counts_kernel(CountArgs P) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const long long per = chunks_per_wave(P.items, (long long)gridDim.x * kWaves);
    const long long first = wave * per, last = min(first + per, P.items);
    unsigned long long* counts = P.counts;
    auto add = [counts](int key, unsigned long long n) { atomicAdd(&counts[key], n); };
    WaveCounter<int> counter(-1, lane);
    int mx = 0;
    for (long long item = first; item < last; ++item) {
        const long long row = item / P.chunks;
        const int x0 = (int)(item % P.chunks) * 64;
        const int n = min(64, P.T.nx - x0);
        const int raw = load_chunk(P.T.data + (row / P.T.ny) * P.T.sz + (row % P.T.ny) * P.T.sy + x0, n, lane);
        const int label = max(raw, 0);
        mx = max(mx, label);      // (lanes >= n bring 0)
        counter.count(lane < n && (long long)label < P.capacity ? label : -1, add);
    }
    counter.flush(add);
    mx = mvs_fold::wave_fold(mvs_fold::Max<int>{mx}).v;
    if (lane == 0 && mx > 0) atomicMax(P.max_label, mx);
}

// ---- pair overlaps --------------------------------------------------------------------------------------------------------------------
struct PairArgs {
    const int* a;                    // tile a: the walked grid
    long long asz, asy;
    LabelTile B;                     // tile b; m / off: pixel of a -> pixel of b
    int lo[3], n[3];                 // the box of a that is walked
    long long chunks, items;
    unsigned long long* keys;        // the table: slots keys (kEmpty: free) ...
    unsigned long long* counts;      // ... and their counts
    unsigned long long slots;        // a power of two
    int* overflow;
};

// Add n to the count of `key`: open addressing, at most `slots` probes (probe_slot: every slot once).  A free slot is claimed by one
// compare-and-swap kEmpty -> key; whoever loses it to the same key shares the slot, whoever loses it to another key goes on.  A slot
// never changes once it holds a key, so a stale read of a key is still right and a stale read of kEmpty only costs the
// compare-and-swap, which answers with the slot's real content.  No lane waits for another one: with the table exhausted the voxels
// are dropped and *overflow raised.
__device__ __forceinline__ void table_add(unsigned long long* keys, unsigned long long* counts, unsigned long long slots, int* overflow,
                                          unsigned long long key, unsigned long long n) {
    const unsigned long long h = hash_key(key);
    for (unsigned long long i = 0; i < slots; ++i) {
        const unsigned long long s = (h + i) & (slots - 1ull);
        unsigned long long cur = keys[s];
        if (cur == kEmpty) {
            cur = atomicCAS(&keys[s], kEmpty, key);
            if (cur == kEmpty) cur = key;
        }
        if (cur == key) {
            atomicAdd(&counts[s], n);
            return;
        }
    }
    atomicOr(overflow, 1);
}

// The co-occurrence table of (a, b): every voxel p of the box of a, mapped into b; where b is in bounds and max(A[p], 0) |
// max(B[q], 0) is not 0 the pair counts one.  Chunks of 64 consecutive voxels of a row per wave, runs combined before the table.
__global__ __launch_bounds__(kThreads) void label_pairs_kernel(PairArgs P) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const long long per = chunks_per_wave(P.items, (long long)gridDim.x * kWaves);
    const long long first = wave * per, last = min(first + per, P.items);
    unsigned long long *keys = P.keys, *counts = P.counts;
    const unsigned long long slots = P.slots;
    int* overflow = P.overflow;
    auto add = [keys, counts, slots, overflow](unsigned long long key, unsigned long long n) { table_add(keys, counts, slots, overflow, key, n); };
    WaveCounter<unsigned long long> counter(kEmpty, lane);
    for (long long item = first; item < last; ++item) {
        const long long row = item / P.chunks;
        const int z = P.lo[0] + (int)(row / P.n[1]), y = P.lo[1] + (int)(row % P.n[1]);
        const int xl = (int)(item % P.chunks) * 64 + lane;
        const int x = P.lo[2] + xl;
        unsigned long long key = kEmpty;
        if (xl < P.n[2]) {
            double c[3];
            tile_coord(P.B, (double)z, (double)y, (double)x, c);
            if (tile_in_bounds(P.B, c)) {
                const int la = max(P.a[z * P.asz + y * P.asy + x], 0), lb = max(tile_label(P.B, c), 0);
                if (la | lb) key = pair_key(la, lb);
            }
        }
        counter.count(key, add);
    }
    counter.flush(add);
}

// The occupied slots as triples, in no defined order: a wave reserves room for its occupied slots with one integer atomic; triples
// beyond `capacity` are counted and not written.
__global__ __launch_bounds__(kThreads) void label_pairs_compact_kernel(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ counts,
                                                                       unsigned long long slots, unsigned long long capacity, int* la_out, int* lb_out,
                                                                       unsigned long long* n_out, unsigned long long* n_unique) {
    const int lane = threadIdx.x & 63;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kThreads; base < slots; base += (unsigned long long)gridDim.x * kThreads) {
        const unsigned long long s = base + threadIdx.x;      // (slots is a multiple of the workgroup: the loop is the same for all lanes)
        const unsigned long long key = s < slots ? keys[s] : kEmpty;
        const bool used = key != kEmpty;
        const unsigned long long mask = __ballot(used);
        if (!mask) continue;
        const int leader = __ffsll((long long)mask) - 1;
        unsigned long long at = 0;
        if (lane == leader) at = atomicAdd(n_unique, (unsigned long long)__popcll(mask));
        at = __shfl(at, leader) + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
        if (used && at < capacity) {
            la_out[at] = key_la(key);
            lb_out[at] = key_lb(key);
            n_out[at] = counts[s];
        }
    }
}

// ---- fuse ---------------------------------------------------------------------------------------------------------------------------
struct FuseArgs {
    const LabelTile* views;
    int nviews;
    int* out;
    int oz, oy, ox;        // the output box
    int org[3];            // index of its first voxel on the grid the views' m / off refer to
    int nbz, nby, nbx;     // brick grid
    int bz, by;            // brick extent along z and y: 4 x 4 (3D) or 1 x 16 (2D)
};

// out(p) = lut_w[L_w[q]] of the view w, among those in bounds at p, with the largest d = min over the axes with n_k > 1 of
// min(c_k, (n_k - 1) - c_k); ties go to the lowest view index (views are visited in ascending order, a later one wins only with a
// larger d); 0 where no view is in bounds, the label is negative or not below lut_len.  Bricks and the culling of views per brick
// are those of label_fuse_kernel (mvs_masks.hip).
__global__ __launch_bounds__(kThreads) void label_tiles_fuse_kernel(FuseArgs P) {
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
    const int lo[3] = {P.org[0] + bzi * P.bz, P.org[1] + byi * P.by, P.org[2] + bx * kBrickX};
    const int hi[3] = {P.org[0] + min(bzi * P.bz + P.bz, P.oz) - 1, P.org[1] + min(byi * P.by + P.by, P.oy) - 1,
                       P.org[2] + min(bx * kBrickX + kBrickX, P.ox) - 1};
    const double pz = (double)(P.org[0] + z), py = (double)(P.org[1] + y);

    int best_view[kVPT], best_label[kVPT];
    double best_d[kVPT];
#pragma unroll
    for (int j = 0; j < kVPT; ++j) {
        best_view[j] = -1;
        best_label[j] = 0;
        best_d[j] = -1.0;
    }

    for (int base = 0; base < P.nviews; base += 64) {
        __syncthreads();
        if (wave == 0) {
            const int v = base + lane;
            bool act = false;
            if (v < P.nviews) act = brick_hits_tile(P.views[v], lo, hi);
            const unsigned long long mask = __ballot(act);
            if (act) s_act[__popcll(mask & ((1ull << lane) - 1ull))] = v;
            if (lane == 0) s_nact = __popcll(mask);
        }
        __syncthreads();
        const int nact = s_nact;
        if (!row_ok) continue;
        for (int a = 0; a < nact; ++a) {
            const int vi = __builtin_amdgcn_readfirstlane(s_act[a]);
            const LabelTile& V = P.views[vi];
            const double nm[3] = {(double)(V.nz - 1), (double)(V.ny - 1), (double)(V.nx - 1)};
#pragma unroll
            for (int j = 0; j < kVPT; ++j) {
                double c[3];
                tile_coord(V, pz, py, (double)(P.org[2] + x0 + j), c);
                if (!tile_in_bounds(V, c)) continue;
                double d = INFINITY;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (nm[k] > 0.0) d = fmin(d, fmin(c[k], nm[k] - c[k]));
                if (d > best_d[j]) {
                    best_d[j] = d;
                    best_view[j] = vi;
                    best_label[j] = tile_label(V, c);
                }
            }
        }
    }
    if (!row_ok) return;
    int res[kVPT];
#pragma unroll
    for (int j = 0; j < kVPT; ++j) {
        res[j] = 0;
        if (best_view[j] < 0 || best_label[j] < 0) continue;
        const LabelTile& V = P.views[best_view[j]];
        if (!V.lut) res[j] = best_label[j];
        else if (best_label[j] < V.lut_len) res[j] = V.lut[best_label[j]];
    }
    int* q = P.out + ((long long)z * P.oy + y) * (long long)P.ox + x0;
    if (x0 + kVPT <= P.ox && ((unsigned long long)q & 15u) == 0) {
        *(int4*)q = make_int4(res[0], res[1], res[2], res[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kVPT; ++j)
            if (x0 + j < P.ox) q[j] = res[j];
    }
}

// ---- host pieces --------------------------------------------------------------------------------------------------------------------
// What the entries require of a label tile (dtype is not read: int32 by contract).
int check_label_tile(MvsContext* c, const char* what, const mvs_view_t* v, int ndim, int i) {
    if (!v->data) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: tile %d without data", what, i);
    if (v->mem != MVS_MEM_HOST && v->mem != MVS_MEM_DEVICE) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: tile %d: bad mem", what, i);
    for (int k = 0; k < 3; ++k)
        if (v->shape[k] < 1 || v->shape[k] > 0x7fffffffLL) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: tile %d: shape[%d] out of range", what, i, k);
    if (ndim == 2 && v->shape[0] != 1) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: tile %d: 2D tiles have shape[0] == 1", what, i);
    if (v->stride[2] != 1) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: tile %d: the stride along x must be 1", what, i);
    if (v->stride[0] < 0 || v->stride[1] < 0) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: tile %d: negative strides", what, i);
    if ((unsigned long long)v->data % sizeof(int32_t)) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: tile %d: data not aligned to int32", what, i);
    if (v->mem == MVS_MEM_HOST && (v->stride[1] != v->shape[2] || v->stride[0] != v->shape[1] * v->shape[2]))
        return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: tile %d: host tiles must be C-contiguous", what, i);
    return MVS_OK;
}

// The record of a checked tile that reads its voxels at dev_data (a staged host tile is C-contiguous).
LabelTile label_tile(const mvs_view_t& v, const void* dev_data) {
    LabelTile t{};
    t.data = (const int*)dev_data;
    t.sz = v.mem == MVS_MEM_HOST ? v.shape[1] * v.shape[2] : v.stride[0];
    t.sy = v.mem == MVS_MEM_HOST ? v.shape[2] : v.stride[1];
    t.nz = (int)v.shape[0];
    t.ny = (int)v.shape[1];
    t.nx = (int)v.shape[2];
    std::copy(v.matrix, v.matrix + 9, t.m);
    std::copy(v.offset, v.offset + 3, t.off);
    return t;
}

int check_ndim(MvsContext* c, const char* what, int ndim) {
    return ndim == 2 || ndim == 3 ? MVS_OK : mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", what);
}

}  // namespace

extern "C" int mvs_label_counts(int device, const mvs_view_t* tile, int32_t ndim, int64_t capacity, uint64_t* counts_out, int64_t* max_label_out) {
    const char* what = "mvs_label_counts";
    MvsContext* c0 = mvs_ctx(device);
    if (!tile || !counts_out || !max_label_out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    int rc = check_ndim(c0, what, ndim);
    if (rc) return rc;
    if (capacity < 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: capacity < 1", what);
    if (capacity > MVS_LABEL_COUNT_MAX_CAPACITY) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: capacity above 2^31", what);
    rc = check_label_tile(c0, what, tile, ndim, 0);
    if (rc) return rc;
    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    // one block: a host tile, the counts, the maximum
    size_t tile_bytes = 0;
    rc = mvs_stage_views_bytes(c, tile, 1, sizeof(int32_t), &tile_bytes);
    if (rc) return rc;
    const size_t count_bytes = sizeof(unsigned long long) * (size_t)capacity;
    MvsWorkArea area(c);
    rc = area.alloc(tile_bytes + align_up(count_bytes) + 256);
    if (rc) return rc;
    char* base = (char*)area.ptr;
    size_t cursor = 0;
    const void* dptr;
    rc = mvs_stage_view(c, *tile, sizeof(int32_t), base, &cursor, &dptr);
    if (rc) return rc;
    CountArgs P;
    P.T = label_tile(*tile, dptr);
    P.chunks = row_chunks(P.T.nx);
    P.items = (long long)P.T.nz * P.T.ny * P.chunks;
    P.capacity = capacity;
    P.counts = (unsigned long long*)(base + tile_bytes);
    P.max_label = (int*)(base + tile_bytes + align_up(count_bytes));
    MVS_HIP_TRY(c, hipMemsetAsync(P.counts, 0, align_up(count_bytes) + 256, c->stream));
    const int nblocks = grid_blocks(P.items, kWaves);
    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    hipLaunchKernelGGL(label_counts_kernel, dim3(nblocks), dim3(kThreads), 0, c->stream, P);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    int mx = 0;
    MVS_HIP_TRY(c, hipMemcpyAsync(counts_out, P.counts, count_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipMemcpyAsync(&mx, P.max_label, sizeof(mx), hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    *max_label_out = mx;
    return area.release();
}

extern "C" int mvs_label_pair_overlaps(int device, const mvs_view_t* a, const mvs_view_t* b, int32_t ndim, const int64_t box_lo[3],
                                       const int64_t box_n[3], int64_t capacity, int32_t* la_out, int32_t* lb_out, uint64_t* n_out,
                                       int64_t* n_unique_out) {
    const char* what = "mvs_label_pair_overlaps";
    MvsContext* c0 = mvs_ctx(device);
    if (!a || !b || !box_lo || !box_n || !la_out || !lb_out || !n_out || !n_unique_out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    int rc = check_ndim(c0, what, ndim);
    if (rc) return rc;
    if (capacity < 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: capacity < 1", what);
    if (capacity > MVS_LABEL_PAIR_MAX_CAPACITY) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: capacity above 2^27", what);
    const mvs_view_t* tiles[2] = {a, b};
    for (int i = 0; i < 2; ++i) {
        rc = check_label_tile(c0, what, tiles[i], ndim, i);
        if (rc) return rc;
    }
    if (!box_in_tile(box_lo, box_n, a->shape)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: the box is empty or not inside tile a", what);
    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    // one block: the host tiles, the table (keys, counts), the triples, the two words
    size_t tile_bytes = 0;
    for (int i = 0; i < 2; ++i) {
        size_t bytes = 0;
        rc = mvs_stage_views_bytes(c, tiles[i], 1, sizeof(int32_t), &bytes);
        if (rc) return rc;
        tile_bytes += bytes;
    }
    const size_t slots = (size_t)table_slots(capacity);
    const size_t slot_bytes = sizeof(unsigned long long) * slots;       // (a multiple of 256)
    const size_t la_bytes = align_up(sizeof(int32_t) * (size_t)capacity), n_bytes = align_up(sizeof(uint64_t) * (size_t)capacity);
    MvsWorkArea area(c);
    rc = area.alloc(tile_bytes + 2 * slot_bytes + 2 * la_bytes + n_bytes + 256);
    if (rc) return rc;
    char* base = (char*)area.ptr;
    size_t cursor = 0;
    const void* dptr[2];
    for (int i = 0; i < 2; ++i) {
        rc = mvs_stage_view(c, *tiles[i], sizeof(int32_t), base, &cursor, &dptr[i]);
        if (rc) return rc;
    }
    const LabelTile A = label_tile(*a, dptr[0]);
    PairArgs P;
    P.a = A.data;
    P.asz = A.sz;
    P.asy = A.sy;
    P.B = label_tile(*b, dptr[1]);
    for (int k = 0; k < 3; ++k) {
        P.lo[k] = (int)box_lo[k];
        P.n[k] = (int)box_n[k];
    }
    P.chunks = row_chunks(P.n[2]);
    P.items = (long long)P.n[0] * P.n[1] * P.chunks;
    char* at = base + tile_bytes;
    P.keys = (unsigned long long*)at;
    P.counts = (unsigned long long*)(at + slot_bytes);
    P.slots = slots;
    int* d_la = (int*)(at + 2 * slot_bytes);
    int* d_lb = (int*)(at + 2 * slot_bytes + la_bytes);
    unsigned long long* d_n = (unsigned long long*)(at + 2 * slot_bytes + 2 * la_bytes);
    unsigned long long* d_unique = (unsigned long long*)(at + 2 * slot_bytes + 2 * la_bytes + n_bytes);
    P.overflow = (int*)(d_unique + 1);
    MVS_HIP_TRY(c, hipMemsetAsync(P.keys, 0xff, slot_bytes, c->stream));      // kEmpty
    MVS_HIP_TRY(c, hipMemsetAsync(P.counts, 0, slot_bytes, c->stream));
    MVS_HIP_TRY(c, hipMemsetAsync(d_unique, 0, 256, c->stream));

    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    hipLaunchKernelGGL(label_pairs_kernel, dim3(grid_blocks(P.items, kWaves)), dim3(kThreads), 0, c->stream, P);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(label_pairs_compact_kernel, dim3(grid_blocks((long long)slots, kThreads)), dim3(kThreads), 0, c->stream,
                       (const unsigned long long*)P.keys, (const unsigned long long*)P.counts, (unsigned long long)slots, (unsigned long long)capacity, d_la,
                       d_lb, d_n, d_unique);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    unsigned long long words[2] = {0, 0};      // n_unique; the overflow flag in the low half of the second
    MVS_HIP_TRY(c, hipMemcpyAsync(words, d_unique, sizeof(words), hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const bool overflow = (words[1] & 0xffffffffull) != 0;
    const size_t n_got = (size_t)std::min<unsigned long long>(words[0], (unsigned long long)capacity);
    if (n_got) {
        MVS_HIP_TRY(c, hipMemcpyAsync(la_out, d_la, sizeof(int32_t) * n_got, hipMemcpyDeviceToHost, c->stream));
        MVS_HIP_TRY(c, hipMemcpyAsync(lb_out, d_lb, sizeof(int32_t) * n_got, hipMemcpyDeviceToHost, c->stream));
        MVS_HIP_TRY(c, hipMemcpyAsync(n_out, d_n, sizeof(uint64_t) * n_got, hipMemcpyDeviceToHost, c->stream));
        MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    *n_unique_out = (int64_t)words[0];
    rc = area.release();
    if (rc) return rc;
    return (overflow || words[0] > (unsigned long long)capacity) ? MVS_LABEL_INCOMPLETE : MVS_OK;
}

extern "C" int mvs_label_tiles_fuse(int device, const mvs_view_t* views, int32_t n_views, int32_t ndim, const int32_t* const* luts,
                                    const int64_t* lut_len, const int64_t out_shape[3], const int64_t index_origin[3], int32_t* out, int32_t out_mem) {
    const char* what = "mvs_label_tiles_fuse";
    MvsContext* c0 = mvs_ctx(device);
    if (!views || n_views < 1 || !out_shape || !out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL/empty argument", what);
    int rc = check_ndim(c0, what, ndim);
    if (rc) return rc;
    if (out_mem != MVS_MEM_HOST && out_mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: bad out_mem", what);
    if (luts && !lut_len) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: luts without lut_len", what);
    for (int k = 0; k < 3; ++k) {
        const int64_t org = index_origin ? index_origin[k] : 0;
        if (out_shape[k] < 1 || out_shape[k] > 0x7fffffffLL) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: out_shape[%d] out of range", what, k);
        if (org < -0x40000000LL || org > 0x7fffffffLL - out_shape[k]) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: index_origin[%d] out of range", what, k);
    }
    if (ndim == 2 && out_shape[0] != 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: 2D grids have out_shape[0] == 1", what);
    for (int i = 0; i < n_views; ++i) {
        rc = check_label_tile(c0, what, &views[i], ndim, i);
        if (rc) return rc;
        if (luts && luts[i] && (lut_len[i] < 1 || lut_len[i] > 0x7fffffffLL)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: lut_len[%d] out of range", what, i);
    }
    FuseArgs P;
    P.nviews = n_views;
    P.oz = (int)out_shape[0]; P.oy = (int)out_shape[1]; P.ox = (int)out_shape[2];
    for (int k = 0; k < 3; ++k) P.org[k] = index_origin ? (int)index_origin[k] : 0;
    P.bz = ndim == 3 ? 4 : 1;
    P.by = ndim == 3 ? 4 : 16;
    P.nbz = (P.oz + P.bz - 1) / P.bz;
    P.nby = (P.oy + P.by - 1) / P.by;
    P.nbx = (P.ox + kBrickX - 1) / kBrickX;
    const long long nblocks = (long long)P.nbz * P.nby * P.nbx;
    if (nblocks > 0x7fffffffLL) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 bricks", what);
    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    // one block: the tile records, the host tiles, a host result
    size_t tile_bytes = 0;
    rc = mvs_stage_views_bytes(c, views, n_views, sizeof(int32_t), &tile_bytes);
    if (rc) return rc;
    const size_t rec_bytes = align_up(sizeof(LabelTile) * (size_t)n_views);
    const size_t out_bytes = sizeof(int32_t) * (size_t)out_shape[0] * (size_t)out_shape[1] * (size_t)out_shape[2];
    MvsWorkArea area(c);
    rc = area.alloc(rec_bytes + tile_bytes + (out_mem == MVS_MEM_HOST ? out_bytes : 0));
    if (rc) return rc;
    char* base = (char*)area.ptr;
    std::vector<LabelTile> recs((size_t)n_views);
    size_t cursor = 0;
    for (int i = 0; i < n_views; ++i) {
        const void* dptr;
        rc = mvs_stage_view(c, views[i], sizeof(int32_t), base + rec_bytes, &cursor, &dptr);
        if (rc) return rc;
        recs[i] = label_tile(views[i], dptr);
        recs[i].lut = luts ? luts[i] : nullptr;
        recs[i].lut_len = recs[i].lut ? (int)lut_len[i] : 0;
    }
    MVS_HIP_TRY(c, hipMemcpyAsync(base, recs.data(), sizeof(LabelTile) * (size_t)n_views, hipMemcpyHostToDevice, c->stream));
    P.views = (const LabelTile*)base;
    P.out = out_mem == MVS_MEM_HOST ? (int*)(base + rec_bytes + tile_bytes) : (int*)out;

    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    hipLaunchKernelGGL(label_tiles_fuse_kernel, dim3((unsigned)nblocks), dim3(kThreads), 0, c->stream, P);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    if (out_mem == MVS_MEM_HOST) MVS_HIP_TRY(c, hipMemcpyAsync(out, P.out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the records and host tiles were copied from pageable memory of this call)
    return area.release();
}
