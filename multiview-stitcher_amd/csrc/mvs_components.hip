// mvs_components.hip -- connected-component labelling of one thresholded tile on gfx950 (mvs_label_components, labels.py): a
// uint8 / uint16 / float32 tile becomes an int32 label image with the numbering of scipy.ndimage.label.  Six launches on one
// stream: rows (runs of foreground along x), merge (lock-free union of the runs across y and z), flatten (every voxel to its root,
// and the voxels per root when small components are dropped), and the numbering of the roots in raster order as count / scan /
// rank, then relabel.  Union and find: mvs_unionfind.h, which states the invariant everything rests on -- parent[i] <= i, only ever
// lowered -- so the root of a component is its first voxel in raster order whatever the order of execution, and numbering the roots
// in raster order is scipy's numbering.  Integer atomics only: equal inputs give equal bits.  Neighbourhood, launch geometry, scan
// partition, scratch and limits: mvs_components_plan.h.
#include "mvs_internal.h"
#include "mvs_fuse_dev.h"
#include "mvs_components_plan.h"
#include "mvs_unionfind.h"

#include <algorithm>

namespace {

using namespace mvs_components_plan;
using namespace mvs_unionfind;

// The tile as the row launch reads it and the chunk walk the row and merge launches share: a wave takes 64 consecutive voxels of
// a row at a time and ONE contiguous range of `per` such chunks (mvs_labels_plan.h), the same range in both launches.
struct TileWalk {
    long long sz, sy;                // element strides of the tile
    int nz, ny, nx;
    long long chunks, items, per;    // chunks per row; rows * chunks; chunks per wave
    float threshold;
};

// The 64 voxels at p, one per lane (lanes >= n: 0).  A whole chunk on a 16-byte boundary is read by 4 / 8 / 16 lanes (uint8 /
// uint16 / float32) with one 16-byte load each and handed out by shuffles, as load_chunk of mvs_labels.hip does for int32; the
// branch is the same for all lanes of the wave.
template <typename T>
__device__ __forceinline__ T load_voxels(const T* p, int n, int lane) {
    constexpr int kPer = 16 / (int)sizeof(T);      // voxels of one 16-byte load
    if (n == 64 && ((unsigned long long)p & 15u) == 0) {
        int4 w = make_int4(0, 0, 0, 0);
        if (lane < 64 / kPer) w = *(const int4*)(p + kPer * lane);
        const int src = lane / kPer, k = lane % kPer;
        const int word = k * (int)sizeof(T) / 4;
        const int a = __shfl(w.x, src), b = __shfl(w.y, src), c = __shfl(w.z, src), d = __shfl(w.w, src);
        const unsigned int u = (unsigned int)(word == 0 ? a : (word == 1 ? b : (word == 2 ? c : d)));
        if constexpr (sizeof(T) == 4) return __uint_as_float(u);
        else return (T)(u >> (8 * ((k * (int)sizeof(T)) & 3)));
    }
    return lane < n ? p[lane] : T(0);
}

// ---- 1. rows ------------------------------------------------------------------------------------------------------------------------
// parent[p] = the linear index of the first voxel of p's run of foreground along x, kBackground for a background voxel.  The start
// of the run that reaches the end of a chunk is carried in a register into the next chunk of the row.  A run that goes on from
// another wave's range starts anew at this wave's first chunk: the merge launch joins that seam.  No atomics.
template <typename T>
__global__ __launch_bounds__(kThreads) void component_rows_kernel(TileWalk W, const T* __restrict__ data, int* __restrict__ parent) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const long long first = wave * W.per, last = min(first + W.per, W.items);
    int carry = kBackground;      // start of the run that ended the previous chunk of this row at its last voxel (same in every lane)
    for (long long item = first; item < last; ++item) {
        const long long row = item / W.chunks;
        const int x0 = (int)(item % W.chunks) * 64;
        const int n = min(64, W.nx - x0);
        if (x0 == 0) carry = kBackground;
        const T v = load_voxels(data + (row / W.ny) * W.sz + (row % W.ny) * W.sy + x0, n, lane);
        const bool fg = lane < n && (float)v > W.threshold;      // (a NaN is not)
        const unsigned long long mask = __ballot(fg);
        const int base = (int)(row * W.nx + x0);
        const unsigned long long below = ~mask & ((1ull << lane) - 1ull);      // the background lanes before this one
        const int start = below ? base + 64 - __clzll((long long)below) : (carry >= 0 ? carry : base);
        if (lane < n) parent[base + lane] = fg ? start : kBackground;
        if (n == 64 && (mask >> 63)) {
            if (mask != ~0ull) carry = base + 64 - __clzll((long long)~mask);
            else if (carry < 0) carry = base;
        } else {
            carry = kBackground;
        }
    }
}

// ---- 2. merge -----------------------------------------------------------------------------------------------------------------------
struct MergeArgs {
    TileWalk W;
    int n_groups;
    RowGroup groups[kMaxRowGroups];
};

// Per neighbour row (dz, dy) of the half neighbourhood and per dx of it, a voxel p with p and q = p + o both foreground joins the
// two runs.  Foreground is the sign of parent[], which never changes, so plain loads decide it; one ballot per neighbour row (and
// one for the two voxels beside the chunk) gives the row's foreground as bits, and the three dx are shifts of them.  Consecutive
// lanes with p and q foreground are one run of p's and one run of q's: only the first lane of such a run calls the union, so a
// tile of foreground sends one union per chunk and row, not 64.  A diagonal is skipped where the voxel straight across is
// foreground (q and its x neighbour are one run) or where p's x neighbour on that side is (it is of p's run, and straight across
// from q): diagonals cost a union only where two objects touch by a corner alone.  The chase starts from the parents the lane has
// loaded already -- stale or not, they are ancestors -- and the root decision is uf_unite's: the value its atomic returns.
__global__ __launch_bounds__(kThreads) void component_merge_kernel(MergeArgs P, int* parent) {
    const TileWalk& W = P.W;
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const long long first = wave * W.per, last = min(first + W.per, W.items);
    for (long long item = first; item < last; ++item) {
        const long long row = item / W.chunks;
        const int z = (int)(row / W.ny), y = (int)(row % W.ny);
        const int x0 = (int)(item % W.chunks) * 64;
        const int n = min(64, W.nx - x0);
        const int base = (int)(row * W.nx + x0);
        const int me = lane < n ? parent[base + lane] : kBackground;
        const unsigned long long fgp = __ballot(me >= 0);
        if (!fgp) continue;
        // the seam the row launch left: this wave's range begins inside a row
        if (item == first && x0 > 0 && lane == 0 && me >= 0 && parent[base - 1] >= 0) uf_unite(parent, me, base - 1);
        for (int g = 0; g < P.n_groups; ++g) {
            const int qz = z + P.groups[g].dz, qy = y + P.groups[g].dy;
            if (qz < 0 || qz >= W.nz || qy < 0 || qy >= W.ny) continue;
            const int qbase = (int)(((long long)qz * W.ny + qy) * W.nx + x0);
            const int nb = lane < n ? parent[qbase + lane] : kBackground;
            const unsigned long long centre = __ballot(nb >= 0);
            int beside = kBackground;      // lane 0: the voxel before the chunk; lane 1: the one after it
            if (lane == 0 && x0 > 0) beside = parent[qbase - 1];
            if (lane == 1 && x0 + 64 < W.nx) beside = parent[qbase + 64];
            const unsigned long long edge = __ballot(beside >= 0);
            if (!(centre | edge)) continue;
            const unsigned long long across = fgp & centre;
            for (int dx = -1; dx <= 1; ++dx) {
                if (!((P.groups[g].dx_mask >> (dx + 1)) & 1u)) continue;
                unsigned long long both;
                if (dx == 0) both = across;
                else if (dx < 0) both = fgp & ((centre << 1) | (edge & 1ull)) & ~across & ~(fgp << 1);
                else both = fgp & ((centre >> 1) | ((edge >> 1) << 63)) & ~across & ~(fgp >> 1);
                const unsigned long long heads = both & ~(both << 1);
                if ((heads >> lane) & 1ull) uf_unite(parent, me, dx == 0 ? nb : qbase + lane + dx);
            }
        }
    }
}

// ---- 3. flatten (and 4. sizes) --------------------------------------------------------------------------------------------------------
// Voxels per root, counted by a wave over its chunks.  One root -- the wave's `sticky` one, the root of the first foreground voxel
// it met -- is counted in a register by ballots, however ragged its runs, and added once when the wave is done or when a chunk
// with foreground holds none of it and the wave takes that chunk's first root instead.  A large object therefore costs one atomic
// per wave on its one counter, not one per run.  The other roots are counted as mvs_label_counts counts labels: equal roots of
// consecutive lanes are a run, found by one shuffle and one ballot, and the first lane of the run adds its length.  Every lane of
// the wave calls count() and flush() together; sticky / sticky_n hold the same value in every lane.
struct RootCounter {
    unsigned int* sizes;
    int lane;
    int sticky = kBackground;
    unsigned int sticky_n = 0;

    __device__ __forceinline__ void flush() {
        if (sticky_n && lane == 0) atomicAdd(&sizes[sticky], sticky_n);
        sticky_n = 0;
    }

    __device__ __forceinline__ void count(int root) {
        const unsigned long long fg = __ballot(root >= 0);
        if (!fg) return;
        unsigned long long mine = sticky >= 0 ? __ballot(root == sticky) : 0ull;
        if (!mine) {
            flush();
            sticky = __shfl(root, __ffsll((long long)fg) - 1);
            mine = __ballot(root == sticky);
        }
        sticky_n += (unsigned int)__popcll(mine);
        const int key = root == sticky ? kBackground : root;
        const int prev = __shfl_up(key, 1);
        const bool head = lane == 0 || key != prev;
        const unsigned long long heads = __ballot(head);
        if (head && key >= 0) {
            const unsigned long long next = lane == 63 ? 0ull : heads >> (lane + 1);
            atomicAdd(&sizes[key], (unsigned int)(next ? __ffsll((long long)next) : 64 - lane));
        }
    }
};

// parent[p] = root(p) over the flat array, chunks of 64 voxels and a contiguous range of them per wave.  Every union is done, so
// roots no longer change, and a voxel that is no root never reads as one: parents are only lowered.  With `sizes` (zeros at the
// start) the voxels per root are counted on the way.
__global__ __launch_bounds__(kThreads) void component_flatten_kernel(int* parent, long long n_voxels, long long items, long long per, unsigned int* sizes) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const long long first = wave * per, last = min(first + per, items);
    RootCounter counter{sizes, lane};
    for (long long item = first; item < last; ++item) {
        const long long p = item * 64 + lane;
        int root = kBackground;
        if (p < n_voxels) {
            const int cur = parent[p];
            if (cur >= 0) {
                root = uf_find(parent, cur);
                if (root != cur) parent[p] = root;
            }
        }
        if (sizes) counter.count(root);
    }
    if (sizes) counter.flush();
}

// ---- 5. number ----------------------------------------------------------------------------------------------------------------------
struct NumberArgs {
    const int* parent;
    const unsigned int* sizes;       // NULL: every component is kept
    unsigned int min_voxels;
    long long n_voxels, span;        // ScanPlan: workgroup b has the voxels [b * span, (b + 1) * span)
};

// p is the root of a component that keeps its id
__device__ __forceinline__ bool kept_root(const NumberArgs& P, long long p) {
    return P.parent[p] == (int)p && (!P.sizes || P.sizes[p] >= P.min_voxels);
}

// block_counts[b] = the kept roots of workgroup b's voxels.  No atomics.
__global__ __launch_bounds__(kThreads) void component_count_kernel(NumberArgs P, int* block_counts) {
    __shared__ int s_wave[kWaves];
    const long long begin = (long long)blockIdx.x * P.span, end = min(begin + P.span, P.n_voxels);
    int count = 0;      // of this wave: the same in every lane
    for (long long p0 = begin; p0 < end; p0 += kThreads) {
        const long long p = p0 + threadIdx.x;
        count += __popcll(__ballot(p < end && kept_root(P, p)));
    }
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kWaves; ++w) total += s_wave[w];
        block_counts[blockIdx.x] = total;
    }
}

// One workgroup: block_counts[0 .. blocks) becomes its exclusive prefix sum and block_counts[blocks] the total, the number of ids.
// A thread sums its stretch of consecutive counts, thread 0 scans the 256 sums, the thread writes its stretch back.
__global__ __launch_bounds__(kThreads) void component_scan_kernel(int* block_counts, int blocks) {
    __shared__ int s_sum[kThreads];
    const int stretch = (blocks + kThreads - 1) / kThreads;
    const int lo = min((int)threadIdx.x * stretch, blocks), hi = min(lo + stretch, blocks);
    int sum = 0;
    for (int b = lo; b < hi; ++b) sum += block_counts[b];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int running = 0;
        for (int t = 0; t < kThreads; ++t) {
            const int s = s_sum[t];
            s_sum[t] = running;
            running += s;
        }
        block_counts[blocks] = running;
    }
    __syncthreads();
    int running = s_sum[threadIdx.x];
    for (int b = lo; b < hi; ++b) {
        const int cnt = block_counts[b];
        block_counts[b] = running;
        running += cnt;
    }
}

// out[root] = the id of the root: block base + kept roots before it in the workgroup's range + 1; 0 at a root that is dropped.
// Only roots are written: the relabel launch reads out[] at roots alone.
__global__ __launch_bounds__(kThreads) void component_rank_kernel(NumberArgs P, const int* __restrict__ block_base, int* out) {
    __shared__ int s_wave[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long begin = (long long)blockIdx.x * P.span, end = min(begin + P.span, P.n_voxels);
    int running = block_base[blockIdx.x];
    for (long long p0 = begin; p0 < end; p0 += kThreads) {      // (the same trips for every thread of the workgroup)
        const long long p = p0 + threadIdx.x;
        const bool root = p < end && P.parent[p] == (int)p;
        const bool kept = root && (!P.sizes || P.sizes[p] >= P.min_voxels);
        const unsigned long long mask = __ballot(kept);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        if (root) out[p] = kept ? running + before + __popcll(mask & ((1ull << lane) - 1ull)) + 1 : 0;
        running += total;
        __syncthreads();
    }
}

// ---- 6. relabel ---------------------------------------------------------------------------------------------------------------------
// out[p] = out[parent[p]] -- the id at p's root -- or 0 for background, four voxels per lane with 16-byte loads and stores where the
// result is on a 16-byte boundary.  A root's own slot is rewritten with the value it holds, so a lane that reads it meanwhile sees
// the id either way.
__device__ __forceinline__ int id_of(const int* out, int root) { return root < 0 ? 0 : out[root]; }

__global__ __launch_bounds__(kThreads) void component_relabel_kernel(const int* __restrict__ parent, long long n_voxels, int* out) {
    const bool vec = ((unsigned long long)out & 15u) == 0;
    const long long groups = (n_voxels + 3) / 4;
    for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kThreads) {
        const long long p = 4 * g;
        if (vec && p + 4 <= n_voxels) {
            const int4 r = *(const int4*)(parent + p);
            *(int4*)(out + p) = make_int4(id_of(out, r.x), id_of(out, r.y), id_of(out, r.z), id_of(out, r.w));
        } else {
            for (long long q = p; q < min(p + 4, n_voxels); ++q) out[q] = id_of(out, parent[q]);
        }
    }
}

// What the entry requires of its tile beyond mvs_check_tile_view.
int check_layout(MvsContext* c, const char* what, const mvs_view_t& v) {
    for (int k = 0; k < 3; ++k)
        if (v.shape[k] < 1 || v.shape[k] > 0x7fffffffLL) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: shape[%d] out of range", what, k);
    if (v.stride[2] != 1) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: the stride along x must be 1", what);
    if (v.stride[0] < 0 || v.stride[1] < 0) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: negative strides", what);
    if ((unsigned long long)v.data % mvs_dtype_size(v.dtype)) return mvs_fail(c, MVS_ERR_INVALID_ARG, "%s: data not aligned to its type", what);
    if (v.mem == MVS_MEM_HOST && (v.stride[1] != v.shape[2] || v.stride[0] != v.shape[1] * v.shape[2]))
        return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: host tiles must be C-contiguous", what);
    return MVS_OK;
}

}  // namespace

extern "C" int mvs_label_components(int device, const mvs_view_t* tile, int32_t ndim, float threshold, int32_t connectivity, int64_t min_voxels,
                                    int32_t* labels_out, int32_t out_mem, int64_t* n_labels_out) {
    const char* what = "mvs_label_components";
    MvsContext* c0 = mvs_ctx(device);
    if (!tile || !labels_out || !n_labels_out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", what);
    if (connectivity < 1 || connectivity > ndim) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: connectivity must be 1 .. ndim", what);
    if (out_mem != MVS_MEM_HOST && out_mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: bad out_mem", what);
    int rc = mvs_check_tile_view(c0, what, tile, ndim);
    if (rc) return rc;
    rc = check_layout(c0, what, *tile);
    if (rc) return rc;
    const long long n_voxels = voxel_count(tile->shape);
    if (n_voxels < 0) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 voxels", what);
    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    // one block: a host tile, parent, sizes, the scan's counts, a host result
    const size_t es = mvs_dtype_size(tile->dtype);
    size_t tile_bytes = 0;
    rc = mvs_stage_views_bytes(c, tile, 1, es, &tile_bytes);
    if (rc) return rc;
    const bool filter = min_voxels > 1;
    const size_t out_bytes = sizeof(int32_t) * (size_t)n_voxels;
    MvsWorkArea area(c);
    rc = area.alloc(tile_bytes + parent_bytes(n_voxels) + sizes_bytes(n_voxels, min_voxels) + scan_bytes() + (out_mem == MVS_MEM_HOST ? out_bytes : 0));
    if (rc) return rc;
    char* base = (char*)area.ptr;
    size_t cursor = 0;
    const void* dptr;
    rc = mvs_stage_view(c, *tile, es, base, &cursor, &dptr);
    if (rc) return rc;
    char* at = base + tile_bytes;
    int* parent = (int*)at;
    at += parent_bytes(n_voxels);
    unsigned int* sizes = filter ? (unsigned int*)at : nullptr;
    at += sizes_bytes(n_voxels, min_voxels);
    int* block_counts = (int*)at;
    at += scan_bytes();
    int* out = out_mem == MVS_MEM_HOST ? (int*)at : labels_out;

    MergeArgs M{};
    TileWalk& W = M.W;
    const bool staged = tile->mem == MVS_MEM_HOST;
    W.sz = staged ? tile->shape[1] * tile->shape[2] : tile->stride[0];
    W.sy = staged ? tile->shape[2] : tile->stride[1];
    W.nz = (int)tile->shape[0]; W.ny = (int)tile->shape[1]; W.nx = (int)tile->shape[2];
    W.chunks = row_chunks(W.nx);
    W.items = (long long)W.nz * W.ny * W.chunks;
    const int row_blocks = grid_blocks(W.items, kWaves);
    W.per = chunks_per_wave(W.items, (long long)row_blocks * kWaves);
    W.threshold = threshold;
    M.n_groups = row_groups(ndim, connectivity, M.groups);
    const long long flat_items = (n_voxels + 63) / 64;
    const int flat_blocks = grid_blocks(flat_items, kWaves);
    const ScanPlan scan = scan_plan(n_voxels);
    NumberArgs N{parent, sizes, (unsigned int)std::min<int64_t>(min_voxels, 0xffffffffLL), n_voxels, scan.span};

    if (filter) MVS_HIP_TRY(c, hipMemsetAsync(sizes, 0, sizes_bytes(n_voxels, min_voxels), c->stream));
    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    mvs_dispatch_dtype(tile->dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((component_rows_kernel<T>), dim3(row_blocks), dim3(kThreads), 0, c->stream, W, (const T*)dptr, parent);
    });
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(component_merge_kernel, dim3(row_blocks), dim3(kThreads), 0, c->stream, M, parent);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(component_flatten_kernel, dim3(flat_blocks), dim3(kThreads), 0, c->stream, parent, n_voxels, flat_items,
                       chunks_per_wave(flat_items, (long long)flat_blocks * kWaves), sizes);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(component_count_kernel, dim3(scan.blocks), dim3(kThreads), 0, c->stream, N, block_counts);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(component_scan_kernel, dim3(1), dim3(kThreads), 0, c->stream, block_counts, scan.blocks);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(component_rank_kernel, dim3(scan.blocks), dim3(kThreads), 0, c->stream, N, (const int*)block_counts, out);
    MVS_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(component_relabel_kernel, dim3(grid_blocks((n_voxels + 3) / 4, kThreads)), dim3(kThreads), 0, c->stream, (const int*)parent, n_voxels,
                       out);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    int n_labels = 0;
    MVS_HIP_TRY(c, hipMemcpyAsync(&n_labels, block_counts + scan.blocks, sizeof(n_labels), hipMemcpyDeviceToHost, c->stream));
    if (out_mem == MVS_MEM_HOST) MVS_HIP_TRY(c, hipMemcpyAsync(labels_out, out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_labels_out = n_labels;
    return area.release();
}
