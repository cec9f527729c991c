// mvs_tile_apply.h -- what the two "a gain and an offset per voxel of a tile" entry points share (mvs_intensity_apply,
// mvs_intensity.hip; mvs_plane_apply, mvs_shading.hip): the aligned element vector and the rounding store of their kernels, the
// split of a row into a scalar head, whole vectors and a scalar tail (host/device: tests/native/tile_row_split_host_test.cpp
// runs it on the host), and the host frame of the entry point.  The kernels themselves differ (rows through LDS / coefficients
// in registers along z) and stay in their files.
#pragma once
#include "mvs_internal.h"
#include "mvs_fuse_dev.h"
#include "mvs_intensity_dev.h"

// ---- device pieces ------------------------------------------------------------------------------------------------------------------
template <typename T, int V>
struct alignas(V * sizeof(T)) TileVec {
    T v[V];
};

template <typename TOut> __device__ __forceinline__ TOut tile_store(float y);
template <> __device__ __forceinline__ float tile_store<float>(float y) { return y; }
template <> __device__ __forceinline__ unsigned char tile_store<unsigned char>(float y) { return (unsigned char)intensity_saturate(y, 255.f); }
template <> __device__ __forceinline__ unsigned short tile_store<unsigned short>(float y) { return (unsigned short)intensity_saturate(y, 65535.f); }

// elements per lane and step: 16 bytes on the wider side
template <typename TIn, typename TOut>
constexpr int tile_vec_len() {
    return 16 / (int)(sizeof(TIn) > sizeof(TOut) ? sizeof(TIn) : sizeof(TOut));
}

// ---- the row split --------------------------------------------------------------------------------------------------------------------
// A row of nx elements, read at src_addr (elements of in_es bytes) and written at dst_addr (out_es bytes): [0, head) and [tail, nx)
// go element by element, [head, tail) in nvec vectors of V elements.  The head runs up to the first source element aligned to
// V * in_es bytes.  The whole row is scalar (head = nx) when the head exceeds the row, when the source is not element-aligned,
// when the destination at `head` is not aligned to V * out_es bytes, or when the caller forbids vectors.
struct TileRowSplit {
    int head, nvec, tail;
};

MVS_HD TileRowSplit tile_row_split(unsigned long long src_addr, unsigned long long dst_addr, int nx, int in_es, int out_es, int V, bool vectors_allowed) {
    const unsigned long long in_vec = (unsigned long long)(V * in_es), out_vec = (unsigned long long)(V * out_es);
    const unsigned long long mis = src_addr % in_vec;
    int head = mis ? (int)((in_vec - mis) / (unsigned long long)in_es) : 0;
    if (head > nx || mis % (unsigned long long)in_es || (dst_addr + (unsigned long long)head * (unsigned long long)out_es) % out_vec || !vectors_allowed) head = nx;
    const int nvec = (nx - head) / V;
    return TileRowSplit{head, nvec, head + nvec * V};
}

// ---- the host frame -------------------------------------------------------------------------------------------------------------------
struct TileApplyArgs {
    const void* in;
    void* out;
    long long in_sz, in_sy;                         // elements; the output is C-contiguous
    int nz, ny, nx;
};

// For the `prepare` of the entries that interpolate per-cell values (mvs_intensity_apply, mvs_field_warp): the host's `values`
// (value_bytes of them) and its per-axis `tables` -- for z, y, x in turn shape[k] int32 lower cells, then shape[k] float32 weights
// -- through scratch slot 2.  *dvalues, cell[k] and frac[k] are where the kernel reads them.
inline int mvs_tile_apply_tables(MvsContext* c, const mvs_view_t* view, const void* values, size_t value_bytes, const void* tables, const void** dvalues,
                                 const int* cell[3], const float* frac[3]) {
    const size_t table_bytes = 8 * ((size_t)view->shape[0] + view->shape[1] + view->shape[2]);
    char* small = (char*)mvs_scratch(c, 2, align_up(value_bytes) + table_bytes);
    if (!small) return mvs_alloc_failed(c);
    MVS_HIP_TRY(c, hipMemcpyAsync(small, values, value_bytes, hipMemcpyHostToDevice, c->stream));
    MVS_HIP_TRY(c, hipMemcpyAsync(small + align_up(value_bytes), tables, table_bytes, hipMemcpyHostToDevice, c->stream));
    *dvalues = small;
    char* t = small + align_up(value_bytes);
    for (int k = 0; k < 3; ++k) {
        cell[k] = (const int*)t;
        frac[k] = (const float*)(t + 4 * (size_t)view->shape[k]);
        t += 8 * (size_t)view->shape[k];
    }
    return MVS_OK;
}

// One apply entry point after its own refusals: the refusals both share, the context, the tile through scratch slot 0, the output
// (scratch slot 1 for a host result), `prepare(c, args)` for the entry's coefficients and launch geometry (scratch slot 2 is
// its), the timed `launch(tin, tout)` with tout of the input's type or float, and the download.
template <typename Prepare, typename Launch>
int mvs_tile_apply(int device, const char* what, const mvs_view_t* view, int ndim, void* out, int out_dtype, int out_mem, Prepare&& prepare,
                   Launch&& launch) {
    MvsContext* c0 = mvs_ctx(device);
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", what);
    int rc = mvs_check_tile_view(c0, what, view, ndim);
    if (rc) return rc;
    if (out_mem != MVS_MEM_HOST && out_mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: bad out_mem", what);
    if (out_dtype != view->dtype && out_dtype != MVS_F32)
        return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: out_dtype must be the input's dtype or float32 (%d -> %d given)", what, view->dtype, out_dtype);
    for (int k = 0; k < 3; ++k)
        if (view->shape[k] < 1 || view->shape[k] > 0x7fffffffLL) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: view shape[%d] out of range", what, k);
    if (view->mem == MVS_MEM_DEVICE && view->stride[2] != 1) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: view stride along x must be 1", what);
    const bool in_place = view->mem == MVS_MEM_DEVICE && out_mem == MVS_MEM_DEVICE && out == view->data;
    if (in_place && (out_dtype != view->dtype || view->stride[1] != view->shape[2] || view->stride[0] != view->shape[1] * view->shape[2]))
        return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: in place needs a contiguous array and out_dtype == dtype", what);
    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    TileApplyArgs A;
    rc = mvs_stage_tile_views(c, &view, 1, ndim, &A.in, nullptr);
    if (rc) return rc;
    A.in_sz = view->mem == MVS_MEM_HOST ? view->shape[1] * view->shape[2] : view->stride[0];
    A.in_sy = view->mem == MVS_MEM_HOST ? view->shape[2] : view->stride[1];
    A.nz = (int)view->shape[0]; A.ny = (int)view->shape[1]; A.nx = (int)view->shape[2];
    const size_t out_bytes = (size_t)view->shape[0] * view->shape[1] * view->shape[2] * mvs_dtype_size(out_dtype);
    A.out = out;
    if (out_mem == MVS_MEM_HOST) {
        A.out = mvs_scratch(c, 1, out_bytes);
        if (!A.out) return mvs_alloc_failed(c);
    }
    rc = prepare(c, A);
    if (rc) return rc;

    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    mvs_dispatch_dtype(view->dtype, [&](auto tin) {
        if (out_dtype == view->dtype) launch(tin, tin);
        else launch(tin, 0.f);
    });
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    if (out_mem == MVS_MEM_HOST) MVS_HIP_TRY(c, hipMemcpyAsync(out, A.out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MVS_OK;
}
