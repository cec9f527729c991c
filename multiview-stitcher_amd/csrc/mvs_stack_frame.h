// mvs_stack_frame.h -- internal: what the entry points that fuse a resampled (V, *S) stack share (mvs_mv_deconv, mvs_multiband_fuse).
// Two parts.  The integer geometry (namespace mvs_stack_frame) is host-only pure C++, so the plan headers build on it and
// tests/native/deconv_plan_host_test.cpp compiles it with the host compiler under the address and undefined-behaviour sanitizers: the
// output box of a call and the builder of a work-area layout.  The HIP part (compiled by hipcc only) holds the refusals whose text
// the entries share, as functions so that each entry keeps the order of its own between them, and the call frame after the refusals.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mvs_stack_frame {

// The result of a stack call: the stack's shape less `trim` on either side of every axis, as `out_dtype` (enum mvs_dtype of
// include/mvs_hip.h, restated here to keep this part free of other headers: 0 uint8, 1 uint16, 2 float32; the HIP part asserts it).
constexpr int32_t kU8 = 0, kU16 = 1, kF32 = 2;

struct OutBox {
    long long oz, oy, ox;
    size_t out_bytes;
};

inline OutBox out_box(const int64_t shape[3], const int64_t trim[3], int32_t out_dtype) {
    OutBox b;
    b.oz = shape[0] - 2 * trim[0], b.oy = shape[1] - 2 * trim[1], b.ox = shape[2] - 2 * trim[2];
    b.out_bytes = (size_t)(b.oz * b.oy * b.ox) * (out_dtype == kF32 ? 4 : out_dtype == kU16 ? 2 : 1);
    return b;
}

// The parts of one device work area, in the order they are taken.  A part starts where the one before it ended and its bytes are
// padded to a multiple of `align`: 256 keeps the next part on a 256-byte boundary, 4 packs float volumes, 1 takes the bytes as they
// are (the staging of a host result, last).  A part of 0 bytes takes nothing and shares its offset with the next one.
struct Layout {
    size_t total = 0;
    size_t take(size_t bytes, size_t align) {
        const size_t at = total;
        total += (bytes + align - 1) / align * align;
        return at;
    }
};

}  // namespace mvs_stack_frame

#ifdef __HIPCC__
#include "mvs_internal.h"

static_assert(MVS_U8 == mvs_stack_frame::kU8 && MVS_U16 == mvs_stack_frame::kU16 && MVS_F32 == mvs_stack_frame::kF32, "out_box restates enum mvs_dtype");

// ---- the refusals both entries word alike; `what` is the entry's name ------------------------------------------------------------
inline int mvs_stack_check_out(MvsContext* c0, const char* what, int32_t out_mem, int32_t out_dtype) {
    if (out_mem != MVS_MEM_HOST && out_mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: bad out_mem", what);
    if (out_dtype != MVS_U8 && out_dtype != MVS_U16 && out_dtype != MVS_F32) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: bad out_dtype", what);
    return MVS_OK;
}

inline int mvs_stack_check_trim(MvsContext* c0, const char* what, const int64_t shape[3], const int64_t trim[3], int k) {
    if (trim[k] < 0 || 2 * trim[k] >= shape[k]) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: trim on axis %d leaves nothing", what, k);
    return MVS_OK;
}

inline int mvs_stack_check_size(MvsContext* c0, const char* what, long long voxels, int n_views) {
    if (voxels * n_views > (1LL << 40)) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: too large", what);
    return MVS_OK;
}

// ---- one call after its refusals ---------------------------------------------------------------------------------------------------
// begin(): the context, its lock (held until the frame goes) and the device.  reserve(): the work area of `total` bytes from the
// context's pool, `dout` (the caller's pointer, or the `out_bytes` at `off_out` of the work area that stage a host result), and the
// start of the timed span.  The entry then queues its launches on c->stream.  finish(): the end of the timed span, the download and
// the wait of a host result, and the work area back to the pool.  An error return in between leaves through ~MvsWorkArea, which
// waits for the stream first.
struct MvsStackFrame {
    MvsContext* c = nullptr;
    std::unique_lock<std::recursive_mutex> lock;
    MvsWorkArea work{nullptr};      // (after `lock`: it goes first)
    char* W = nullptr;              // the work area
    void* out = nullptr;            // the caller's result pointer
    void* dout = nullptr;           // where the kernels write the result
    size_t staged_bytes = 0;        // of a host result, else 0

    int begin(int device) {
        int rc = mvs_check_ready(device, &c);
        if (rc) return rc;
        lock = std::unique_lock<std::recursive_mutex>(c->mu);
        MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));
        work.c = c;
        return MVS_OK;
    }

    int reserve(size_t total, size_t off_out, void* out_, int32_t out_mem, size_t out_bytes) {
        int rc = work.alloc(total);
        if (rc) return rc;
        W = (char*)work.ptr;
        out = out_;
        staged_bytes = out_mem == MVS_MEM_HOST ? out_bytes : 0;
        dout = out_mem == MVS_MEM_HOST ? (void*)(W + off_out) : out;
        MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
        return MVS_OK;
    }

    int finish() {
        MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
        c->timing_valid = true;
        if (staged_bytes) {
            MVS_HIP_TRY(c, hipMemcpyAsync(out, dout, staged_bytes, hipMemcpyDeviceToHost, c->stream));
            MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        // the work area goes back to the pool; the pool hands it out again only to work later on this stream
        return work.release();
    }
};
#endif  // __HIPCC__
