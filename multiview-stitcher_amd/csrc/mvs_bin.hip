// mvs_bin.hip -- block-mean binning of tiles on the GPU (gfx950): the mvs_bin_mean* entry points.
#include "mvs_internal.h"
#include "mvs_bin_dev.h"

#include <algorithm>

namespace {
inline int grid_for(long long n) { return (int)std::min<long long>((n + 255) / 256, 256 * 8); }
}  // namespace

// ---- block-mean binning == sim.coarsen(bins, boundary="trim").mean().astype(dtype) (registration.py:1732-1741) ----
namespace {
template <typename T>
__global__ void bin_mean_kernel(const T* __restrict__ in, long long sz, long long sy, T* __restrict__ out, int oz, int oy, int ox,
                                int bz, int by, int bx) {
    const long long n = (long long)oz * oy * ox;
    const double count = (double)bz * by * bx;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % ox);
        const long long t = i / ox;
        const int y = (int)(t % oy), z = (int)(t / oy);
        double acc = 0.0;
        for (int dz = 0; dz < bz; ++dz)
            for (int dy = 0; dy < by; ++dy) {
                const T* row = in + (long long)(z * bz + dz) * sz + (long long)(y * by + dy) * sy + (long long)x * bx;
                for (int dx = 0; dx < bx; ++dx) acc += (double)row[dx];
            }
        out[i] = mvs_bin::mean_cast<T>(acc, count);   // sum / count in double; astype: truncation for integer dtypes
    }
}
// uint16, bin 2 along x, rows 16-byte aligned: a thread produces 4 consecutive outputs of a row from one 16-byte load per
// input row (the generic kernel reads element by element: 1.3 TB/s on a 512^3 tile).  Integer sums are exact in double,
// so the order of the additions does not matter and the result equals the generic kernel's.
__global__ __launch_bounds__(256) void bin_mean_u16x2_kernel(const unsigned short* __restrict__ in, long long sz, long long sy,
                                                             unsigned short* __restrict__ out, int oz, int oy, int ox, int bz, int by) {
    const int gx = ox >> 2;                                   // groups of 4 outputs per row (ox % 4 == 0)
    const long long ngroups = (long long)oz * oy * gx;
    const double count = (double)bz * by * 2;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (long long)gridDim.x * blockDim.x) {
        const int xg = (int)(g % gx);
        const long long t = g / gx;
        const int y = (int)(t % oy), z = (int)(t / oy);
        unsigned int acc[4] = {0u, 0u, 0u, 0u};               // at most 2 * by * bz * 65535: fits for by * bz <= 32767
        for (int dz = 0; dz < bz; ++dz)
            for (int dy = 0; dy < by; ++dy) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(in + (long long)(z * bz + dz) * sz + (long long)(y * by + dy) * sy + (long long)xg * 8);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] += (v[k] & 0xffffu) + (v[k] >> 16);
            }
        unsigned short r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = mvs_bin::mean_cast<unsigned short>(acc[k], count);   // astype: truncation
        *reinterpret_cast<uint2*>(out + ((long long)z * oy + y) * ox + (long long)xg * 4) =
            make_uint2((unsigned int)r[0] | ((unsigned int)r[1] << 16), (unsigned int)r[2] | ((unsigned int)r[3] << 16));
    }
}
// the same for up to kBinBatch views of one shape in one launch: blockIdx.y = view (pointer table in the kernel arguments)
constexpr int kBinBatch = 32;
struct BinBatch {
    const unsigned short* in[kBinBatch];
    unsigned short* out[kBinBatch];
};
__global__ __launch_bounds__(256) void bin_mean_u16x2_batch_kernel(BinBatch B, long long sz, long long sy, int oz, int oy, int ox, int bz, int by) {
    const unsigned short* __restrict__ in = B.in[blockIdx.y];
    unsigned short* __restrict__ out = B.out[blockIdx.y];
    const int gx = ox >> 2;
    const long long ngroups = (long long)oz * oy * gx;
    const double count = (double)bz * by * 2;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (long long)gridDim.x * blockDim.x) {
        const int xg = (int)(g % gx);
        const long long t = g / gx;
        const int y = (int)(t % oy), z = (int)(t / oy);
        unsigned int acc[4] = {0u, 0u, 0u, 0u};
        for (int dz = 0; dz < bz; ++dz)
            for (int dy = 0; dy < by; ++dy) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(in + (long long)(z * bz + dz) * sz + (long long)(y * by + dy) * sy + (long long)xg * 8);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] += (v[k] & 0xffffu) + (v[k] >> 16);
            }
        unsigned short r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = mvs_bin::mean_cast<unsigned short>(acc[k], count);   // astype: truncation
        *reinterpret_cast<uint2*>(out + ((long long)z * oy + y) * ox + (long long)xg * 4) =
            make_uint2((unsigned int)r[0] | ((unsigned int)r[1] << 16), (unsigned int)r[2] | ((unsigned int)r[3] << 16));
    }
}
}  // namespace

static int bin_mean_impl(int device, const void* in, int32_t dtype, int32_t mem, const int64_t shape[3], const int64_t stride[3],
                         const int64_t bin[3], void* out, int32_t out_mem, bool wait);

// mvs_bin_mean_async for n views of one shape, stride and dtype in one call (and, for 16-bit tiles binned by 2 along x, one launch per
// kBinBatch views): registration.register bins all tiles of a mosaic before its pairs start.
extern "C" int mvs_bin_mean_batch_async(int device, int32_t n_views, const void* const* in, int32_t dtype, const int64_t shape[3],
                                        const int64_t stride[3], const int64_t bin[3], void* const* out) {
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (n_views < 0 || (n_views > 0 && (!in || !out)) || !shape || !stride || !bin) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_bin_mean_batch_async: NULL argument");
    bool vec = dtype == MVS_U16 && stride[2] == 1 && bin[2] == 2 && bin[0] >= 1 && bin[1] >= 1 && shape[0] >= bin[0] && shape[1] >= bin[1] &&
               shape[2] >= 2 && (shape[2] / 2) % 4 == 0 && stride[1] % 8 == 0 && stride[0] % 8 == 0 && bin[0] * bin[1] <= 16384;
    for (int v = 0; v < n_views && vec; ++v) vec = in[v] && out[v] && ((uintptr_t)in[v] % 16) == 0 && ((uintptr_t)out[v] % 8) == 0;
    if (!vec) {
        for (int v = 0; v < n_views; ++v) {
            rc = bin_mean_impl(device, in[v], dtype, MVS_MEM_DEVICE, shape, stride, bin, out[v], MVS_MEM_DEVICE, false);
            if (rc) return rc;
        }
        return MVS_OK;
    }
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));
    const int oz = (int)(shape[0] / bin[0]), oy = (int)(shape[1] / bin[1]), ox = (int)(shape[2] / 2);
    const long long n = (long long)oz * oy * ox;
    for (int v0 = 0; v0 < n_views; v0 += kBinBatch) {
        const int nb = std::min(kBinBatch, n_views - v0);
        BinBatch B;
        for (int k = 0; k < kBinBatch; ++k) {
            B.in[k] = (const unsigned short*)in[v0 + std::min(k, nb - 1)];
            B.out[k] = (unsigned short*)out[v0 + std::min(k, nb - 1)];
        }
        hipLaunchKernelGGL(bin_mean_u16x2_batch_kernel, dim3(grid_for(n / 4), nb), dim3(256), 0, c->stream, B, (long long)stride[0], (long long)stride[1],
                           oz, oy, ox, (int)bin[0], (int)bin[1]);
    }
    MVS_HIP_TRY(c, hipGetLastError());
    return MVS_OK;
}

extern "C" int mvs_bin_mean(int device, const void* in, int32_t dtype, int32_t mem, const int64_t shape[3],
                            const int64_t stride[3], const int64_t bin[3], void* out, int32_t out_mem) {
    return bin_mean_impl(device, in, dtype, mem, shape, stride, bin, out, out_mem, true);
}

// The same launch without the final wait (device memory on both sides only): the caller orders later work with
// mvs_synchronize(device) -- used to bin all tiles of a mosaic while the host builds its overlap graph.
extern "C" int mvs_bin_mean_async(int device, const void* in, int32_t dtype, const int64_t shape[3], const int64_t stride[3],
                                  const int64_t bin[3], void* out) {
    return bin_mean_impl(device, in, dtype, MVS_MEM_DEVICE, shape, stride, bin, out, MVS_MEM_DEVICE, false);
}

static int bin_mean_impl(int device, const void* in, int32_t dtype, int32_t mem, const int64_t shape[3], const int64_t stride[3],
                         const int64_t bin[3], void* out, int32_t out_mem, bool wait) {
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (!in || !out || !shape || !stride || !bin) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_bin_mean: NULL argument");
    const size_t es = mvs_dtype_size(dtype);
    if (!es) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_bin_mean: bad dtype");
    if (stride[2] != 1) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "mvs_bin_mean: x stride must be 1");
    int o[3];
    for (int k = 0; k < 3; ++k) {
        if (bin[k] < 1 || shape[k] < bin[k]) return mvs_fail(c, MVS_ERR_INVALID_ARG, "mvs_bin_mean: bad bin/shape on axis %d", k);
        o[k] = (int)(shape[k] / bin[k]);
    }
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));
    const void* din = in;
    long long sz = stride[0], sy = stride[1];
    if (mem == MVS_MEM_HOST) {
        if (stride[1] != shape[2] || stride[0] != shape[1] * shape[2])
            return mvs_fail(c, MVS_ERR_UNSUPPORTED, "mvs_bin_mean: host input must be C-contiguous");
        const size_t nb = (size_t)shape[0] * shape[1] * shape[2] * es;
        void* s = mvs_scratch(c, 4, nb);
        if (!s) return mvs_alloc_failed(c);
        MVS_HIP_TRY(c, hipMemcpyAsync(s, in, nb, hipMemcpyHostToDevice, c->stream));
        din = s;
    }
    const long long n = (long long)o[0] * o[1] * o[2];
    void* dout = out;
    if (out_mem == MVS_MEM_HOST) {
        dout = mvs_scratch(c, 5, (size_t)n * es);
        if (!dout) return mvs_alloc_failed(c);
    }
    const int gb = grid_for(n);
    const bool vec_u16 = dtype == MVS_U16 && bin[2] == 2 && o[2] % 4 == 0 && sy % 8 == 0 && sz % 8 == 0 && ((uintptr_t)din % 16) == 0 &&
                         ((uintptr_t)dout % 8) == 0 && bin[0] * bin[1] <= 16384;
    if (vec_u16) {
        hipLaunchKernelGGL(bin_mean_u16x2_kernel, dim3(grid_for(n / 4)), dim3(256), 0, c->stream, (const unsigned short*)din, sz, sy,
                           (unsigned short*)dout, o[0], o[1], o[2], (int)bin[0], (int)bin[1]);
    } else
        mvs_dispatch_dtype(dtype, [&](auto tag) {
            using T = decltype(tag);
            hipLaunchKernelGGL(bin_mean_kernel<T>, dim3(gb), dim3(256), 0, c->stream, (const T*)din, sz, sy, (T*)dout, o[0], o[1], o[2],
                               (int)bin[0], (int)bin[1], (int)bin[2]);
        });
    MVS_HIP_TRY(c, hipGetLastError());
    if (out_mem == MVS_MEM_HOST) MVS_HIP_TRY(c, hipMemcpyAsync(out, dout, (size_t)n * es, hipMemcpyDeviceToHost, c->stream));
    if (wait) MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MVS_OK;
}
