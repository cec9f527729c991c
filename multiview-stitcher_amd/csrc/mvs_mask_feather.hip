// mvs_mask_feather.hip -- a binary mask as a feathered weight tile (masks.feather) on gfx950: W = rint(252 (1 - cos(pi min(t, 1))) / 2)
// with t the distance to the nearest zero voxel of the mask in units of the feather width per axis.  The squared distance is an
// integer, N = D t^2 capped at D (mvs_mask_feather_plan.h: the scale, the z slabs and the scratch bound), computed by separable
// min-plus passes x, y, z over uint32 planes; the last pass turns N into W in float64.  Integer minima in a fixed order and no
// atomics: equal inputs give equal bytes, and so do different slab sizes.
#include "mvs_internal.h"
#include "mvs_fuse_dev.h"
#include "mvs_mask_feather_plan.h"

#include <cmath>

namespace {

using namespace mvs_mask_feather_plan;
static_assert(kMaxWidth == MVS_FEATHER_MAX_WIDTH && kFullWeight == MVS_FEATHER_FULL_WEIGHT, "limits of mvs_hip.h and mvs_mask_feather_plan.h differ");

struct FeatherDims {
    int nz, ny, nx;
    long long groups;            // groups of kGroup voxels per row
};

// where a pass writes: the uint32 plane set (plane z - plane0) or, as the last pass, the uint8 result (plane z)
struct FeatherOut {
    unsigned int* n;
    long long plane0;
    unsigned char* w;            // not NULL: the last pass
    unsigned int D;
};

// W of N = D t^2: float64, rounded to nearest even.  N == 0 and N == D are exact without the cosine.
__device__ __forceinline__ unsigned char weight_of(unsigned int N, unsigned int D) {
    if (N == 0u) return 0;
    if (N >= D) return (unsigned char)kFullWeight;
    const double t = sqrt((double)N / (double)D);
    return (unsigned char)(int)rint((double)kFullWeight * (0.5 * (1.0 - cos(M_PI * t))));
}

__device__ __forceinline__ void emit(const FeatherOut& O, const FeatherDims& Dm, long long z, long long y, long long x, unsigned int N) {
    if (O.w) O.w[(z * Dm.ny + y) * (long long)Dm.nx + x] = weight_of(N, O.D);
    else O.n[((z - O.plane0) * Dm.ny + y) * (long long)Dm.nx + x] = N;
}

// the four bytes of a word that are zero, as four bits
__device__ __forceinline__ unsigned int zero_bits4(unsigned int d) {
    const unsigned int nz = (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;      // bit 7 of every byte that is not zero
    const unsigned int z = (~nz & 0x80808080u) >> 7;
    return (z & 1u) | ((z >> 7) & 2u) | ((z >> 14) & 4u) | ((z >> 21) & 8u);
}

// x pass: N = min(D, d^2 P_x), d the distance to the nearest zero voxel of the row within +- (w - 1) voxels (voxels outside the row
// are not zero).  A lane takes one group of 16 voxels: the zero voxels of the positions x0 - 32 .. x0 + 47 as 80 bits (16-byte loads
// where a group is whole and aligned, bytes otherwise), per voxel the 63 bits around it, and the nearest set bit on either side by
// one count of leading and one of trailing zeros.
__global__ __launch_bounds__(kThreads) void feather_x_kernel(const unsigned char* __restrict__ mask, long long sz, long long sy, FeatherDims Dm, long long z_lo,
                                                             long long z_hi, int w, unsigned int Px, FeatherOut O) {
    const long long items = (z_hi - z_lo) * Dm.ny * Dm.groups;
    for (long long item = (long long)blockIdx.x * kThreads + threadIdx.x; item < items; item += (long long)gridDim.x * kThreads) {
        const long long row = item / Dm.groups, g = item % Dm.groups;
        const long long z = z_lo + row / Dm.ny, y = row % Dm.ny, x0 = g * kGroup;
        const unsigned char* line = mask + z * sz + y * sy;
        unsigned long long part[5];
#pragma unroll
        for (int k = -2; k <= 2; ++k) {
            const long long xs = x0 + k * kGroup;
            unsigned int bits = 0u;
            const bool need = xs + kGroup > 0 && xs < Dm.nx && ((k >= -1 && k <= 1) || w > kGroup);      // w <= 16 stays within g - 1 .. g + 1
            if (need) {
                const unsigned char* p = line + xs;
                if (xs >= 0 && xs + kGroup <= Dm.nx && ((unsigned long long)p & 15u) == 0) {
                    const uint4 v = *(const uint4*)p;
                    bits = zero_bits4(v.x) | (zero_bits4(v.y) << 4) | (zero_bits4(v.z) << 8) | (zero_bits4(v.w) << 12);
                } else {
#pragma unroll
                    for (int j = 0; j < kGroup; ++j)
                        if (xs + j >= 0 && xs + j < Dm.nx && p[j] == 0) bits |= 1u << j;
                }
            }
            part[k + 2] = (unsigned long long)bits;
        }
        const unsigned long long lo = part[0] | (part[1] << 16) | (part[2] << 32) | (part[3] << 48), hi = part[4];      // bit i: position x0 - 32 + i
        const int nvalid = (int)min((long long)kGroup, Dm.nx - x0);
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            if (j >= nvalid) continue;
            const int s = 1 + j;                                                   // 1 .. 16: bit 31 of u is the voxel itself
            const unsigned long long u = ((lo >> s) | (hi << (64 - s))) & 0x7fffffffffffffffull;
            const unsigned long long right = u >> 31, left = u & 0xffffffffull;
            const int dr = right ? __ffsll((long long)right) - 1 : 64;
            const int dl = left ? __clzll((long long)left) - 32 : 64;
            const int d = min(dl, dr);
            const unsigned int N = d >= w ? O.D : min(O.D, (unsigned int)(d * d) * Px);
            emit(O, Dm, z, y, x0 + j, N);
        }
    }
}

// y pass (axis 1) over the planes [z_lo, z_hi) or z pass (axis 0): N(p) = min(D, min_{|j| <= w} N_prev(p + j e) + j^2 P), the
// neighbours inside the mask only; one voxel per lane, consecutive lanes along x.  `in`: the plane set, first plane in_plane0.
__global__ __launch_bounds__(kThreads) void feather_lines_kernel(const unsigned int* __restrict__ in, long long in_plane0, FeatherDims Dm, long long z_lo,
                                                                 long long z_hi, int axis, int w, unsigned int P, FeatherOut O) {
    const long long plane = (long long)Dm.ny * Dm.nx, items = (z_hi - z_lo) * plane;
    const int n = axis ? Dm.ny : Dm.nz;
    const long long step = axis ? (long long)Dm.nx : plane;
    for (long long item = (long long)blockIdx.x * kThreads + threadIdx.x; item < items; item += (long long)gridDim.x * kThreads) {
        const long long z = z_lo + item / plane, rem = item % plane, y = rem / Dm.nx, x = rem % Dm.nx;
        const int at = axis ? (int)y : (int)z;
        const unsigned int* p = in + (z - in_plane0) * plane + rem;
        unsigned int best = O.D;
        for (int j = max(-w, -at); j <= min(w, n - 1 - at); ++j) best = min(best, p[j * step] + (unsigned int)(j * j) * P);
        emit(O, Dm, z, y, x, best);
    }
}

}  // namespace

extern "C" int mvs_mask_feather(int device, const mvs_view_t* mask, int32_t ndim, const int32_t width[3], void* out, int32_t out_mem) {
    const char* what = "mvs_mask_feather";
    MvsContext* c0 = mvs_ctx(device);
    if (!mask || !width || !out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", what);
    if (out_mem != MVS_MEM_HOST && out_mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: bad out_mem", what);
    int w[3] = {1, 1, 1};
    for (int k = 3 - ndim; k < 3; ++k) {
        if (width[k] < 1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: width[%d] < 1", what, k);
        if (width[k] > MVS_FEATHER_MAX_WIDTH) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: width[%d] = %d exceeds %d", what, k, width[k], MVS_FEATHER_MAX_WIDTH);
        w[k] = width[k];
    }
    int rc = mvs_check_tile_view(c0, what, mask, ndim);
    if (rc) return rc;
    if (mask->dtype != MVS_U8) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: masks are uint8", what);
    for (int k = 0; k < 3; ++k)
        if (mask->shape[k] < 1 || mask->shape[k] > 0x7fffffffLL) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: shape[%d] out of range", what, k);
    if (mask->stride[2] != 1) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: the stride along x must be 1", what);
    MvsContext* c;
    rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    FeatherDims Dm;
    Dm.nz = (int)mask->shape[0]; Dm.ny = (int)mask->shape[1]; Dm.nx = (int)mask->shape[2];
    Dm.groups = (Dm.nx + kGroup - 1) / kGroup;
    const Scale S = scale_of(w);
    const bool pass_y = pass_needed(Dm.ny, w[1]), pass_z = pass_needed(Dm.nz, w[0]);
    const int halo = pass_z ? w[0] : 0;
    const long long planes = slab_planes(Dm.nz, Dm.ny, Dm.nx, halo, c->feather_slab_planes);
    const size_t set_bytes = align_up(plane_set_bytes(Dm.nz, Dm.ny, Dm.nx, planes, halo));
    const size_t n_sets = (pass_y && pass_z) ? 2 : ((pass_y || pass_z) ? 1 : 0);
    unsigned int* sets[2] = {nullptr, nullptr};
    if (n_sets) {
        char* base = (char*)mvs_scratch(c, 1, set_bytes * n_sets);
        if (!base) return mvs_alloc_failed(c);
        sets[0] = (unsigned int*)base;
        sets[1] = (unsigned int*)(base + set_bytes * (n_sets - 1));
    }
    // a host mask and a host result go through one block for the duration of the call
    size_t mask_bytes = 0;
    rc = mvs_stage_views_bytes(c, mask, 1, 1, &mask_bytes);
    if (rc) return rc;
    const size_t out_bytes = (size_t)Dm.nz * Dm.ny * Dm.nx;
    MvsWorkArea area(c);
    const size_t area_bytes = mask_bytes + (out_mem == MVS_MEM_HOST ? out_bytes : 0);
    if (area_bytes) {
        rc = area.alloc(area_bytes);
        if (rc) return rc;
    }
    size_t cursor = 0;
    const void* dptr;
    rc = mvs_stage_view(c, *mask, 1, (char*)area.ptr, &cursor, &dptr);
    if (rc) return rc;
    const unsigned char* dmask = (const unsigned char*)dptr;
    const long long sz = mask->mem == MVS_MEM_HOST ? (long long)Dm.ny * Dm.nx : (long long)mask->stride[0];
    const long long sy = mask->mem == MVS_MEM_HOST ? (long long)Dm.nx : (long long)mask->stride[1];
    unsigned char* dout = out_mem == MVS_MEM_HOST ? (unsigned char*)area.ptr + mask_bytes : (unsigned char*)out;

    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    const long long plane = (long long)Dm.ny * Dm.nx;
    for (long long k = 0; k < n_slabs(Dm.nz, planes); ++k) {
        const Slab sl = slab(k, Dm.nz, planes, halo);
        const FeatherOut result{nullptr, 0, dout, S.D};
        {
            const FeatherOut O = n_sets ? FeatherOut{sets[0], sl.h0, nullptr, S.D} : result;
            hipLaunchKernelGGL(feather_x_kernel, dim3(grid_blocks((sl.h1 - sl.h0) * Dm.ny * Dm.groups, kThreads)), dim3(kThreads), 0, c->stream, dmask, sz,
                               sy, Dm, sl.h0, sl.h1, w[2], S.P[2], O);
            MVS_HIP_TRY(c, hipGetLastError());
        }
        const unsigned int* cur = sets[0];
        if (pass_y) {
            const FeatherOut O = pass_z ? FeatherOut{sets[1], sl.h0, nullptr, S.D} : result;
            hipLaunchKernelGGL(feather_lines_kernel, dim3(grid_blocks((sl.h1 - sl.h0) * plane, kThreads)), dim3(kThreads), 0, c->stream, cur, sl.h0, Dm,
                               sl.h0, sl.h1, 1, w[1], S.P[1], O);
            MVS_HIP_TRY(c, hipGetLastError());
            cur = sets[1];
        }
        if (pass_z) {
            hipLaunchKernelGGL(feather_lines_kernel, dim3(grid_blocks((sl.z1 - sl.z0) * plane, kThreads)), dim3(kThreads), 0, c->stream, cur, sl.h0, Dm,
                               sl.z0, sl.z1, 0, w[0], S.P[0], result);
            MVS_HIP_TRY(c, hipGetLastError());
        }
    }
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    if (out_mem == MVS_MEM_HOST) MVS_HIP_TRY(c, hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return area_bytes ? area.release() : MVS_OK;
}
