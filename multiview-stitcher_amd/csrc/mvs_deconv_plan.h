// mvs_deconv_plan.h -- host-only pure C++ of the multi-view deconvolution (mvs_deconv.hip): everything mvs_mv_deconv decides without
// the device -- the tile constants of its kernels, its limits and grid rule, the geometry of one call (padded kernel row, anchors,
// launch extents, the work-area layout) and the tap tables the kernels read.  No HIP: tests/native/deconv_plan_host_test.cpp compiles
// it with the host compiler under the address and undefined-behaviour sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "mvs_stack_frame.h"

namespace mvs_deconv_plan {

constexpr int GX = 8, GY = 8;       // threads of a general-path workgroup (one wave)
constexpr int RX = 8, RY = 4;       // outputs per thread along x / y
constexpr int TX = GX * RX, TY = GY * RY;   // output tile 64 x 32
constexpr int KMAX = 63;            // largest kernel extent per axis of the general path
constexpr int kInitBlocks = 1024;   // workgroups of the init kernel = block maxima the peak kernel reduces

// workgroups of the element-wise grid-stride kernels (256 lanes, one voxel each and step)
inline int grid_for(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 256 * 32)); }

// scipy.ndimage.convolve's origin in correlation order, odd and even extents alike
constexpr int anchor(int k) { return k - 1 - k / 2; }

struct Plan {
    bool separable;                 // three 1-D passes per convolution instead of the general direct one
    int nz, ny, nx, kz, ky, kx;
    int kxp;                        // kx padded to a multiple of 4 (the general path reads its taps four at a time)
    int az, ay, ax;
    long long S;                    // voxels of one view
    long long kvol, kvolp, ksep;    // taps of one kernel: as given, with padded rows, as separable factors
    size_t taps;                    // floats of the whole tap table: 2 sets x V kernels
    unsigned grid_x, grid_y, grid_z;   // the general path: a workgroup per TX x TY tile of every z plane ...
    size_t lds_bytes;               // ... and its dynamic LDS, the window of one plane: (TY + ky - 1) rows of TX + kxp floats
    // the work area: psi | wr | two pass buffers (separable) | two masks (erosion) | block maxima | peak | taps | host result staging
    size_t off_psi, off_wr, off_a, off_b, off_m0, off_m1, off_bm, off_pk, off_tp, off_out, total;
    mvs_stack_frame::OutBox box;
};

// The plan of one call.  kInvalidArg for an extent below 1 (or a shape beyond 32 bits), kUnsupported for a kernel extent above KMAX:
// MVS_ERR_INVALID_ARG and MVS_ERR_UNSUPPORTED of include/mvs_hip.h (mvs_deconv.hip asserts it).
constexpr int kOk = 0, kInvalidArg = -1, kUnsupported = -4;

inline int make_plan(const int64_t shape[3], const int64_t ksize[3], int n_views, bool separable, bool erosion, const int64_t trim[3],
                     int32_t out_dtype, bool host_result, Plan* p) {
    for (int k = 0; k < 3; ++k) {
        if (shape[k] < 1 || shape[k] > 0x7fffffffLL || ksize[k] < 1) return kInvalidArg;
        if (ksize[k] > KMAX) return kUnsupported;
    }
    p->separable = separable;
    p->nz = (int)shape[0], p->ny = (int)shape[1], p->nx = (int)shape[2];
    p->kz = (int)ksize[0], p->ky = (int)ksize[1], p->kx = (int)ksize[2];
    p->kxp = (p->kx + 3) & ~3;
    p->az = anchor(p->kz), p->ay = anchor(p->ky), p->ax = anchor(p->kx);
    p->S = (long long)p->nz * p->ny * p->nx;
    p->kvol = (long long)p->kz * p->ky * p->kx, p->kvolp = (long long)p->kz * p->ky * p->kxp, p->ksep = p->kz + p->ky + p->kx;
    p->taps = (size_t)(2 * n_views * (separable ? p->ksep : p->kvolp));
    p->grid_x = (p->nx + TX - 1) / TX, p->grid_y = (p->ny + TY - 1) / TY, p->grid_z = p->nz;
    p->lds_bytes = (size_t)(TY + p->ky - 1) * (TX + p->kxp) * 4;
    p->box = mvs_stack_frame::out_box(shape, trim, out_dtype);

    // float volumes are packed; the masks, the peak, the taps and whatever follows them start on 256-byte boundaries of the area
    const size_t fS = (size_t)p->S * 4;
    mvs_stack_frame::Layout L;
    p->off_psi = L.take(fS, 4);
    p->off_wr = L.take(fS, 4);
    p->off_a = L.take(separable ? fS : 0, 4);
    p->off_b = L.take(separable ? fS : 0, 4);
    p->off_m0 = L.take(erosion ? (size_t)p->S : 0, 256);
    p->off_m1 = L.take(erosion ? (size_t)p->S : 0, 256);
    p->off_bm = L.take(kInitBlocks * 4, 4);
    p->off_pk = L.take(4, 256);
    p->off_tp = L.take(p->taps * 4, 256);
    p->off_out = L.take(host_result ? p->box.out_bytes : 0, 1);
    p->total = L.total;
    return kOk;
}

// The host tap tables in correlation order (the kernels flipped on every axis): general [set][v][kz][ky][kxp] (x zero-padded) from
// kernels1 / kernels2, separable [set][v][kz + ky + kx] (each factor reversed on its own) from sep1 / sep2.  sep_cval (separable
// only), per view: what the y and the z pass of the back projection read outside the array -- cval 1 times the sums of the factors
// of the passes before them, (sum x, sum x * sum y) of set 2.
inline void make_taps(const Plan& p, int n_views, const float* kernels1, const float* kernels2, const float* sep1, const float* sep2,
                      std::vector<float>* htaps, std::vector<float>* sep_cval) {
    const int V = n_views, kz = p.kz, ky = p.ky, kx = p.kx, kxp = p.kxp;
    const long long kvol = p.kvol, kvolp = p.kvolp, ksep = p.ksep;
    sep_cval->clear();
    if (p.separable) {
        htaps->resize(2 * V * ksep);
        sep_cval->resize(2 * (size_t)V);
        for (int s = 0; s < 2; ++s)
            for (int v = 0; v < V; ++v) {
                const float* src = (s ? sep2 : sep1) + v * ksep;
                float* dst = htaps->data() + (s * V + v) * ksep;
                const int len[3] = {kz, ky, kx};
                int off = 0;
                for (int ax_ = 0; ax_ < 3; ++ax_) {
                    for (int j = 0; j < len[ax_]; ++j) dst[off + j] = src[off + len[ax_] - 1 - j];
                    off += len[ax_];
                }
                if (s == 1) {
                    double sx = 0.0, sy = 0.0;
                    for (int j = 0; j < kx; ++j) sx += src[kz + ky + j];
                    for (int j = 0; j < ky; ++j) sy += src[kz + j];
                    (*sep_cval)[2 * v] = (float)sx;
                    (*sep_cval)[2 * v + 1] = (float)(sx * sy);
                }
            }
    } else {
        htaps->assign(2 * V * kvolp, 0.f);
        for (int s = 0; s < 2; ++s)
            for (int v = 0; v < V; ++v) {
                const float* src = (s ? kernels2 : kernels1) + v * kvol;
                float* dst = htaps->data() + (s * V + v) * kvolp;
                for (int z = 0; z < kz; ++z)
                    for (int y = 0; y < ky; ++y)
                        for (int x = 0; x < kx; ++x)
                            dst[((long long)z * ky + y) * kxp + x] = src[((long long)(kz - 1 - z) * ky + (ky - 1 - y)) * kx + (kx - 1 - x)];
            }
    }
}

}  // namespace mvs_deconv_plan
