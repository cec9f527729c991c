// mvs_dct_dev.h -- internal: the per-view lookup into the normalised DCT-entropy quality grids (weights.content_based_dct,
// weights.py:270-281 of the reference), shared by the standalone weights (mvs_dct_weights.hip) and the fused weighted
// average (fuse_kernel in mvs_fuse.hip).
#pragma once
#include "mvs_internal.h"

struct DctLookup {
    const float* q;        // normalised quality grids, [view][nb0][nb1][nb2]; NULL = no DCT factor
    int nb[3];             // blocks per axis (z, y, x)
    int nblocks;           // nb0 * nb1 * nb2
    double scale[3];       // 1 / ds
    double offset[3];      // -(ds - 1) / (2 ds)
};

// scipy.ndimage.affine_transform(Q_v, diag(1/ds), offset, order=1, mode="nearest") at chunk index p: the coordinate in
// double as scipy forms it (m * p + offset), clamped to [0, n-1], both taps of every axis always read (a NaN next to a
// zero-weight tap propagates as in scipy), second tap clamped to the last node.
__device__ __forceinline__ float dct_lookup(const DctLookup& L, int view, double pz, double py, double px) {
    const float* q = L.q + (long long)view * L.nblocks;
    const double p[3] = {pz, py, px};
    int i0[3], i1[3];
    double t[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double c = L.scale[d] * p[d] + L.offset[d];
        const double hi = (double)(L.nb[d] - 1);
        if (c < 0.0) c = 0.0;
        else if (c > hi) c = hi;
        const double f = floor(c);
        i0[d] = (int)f;
        i1[d] = i0[d] + 1 < L.nb[d] ? i0[d] + 1 : L.nb[d] - 1;
        t[d] = c - f;
    }
    double r = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int iz = a ? i1[0] : i0[0], iy = b ? i1[1] : i0[1], ix = e ? i1[2] : i0[2];
                const double w = (a ? t[0] : 1.0 - t[0]) * (b ? t[1] : 1.0 - t[1]) * (e ? t[2] : 1.0 - t[2]);
                r += w * (double)q[((long long)iz * L.nb[1] + iy) * L.nb[2] + ix];
            }
    return (float)r;
}

// the chunk-level fused weighted average of mvs_fuse.hip with the DCT factor (mvs_fuse_chunk_dct); `keep_start`: the caller
// recorded the context's start event before its own kernels (last_kernel_ms then covers the whole chunk)
// (arguments checked, context locked, device set by the entry)
int mvs_fuse_chunk_impl(MvsContext* c, const mvs_view_t* views, int32_t n_views, const mvs_fuse_opts_t* opts, void* out,
                        const DctLookup* dct, bool keep_start);
