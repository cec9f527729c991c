// mvs_multiband.hip -- multi-band pyramid fusion (Burt & Adelson 1983): every band of the views' disagreement is blended over a zone as
// wide as its wavelength, so detail comes from one view and illumination is blended widely.  The definition (include/mvs_hip.h,
// mvs_multiband_fuse) in short:
//   prepare   F0 = sum_v W_v I_v (the normalised weighted average), D_v = I_v - F0 where the view is finite, the winner map
//             (argmax_v of the masked weights, one byte) whose planes A_v = (winner == v) are the hard-seam masks
//   REDUCE    gD_v, gA_v of level l + 1 from level l: taps [1 4 6 4 1] / 16 along every decimated axis, samples kept at GLOBAL even
//             indices, samples outside the array 0, separable in the order z, y, x
//   collapse  r_l = sum_v (gA_v / sum_u gA_u) (gD_v - EXPAND(gD_v of level l + 1)) + EXPAND(r_{l+1}), from the top level down; level 0
//             is fused with F0 + r_0, the halo trim and the cast
// Every sum has one fixed order that does not depend on where a sample sits in a tile or a chunk (samples outside an array enter the
// same expression as zeros), so equal inputs give equal bits and a voxel gets the same bits in any chunk.  No float atomics.
// Level geometry: mvs_multiband_plan.h.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "mvs_intensity_dev.h"
#include "mvs_internal.h"
#include "mvs_multiband_plan.h"
#include "mvs_stack_frame.h"

namespace {

namespace mp = mvs_multiband_plan;

struct Level {      // one pyramid level: global index of the first sample and extent per axis z, y, x
    int s[3];
    int n[3];
};

struct Plane {      // one plane of a level: float samples, or (A_v of level 0) the winner map compared with a view index
    const float* f;
    const unsigned char* win;
    int view;
};

constexpr int DEC_Z = 1, DEC_Y = 2, DEC_X = 4;

// the three expressions of the pyramid; the library is built without contraction, so each is the roundings it shows
__device__ __forceinline__ float reduce5(float a0, float a1, float a2, float a3, float a4) {
    return (6.f * a2 + 4.f * (a1 + a3) + (a0 + a4)) * 0.0625f;
}
__device__ __forceinline__ float expand_even(float a, float b, float c) { return (6.f * b + (a + c)) * 0.125f; }
__device__ __forceinline__ float expand_odd(float b, float c) { return (b + c) * 0.5f; }

// sample of a plane at GLOBAL indices; 0 outside the level's extent
__device__ __forceinline__ float sample(const Plane& p, const Level& lv, int gz, int gy, int gx) {
    const int z = gz - lv.s[0], y = gy - lv.s[1], x = gx - lv.s[2];
    if ((unsigned)z >= (unsigned)lv.n[0] || (unsigned)y >= (unsigned)lv.n[1] || (unsigned)x >= (unsigned)lv.n[2]) return 0.f;
    const long long i = ((long long)z * lv.n[1] + y) * lv.n[2] + x;
    return p.f ? p.f[i] : (p.win[i] == p.view ? 1.f : 0.f);
}

// ---- prepare ---------------------------------------------------------------------------------------------------------------------
// Four consecutive voxels per lane and step (16-byte loads and stores when `vec`: S a multiple of 4 and 16-byte aligned stacks).
// Three walks over the views in view order: the weight sum and the winner, F0, D_v.  `flag` is raised (integer OR) when any D != 0.
__global__ __launch_bounds__(mp::kThreads) void mb_prepare_kernel(const float* __restrict__ views, const float* __restrict__ weights, int V,
                                                                  long long S, int vec, float* __restrict__ F0, float* __restrict__ D,
                                                                  unsigned char* __restrict__ win, int* __restrict__ flag) {
    __shared__ int any;
    if (threadIdx.x == 0) any = 0;
    __syncthreads();
    int mine = 0;
    const long long groups = (S + 3) / 4;
    for (long long g = (long long)blockIdx.x * mp::kThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * mp::kThreads) {
        const long long i0 = g * 4;
        const int cnt = (int)(S - i0 < 4 ? S - i0 : 4);
        auto load4 = [&](const float* base, float out[4]) {
            if (vec) {
                const float4 q = *reinterpret_cast<const float4*>(base + i0);
                out[0] = q.x, out[1] = q.y, out[2] = q.z, out[3] = q.w;
            } else {
                for (int k = 0; k < 4; ++k) out[k] = k < cnt ? base[i0 + k] : 0.f;
            }
        };
        auto store4 = [&](float* base, const float in[4]) {
            if (vec) {
                *reinterpret_cast<float4*>(base + i0) = make_float4(in[0], in[1], in[2], in[3]);
            } else {
                for (int k = 0; k < cnt; ++k) base[i0 + k] = in[k];
            }
        };
        float sw[4] = {0.f, 0.f, 0.f, 0.f}, bw[4] = {0.f, 0.f, 0.f, 0.f}, f0[4] = {0.f, 0.f, 0.f, 0.f};
        int best[4] = {mp::kNoView, mp::kNoView, mp::kNoView, mp::kNoView};
        float x[4], b[4];
        for (int v = 0; v < V; ++v) {
            load4(views + v * S, x);
            load4(weights + v * S, b);
            for (int k = 0; k < 4; ++k) {
                const float w = isfinite(x[k]) ? b[k] : 0.f;
                sw[k] = sw[k] + w;
                if (w > bw[k]) bw[k] = w, best[k] = v;      // strict: the lowest index wins ties
            }
        }
        bool cov[4];
        for (int k = 0; k < 4; ++k) {
            cov[k] = sw[k] > 0.f;
            if (!cov[k]) best[k] = mp::kNoView;
        }
        for (int v = 0; v < V; ++v) {
            load4(views + v * S, x);
            load4(weights + v * S, b);
            for (int k = 0; k < 4; ++k) {
                const bool m = isfinite(x[k]);
                if (cov[k] && m) f0[k] = f0[k] + (b[k] / sw[k]) * x[k];
            }
        }
        store4(F0, f0);
        for (int v = 0; v < V; ++v) {
            load4(views + v * S, x);
            float d[4];
            for (int k = 0; k < 4; ++k) {
                d[k] = isfinite(x[k]) ? x[k] - f0[k] : 0.f;
                if (k < cnt && d[k] != 0.f) mine = 1;
            }
            store4(D + v * S, d);
        }
        if (vec) {
            *reinterpret_cast<uchar4*>(win + i0) = make_uchar4((unsigned char)best[0], (unsigned char)best[1], (unsigned char)best[2], (unsigned char)best[3]);
        } else {
            for (int k = 0; k < cnt; ++k) win[i0 + k] = (unsigned char)best[k];
        }
    }
    if (mine) atomicOr(&any, 1);
    __syncthreads();
    if (threadIdx.x == 0 && any) atomicOr(flag, 1);
}

// ---- REDUCE ----------------------------------------------------------------------------------------------------------------------
// One launch per level for the 2 V planes gD_v, gA_v.  A workgroup step = one plane, one coarse z, a tile of kTileY x kTileX coarse
// samples: the z pass runs while the window (tile x 2 + 3 along a decimated axis) is read into LDS, the y pass LDS -> LDS, the x pass
// LDS -> global: a level costs one read and a quarter or an eighth of a write.  Returns at once when the views agree everywhere.
struct ReduceArgs {
    const float* d_in;          // V planes of level l
    const float* a_in;          // V planes of level l, NULL at level 0 (the winner map)
    const unsigned char* win;
    float* d_out;               // V planes of level l + 1
    float* a_out;
    Level in, out;
    int dec;                    // DEC_* bits of the axes this step decimates
    int V;
    long long s_in, s_out;      // samples of a plane
};

__global__ __launch_bounds__(mp::kThreads) void mb_reduce_kernel(ReduceArgs a, const int* __restrict__ flag) {
    __shared__ float win1[mp::kWinY][mp::kWinX];
    __shared__ float win2[mp::kTileY][mp::kWinX];
    if (*flag == 0) return;
    const bool dz = a.dec & DEC_Z, dy = a.dec & DEC_Y, dx = a.dec & DEC_X;
    const int wy = dy ? mp::kWinY : mp::kTileY, wx = dx ? mp::kWinX : mp::kTileX;
    const long long ty_n = mp::tiles_y(a.out.n[1]), tx_n = mp::tiles_x(a.out.n[2]);
    const long long steps = 2LL * a.V * a.out.n[0] * ty_n * tx_n;
    for (long long step = blockIdx.x; step < steps; step += gridDim.x) {
        const int tx = (int)(step % tx_n), ty = (int)(step / tx_n % ty_n), oz = (int)(step / (tx_n * ty_n) % a.out.n[0]);
        const int p = (int)(step / (tx_n * ty_n * a.out.n[0]));
        const int v = p < a.V ? p : p - a.V;
        Plane src;
        src.f = p < a.V ? a.d_in + v * a.s_in : (a.a_in ? a.a_in + v * a.s_in : nullptr);
        src.win = a.win;
        src.view = v;
        float* dst = (p < a.V ? a.d_out : a.a_out) + v * a.s_out;
        const int kz = a.out.s[0] + oz, ky0 = a.out.s[1] + ty * mp::kTileY, kx0 = a.out.s[2] + tx * mp::kTileX;   // global coarse indices
        const int gy0 = dy ? 2 * ky0 - 2 : ky0, gx0 = dx ? 2 * kx0 - 2 : kx0;
        for (int i = threadIdx.x; i < wy * wx; i += mp::kThreads) {
            const int r = i / wx, c = i % wx;
            const int gy = gy0 + r, gx = gx0 + c;
            win1[r][c] = dz ? reduce5(sample(src, a.in, 2 * kz - 2, gy, gx), sample(src, a.in, 2 * kz - 1, gy, gx), sample(src, a.in, 2 * kz, gy, gx),
                                      sample(src, a.in, 2 * kz + 1, gy, gx), sample(src, a.in, 2 * kz + 2, gy, gx))
                            : sample(src, a.in, kz, gy, gx);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < mp::kTileY * wx; i += mp::kThreads) {
            const int r = i / wx, c = i % wx;
            win2[r][c] = dy ? reduce5(win1[2 * r][c], win1[2 * r + 1][c], win1[2 * r + 2][c], win1[2 * r + 3][c], win1[2 * r + 4][c]) : win1[r][c];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < mp::kTileY * mp::kTileX; i += mp::kThreads) {
            const int r = i / mp::kTileX, c = i % mp::kTileX;
            const int oy = ty * mp::kTileY + r, ox = tx * mp::kTileX + c;
            if (oy < a.out.n[1] && ox < a.out.n[2]) {
                const float val = dx ? reduce5(win2[r][2 * c], win2[r][2 * c + 1], win2[r][2 * c + 2], win2[r][2 * c + 3], win2[r][2 * c + 4]) : win2[r][c];
                dst[((long long)oz * a.out.n[1] + oy) * a.out.n[2] + ox] = val;
            }
        }
        __syncthreads();      // (the next step refills win1)
    }
}

// ---- collapse --------------------------------------------------------------------------------------------------------------------
// EXPAND of a level-(l+1) plane at one level-l sample, separable in the order z, y, x: the x rule over the y rule over the z rule.
// Global even g = 2K: (c[K-1] + 6 c[K] + c[K+1]) / 8; odd g = 2K + 1: (c[K] + c[K+1]) / 2; missing coarse samples are 0.
__device__ __forceinline__ float expand_z(const Plane& c, const Level& up, int dec, int gz, int ky, int kx) {
    if (!(dec & DEC_Z)) return sample(c, up, gz, ky, kx);
    const int k = gz >> 1;
    if (gz & 1) return expand_odd(sample(c, up, k, ky, kx), sample(c, up, k + 1, ky, kx));
    return expand_even(sample(c, up, k - 1, ky, kx), sample(c, up, k, ky, kx), sample(c, up, k + 1, ky, kx));
}
__device__ __forceinline__ float expand_y(const Plane& c, const Level& up, int dec, int gz, int gy, int kx) {
    if (!(dec & DEC_Y)) return expand_z(c, up, dec, gz, gy, kx);
    const int k = gy >> 1;
    if (gy & 1) return expand_odd(expand_z(c, up, dec, gz, k, kx), expand_z(c, up, dec, gz, k + 1, kx));
    return expand_even(expand_z(c, up, dec, gz, k - 1, kx), expand_z(c, up, dec, gz, k, kx), expand_z(c, up, dec, gz, k + 1, kx));
}
__device__ __forceinline__ float expand(const float* c, const Level& up, int dec, int gz, int gy, int gx) {
    const Plane p{c, nullptr, 0};
    if (!(dec & DEC_X)) return expand_y(p, up, dec, gz, gy, gx);
    const int k = gx >> 1;
    if (gx & 1) return expand_odd(expand_y(p, up, dec, gz, gy, k), expand_y(p, up, dec, gz, gy, k + 1));
    return expand_even(expand_y(p, up, dec, gz, gy, k - 1), expand_y(p, up, dec, gz, gy, k), expand_y(p, up, dec, gz, gy, k + 1));
}

struct CollapseArgs {
    const float* d;             // gD of level l, V planes
    const float* a;             // gA of level l, V planes; NULL at level 0 (the winner map)
    const unsigned char* win;
    const float* d_up;          // gD of level l + 1, V planes; NULL at the top level
    const float* r_up;          // r of level l + 1; NULL at the top level
    Level cur, up;
    int dec;                    // DEC_* bits of the axes level l + 1 decimates
    int V;
    long long s_cur, s_up;
};

// r_l at the level-l sample (z, y, x) (local indices): views in view order; a view whose mask is 0 here adds nothing and is skipped
__device__ __forceinline__ float collapse_sample(const CollapseArgs& a, int z, int y, int x) {
    const long long i = ((long long)z * a.cur.n[1] + y) * a.cur.n[2] + x;
    const int gz = a.cur.s[0] + z, gy = a.cur.s[1] + y, gx = a.cur.s[2] + x;
    float acc = 0.f;
    if (!a.a) {     // level 0: the mask is the winner map, A-hat is 1 for the winner
        const int v = a.win[i];
        if (v != mp::kNoView) {
            float lap = a.d[v * a.s_cur + i];
            if (a.d_up) lap = lap - expand(a.d_up + v * a.s_up, a.up, a.dec, gz, gy, gx);
            acc = lap;
        }
    } else {
        float sum = 0.f;
        for (int v = 0; v < a.V; ++v) sum = sum + a.a[v * a.s_cur + i];
        if (sum > 0.f)
            for (int v = 0; v < a.V; ++v) {
                const float m = a.a[v * a.s_cur + i];
                if (m == 0.f) continue;
                float lap = a.d[v * a.s_cur + i];
                if (a.d_up) lap = lap - expand(a.d_up + v * a.s_up, a.up, a.dec, gz, gy, gx);
                acc = acc + (m / sum) * lap;
            }
    }
    return a.r_up ? acc + expand(a.r_up, a.up, a.dec, gz, gy, gx) : acc;
}

__global__ __launch_bounds__(mp::kThreads) void mb_collapse_kernel(CollapseArgs a, float* __restrict__ r, const int* __restrict__ flag) {
    if (*flag == 0) return;
    const int ny = a.cur.n[1], nx = a.cur.n[2];
    for (long long i = (long long)blockIdx.x * mp::kThreads + threadIdx.x; i < a.s_cur; i += (long long)gridDim.x * mp::kThreads) {
        const int x = (int)(i % nx), y = (int)(i / nx % ny), z = (int)(i / ((long long)nx * ny));
        r[i] = collapse_sample(a, z, y, x);
    }
}

// level 0 with the epilogue: cov ? F0 + r_0 : 0 over the chunk minus its halo, cast (integers: round half to even, saturate)
template <typename T>
__global__ __launch_bounds__(mp::kThreads) void mb_collapse_out_kernel(CollapseArgs a, const float* __restrict__ F0, int t0, int t1, int t2, int oz,
                                                                       int oy, int ox, T* __restrict__ out, const int* __restrict__ flag) {
    const bool chain = *flag != 0;
    const long long n = (long long)oz * oy * ox;
    for (long long i = (long long)blockIdx.x * mp::kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * mp::kThreads) {
        const int x = (int)(i % ox) + t2, y = (int)(i / ox % oy) + t1, z = (int)(i / ((long long)ox * oy)) + t0;
        const long long j = ((long long)z * a.cur.n[1] + y) * a.cur.n[2] + x;
        float val = 0.f;
        if (a.win[j] != mp::kNoView) val = chain ? F0[j] + collapse_sample(a, z, y, x) : F0[j];
        if (sizeof(T) == 4)
            out[i] = (T)val;
        else
            out[i] = (T)intensity_saturate(val, sizeof(T) == 1 ? 255.f : 65535.f);
    }
}

Level level_of(const mp::Plan& p, int l) {
    Level lv;
    for (int d = 0; d < 3; ++d) lv.s[d] = (int)p.axis[d].start[l], lv.n[d] = (int)p.axis[d].n[l];
    return lv;
}

int dec_of(const mp::Plan& p, int l) {
    return (p.axis[0].decimated[l] ? DEC_Z : 0) | (p.axis[1].decimated[l] ? DEC_Y : 0) | (p.axis[2].decimated[l] ? DEC_X : 0);
}

const char* const NAME = "mvs_multiband_fuse";

// One mvs_multiband_fuse call: its arguments, the frame, the plan and the work area laid out over it.  The steps below run in the
// order of the entry point.
struct MultibandCall {
    const float *views, *weights;
    int V;
    const int64_t* shape;
    int ndim;
    const mvs_multiband_opts_t* opts;
    void* out;
    int32_t out_mem;
    MvsStackFrame F;
    mp::Plan plan;
    mvs_stack_frame::OutBox box;
    mp::WorkArea area;

    int L() const { return plan.top; }
    int* flag() const { return (int*)(F.W + area.flag); }
    float* F0() const { return (float*)(F.W + area.f0); }
    unsigned char* win() const { return (unsigned char*)(F.W + area.win); }
    float* gD(int l) const { return (float*)(F.W + area.d[l]); }
    float* gA(int l) const { return (float*)(F.W + area.a[l]); }
    float* r(int l) const { return (float*)(F.W + area.r[l]); }
};

// argument checks (they need no device) and the plan
int mb_check_and_plan(MvsContext* c0, MultibandCall& K) {
    const mvs_multiband_opts_t* opts = K.opts;
    if (!K.views || !K.weights || !K.shape || !opts || !K.out) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_multiband_fuse: NULL argument");
    if (K.V < 1 || K.V > mp::kMaxViews) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_multiband_fuse: n_views must be in 1 .. %d", mp::kMaxViews);
    if (K.ndim != 2 && K.ndim != 3) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_multiband_fuse: ndim must be 2 or 3");
    for (int k = 0; k < 3; ++k)
        if (opts->levels[k] < 0 || opts->levels[k] > mp::kMaxLevels)
            return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "mvs_multiband_fuse: levels[%d] = %d is outside 0 .. %d", k, (int)opts->levels[k], mp::kMaxLevels);
    if (int rc = mvs_stack_check_out(c0, NAME, K.out_mem, opts->out_dtype)) return rc;
    if (K.ndim == 2 && (K.shape[0] != 1 || opts->levels[0] != 0 || opts->trim[0] != 0))
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_multiband_fuse: 2D data has shape[0] == 1, levels[0] == 0 and trim[0] == 0");
    if (!mp::make_plan(opts->levels, opts->index_origin, K.shape, &K.plan))
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "mvs_multiband_fuse: a shape or an index_origin is out of range");
    for (int k = 0; k < 3; ++k)
        if (int rc = mvs_stack_check_trim(c0, NAME, K.shape, opts->trim, k)) return rc;
    if (int rc = mvs_stack_check_size(c0, NAME, K.plan.size[0], K.V)) return rc;
    K.box = mvs_stack_frame::out_box(K.shape, opts->trim, opts->out_dtype);
    K.area = mp::work_area(K.plan, K.V, K.out_mem == MVS_MEM_HOST ? K.box.out_bytes : 0);
    return MVS_OK;
}

// F0, D_v (= gD of level 0), the winner map and the flag
int mb_prepare(MultibandCall& K) {
    MvsContext* c = K.F.c;
    const long long S = K.plan.size[0];
    MVS_HIP_TRY(c, hipMemsetAsync(K.flag(), 0, mp::kFlagBytes, c->stream));
    const int vec = (S % 4 == 0) && ((uintptr_t)K.views % 16 == 0) && ((uintptr_t)K.weights % 16 == 0);
    hipLaunchKernelGGL(mb_prepare_kernel, dim3(mp::grid_blocks((S + 3) / 4, mp::kThreads)), dim3(mp::kThreads), 0, c->stream, K.views, K.weights, K.V, S, vec,
                       K.F0(), K.gD(0), K.win(), K.flag());
    MVS_HIP_TRY(c, hipGetLastError());
    return MVS_OK;
}

// gD, gA of levels 1 .. L, each from the level below
int mb_reduce_levels(MultibandCall& K) {
    MvsContext* c = K.F.c;
    for (int l = 0; l < K.L(); ++l) {
        ReduceArgs a{};
        a.d_in = K.gD(l);
        a.a_in = l ? K.gA(l) : nullptr;
        a.win = K.win();
        a.d_out = K.gD(l + 1);
        a.a_out = K.gA(l + 1);
        a.in = level_of(K.plan, l);
        a.out = level_of(K.plan, l + 1);
        a.dec = dec_of(K.plan, l);
        a.V = K.V;
        a.s_in = K.plan.size[l];
        a.s_out = K.plan.size[l + 1];
        const long long steps = 2LL * K.V * a.out.n[0] * mp::tiles_y(a.out.n[1]) * mp::tiles_x(a.out.n[2]);
        hipLaunchKernelGGL(mb_reduce_kernel, dim3(mp::grid_blocks(steps, 1)), dim3(mp::kThreads), 0, c->stream, a, (const int*)K.flag());
        MVS_HIP_TRY(c, hipGetLastError());
    }
    return MVS_OK;
}

// what the collapse of level l reads
CollapseArgs collapse_args(const MultibandCall& K, int l) {
    const int L = K.L();
    CollapseArgs a{};
    a.d = K.gD(l);
    a.a = l ? K.gA(l) : nullptr;
    a.win = K.win();
    a.d_up = l < L ? K.gD(l + 1) : nullptr;
    a.r_up = l < L ? K.r(l + 1) : nullptr;
    a.cur = level_of(K.plan, l);
    a.up = level_of(K.plan, l < L ? l + 1 : l);
    a.dec = l < L ? dec_of(K.plan, l) : 0;
    a.V = K.V;
    a.s_cur = K.plan.size[l];
    a.s_up = l < L ? K.plan.size[l + 1] : 0;
    return a;
}

// r of levels L .. 1, from the top down
int mb_collapse_levels(MultibandCall& K) {
    MvsContext* c = K.F.c;
    for (int l = K.L(); l > 0; --l) {
        const CollapseArgs a = collapse_args(K, l);
        hipLaunchKernelGGL(mb_collapse_kernel, dim3(mp::grid_blocks(a.s_cur, mp::kThreads)), dim3(mp::kThreads), 0, c->stream, a, K.r(l), (const int*)K.flag());
        MVS_HIP_TRY(c, hipGetLastError());
    }
    return MVS_OK;
}

// level 0 with the epilogue: F0 + r_0, trimmed and cast, where the frame wants the result
int mb_level0_out(MultibandCall& K) {
    MvsContext* c = K.F.c;
    const CollapseArgs a = collapse_args(K, 0);
    const int oz = (int)K.box.oz, oy = (int)K.box.oy, ox = (int)K.box.ox;
    const int grid = mp::grid_blocks(K.box.oz * K.box.oy * K.box.ox, mp::kThreads);
    const int t0 = (int)K.opts->trim[0], t1 = (int)K.opts->trim[1], t2 = (int)K.opts->trim[2];
    mvs_dispatch_dtype(K.opts->out_dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(mb_collapse_out_kernel<T>, dim3(grid), dim3(mp::kThreads), 0, c->stream, a, (const float*)K.F0(), t0, t1, t2, oz, oy, ox,
                           (T*)K.F.dout, (const int*)K.flag());
    });
    MVS_HIP_TRY(c, hipGetLastError());
    return MVS_OK;
}

}  // namespace

extern "C" int mvs_multiband_fuse(int device, const float* views, const float* weights, int32_t n_views, const int64_t shape[3], int32_t ndim,
                                  const mvs_multiband_opts_t* opts, void* out, int32_t out_mem) {
    MultibandCall K{views, weights, n_views, shape, ndim, opts, out, out_mem};
    int rc = mb_check_and_plan(mvs_ctx(device), K);
    if (!rc) rc = K.F.begin(device);
    if (!rc) rc = K.F.reserve(K.area.total, K.area.out, out, out_mem, K.box.out_bytes);
    if (!rc) rc = mb_prepare(K);
    if (!rc) rc = mb_reduce_levels(K);
    if (!rc) rc = mb_collapse_levels(K);
    if (!rc) rc = mb_level0_out(K);
    return rc ? rc : K.F.finish();
}
