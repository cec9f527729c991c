// Host-side run of csrc/mvs_affine_walk_dev.h: which voxels a (block, wave, lane) of the affine registration kernels visits.
// For every shape and pose, block_pos and walk_run are called for every block, wave and lane as a kernel's threads call them,
// and the callback records the voxel and its (fv, v, g, dy).  A plain triple loop over the crop through mvs_ar::coord2 / coord3,
// split and sample2 / sample3 gives the valid set and its values.  tests/test_affine_reg_host.py builds this with hipcc (no GPU
// needed) and asserts the counts of each line:
//   W <ndim> <nz> <ny> <nx> <pose> <blocks> <valid in the loop> <visited> <visited twice> <missing> <extra> <values that differ>
// Poses: the identity, and one of the size the GPU test draws (A - I of a few hundredths, t of a few tenths of a voxel), fixed
// below; it contracts y and x by 3 to 4 %, so that the last row and the last column of a crop -- which the identity can never
// sample -- map inside the moving crop and reach the callback.  Crops: seeded values, a NaN border on y and x of the moving crop
// wherever the axis has at least 8 voxels, and NaN voxels in both crops.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mvs_affine_walk_dev.h"

static unsigned s_state = 20250917u;
static unsigned next_u32() {
    s_state = s_state * 1664525u + 1013904223u;
    return s_state;
}
static float unit_f() { return (float)(next_u32() >> 8) / (float)(1 << 24); }
static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

static const double POSE_A3[9] = {1.0060943, -0.0207997, 0.0150090, 0.0188113, 0.9609793, -0.0260436, 0.0025568, -0.0063249, 0.9596640};
static const double POSE_T3[3] = {-0.3412176, 0.3517592, -0.2111168};
static const double POSE_A2[9] = {1.0, 0.0, 0.0, 0.0, 0.9713206, 0.0225448, 0.0, 0.0093502, 0.9628142};
static const double POSE_T2[3] = {0.0, -0.3435170, -0.2475004};
static const double IDENTITY[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
static const double ZERO[3] = {0.0, 0.0, 0.0};

struct Sample {
    int count = 0;
    float fv, v, g[3], dy;
};

template <int ND>
static bool run_case(const int64_t shape[3], int ipose) {
    const long long nz = shape[0], ny = shape[1], nx = shape[2], n = nz * ny * nx;
    std::vector<float> F(n), M(n);
    for (long long i = 0; i < n; ++i) {
        F[i] = unit_f();
        M[i] = unit_f() * 3.f - 1.f;
    }
    for (long long z = 0; z < nz; ++z)
        for (long long y = 0; y < ny; ++y)
            for (long long x = 0; x < nx; ++x)
                if ((ny >= 8 && (y == 0 || y == ny - 1)) || (nx >= 8 && (x == 0 || x == nx - 1))) M[(z * ny + y) * nx + x] = NAN;
    for (long long i = 0; i < n / 50; ++i) {
        F[next_u32() % (unsigned)n] = NAN;
        M[next_u32() % (unsigned)n] = i % 3 ? NAN : INFINITY;
    }

    mvs_aw::Walk W;
    const double* A = ipose == 0 ? IDENTITY : (ND == 3 ? POSE_A3 : POSE_A2);
    const long long nblocks = mvs_aw::set_geometry(&W, shape, A, ipose == 0 ? ZERO : (ND == 3 ? POSE_T3 : POSE_T2));
    W.fixed = F.data();
    W.moving = M.data();

    // what the threads of a launch of nblocks blocks visit
    std::vector<Sample> seen(n);
    long long twice = 0, wrong = 0;
    for (long long b = 0; b < nblocks; ++b)
        for (int wave = 0; wave < mvs_aw::WAVES; ++wave)
            for (int lane = 0; lane < 64; ++lane) {
                const mvs_aw::BlockPos bp = mvs_aw::block_pos(W, b);
                const long long x = (long long)bp.xb * 64 + lane;
                const double dxd = (double)x - W.c[2];
                const double dzd = ND == 3 ? (double)bp.z - W.c[0] : 0.0;
                mvs_aw::walk_run<ND>(W, bp.z, bp.yc, wave, x, dzd, dxd, [&](float fv, float v, const float* g, float dy) {
                    const long long y = (long long)((double)dy + W.c[1]);      // dy = y - c_y is a small half-integer: exact
                    if (bp.z < 0 || bp.z >= nz || y < 0 || y >= ny || x >= nx) {
                        ++wrong;
                        return;
                    }
                    Sample& s = seen[(bp.z * ny + y) * nx + x];
                    if (s.count++) ++twice;
                    s.fv = fv;
                    s.v = v;
                    s.dy = dy;
                    for (int k = 0; k < ND; ++k) s.g[k] = g[k];
                });
            }

    // the plain loop
    long long valid = 0, visited = 0, missing = 0, extra = wrong, differ = 0;
    for (long long z = 0; z < nz; ++z)
        for (long long y = 0; y < ny; ++y)
            for (long long x = 0; x < nx; ++x) {
                const long long at = (z * ny + y) * nx + x;
                const double d[3] = {(double)z - W.c[0], (double)y - W.c[1], (double)x - W.c[2]};
                float v = 0.f, g[3] = {0.f, 0.f, 0.f};
                bool ok = mvs_ar::finite_f(F[at]);
                if (ok && ND == 3) {
                    long long i0[3];
                    float fr[3];
                    for (int k = 0; k < 3 && ok; ++k) ok = mvs_ar::split(mvs_ar::coord3(W.A + 3 * k, d[0], d[1], d[2], W.o[k]), W.n[k], &i0[k], &fr[k]);
                    if (ok) {
                        float taps[8];
                        for (int t = 0; t < 8; ++t) taps[t] = M[((i0[0] + (t >> 2)) * ny + i0[1] + (t >> 1 & 1)) * nx + i0[2] + (t & 1)];
                        ok = mvs_ar::sample3(taps, fr[0], fr[1], fr[2], &v, g);
                    }
                } else if (ok) {
                    long long i0[2];
                    float fr[2];
                    for (int k = 0; k < 2 && ok; ++k) ok = mvs_ar::split(mvs_ar::coord2(W.A + 3 * (k + 1) + 1, d[1], d[2], W.o[k + 1]), W.n[k + 1], &i0[k], &fr[k]);
                    if (ok) {
                        float taps[4];
                        for (int t = 0; t < 4; ++t) taps[t] = M[(i0[0] + (t >> 1)) * nx + i0[1] + (t & 1)];
                        ok = mvs_ar::sample2(taps, fr[0], fr[1], &v, g);
                    }
                }
                const Sample& s = seen[at];
                valid += ok;
                visited += s.count > 0;
                if (ok && !s.count) ++missing;
                if (!ok && s.count) ++extra;
                if (ok && s.count) {
                    bool same = same_bits(s.fv, F[at]) && same_bits(s.v, v) && same_bits(s.dy, (float)d[1]);
                    for (int k = 0; k < ND; ++k) same = same && same_bits(s.g[k], g[k]);
                    if (!same) ++differ;
                }
            }
    printf("W %d %lld %lld %lld %d %lld %lld %lld %lld %lld %lld %lld\n", ND, nz, ny, nx, ipose, nblocks, valid, visited, twice, missing, extra, differ);
    return twice == 0 && missing == 0 && extra == 0 && differ == 0;
}

int main() {
    const int64_t shapes2[8][3] = {{1, 1, 1}, {1, 5, 63}, {1, 5, 64}, {1, 5, 65}, {1, 127, 3}, {1, 128, 3}, {1, 129, 3}, {1, 257, 130}};
    const int64_t shapes3[2][3] = {{3, 4, 130}, {2, 129, 65}};
    bool ok = true;
    for (int ipose = 0; ipose < 2; ++ipose) {
        for (const auto& s : shapes2) ok = run_case<2>(s, ipose) && ok;
        for (const auto& s : shapes3) ok = run_case<3>(s, ipose) && ok;
    }
    printf(ok ? "done\n" : "FAILED\n");
    return ok ? 0 : 1;
}
