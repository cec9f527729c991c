// Host-side run of csrc/mvs_affine_reg_dev.h (its functions are __host__ __device__): seeded taps, fractions and coordinates go
// through the per-sample routines and every input and result is printed bit for bit.  tests/test_affine_reg_host.py builds
// this with hipcc (no GPU needed), feeds the printed inputs to the float32 mode of tests/affine_reg_oracle.py and compares
// the bits.  Lines:
//   S3 <8 taps> <fz fy fx> <ok> <v> <gz gy gx>      S2 <4 taps> <fy fx> <ok> <v> <gy gx>          (float32 as 8 hex digits)
//   P <p> <n> <ok> <i0> <f>                          C3 <a0 a1 a2 d0 d1 d2 o> <p>   C2 <a0 a1 d0 d1 o> <p>   (float64: 16 digits)
#include <cmath>
#include <cstdio>
#include <cstring>

#include "mvs_affine_reg_dev.h"

static unsigned s_state = 20240607u;
static unsigned next_u32() {
    s_state = s_state * 1664525u + 1013904223u;
    return s_state;
}
static float unit_f() { return (float)(next_u32() >> 8) / (float)(1 << 24); }
static double unit_d() { return ((double)(next_u32() >> 5) * 67108864.0 + (double)(next_u32() >> 6)) / 9007199254740992.0; }
static unsigned bits_f(float v) {
    unsigned u;
    memcpy(&u, &v, 4);
    return u;
}
static unsigned long long bits_d(double v) {
    unsigned long long u;
    memcpy(&u, &v, 8);
    return u;
}

static float special_fraction(int i) {      // every few cases: a fraction of exactly 0, the largest below 1, a half
    switch (i % 7) {
        case 0: return 0.f;
        case 1: return 0.99999994f;
        case 2: return 0.5f;
        default: return unit_f();
    }
}

int main() {
    for (int i = 0; i < 600; ++i) {
        float m[8], fr[3], v = 0.f, g[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 8; ++k) m[k] = unit_f() * (i % 3 == 0 ? 1000.f : 1.f) - (i % 5 == 0 ? 0.5f : 0.f);
        for (int k = 0; k < 3; ++k) fr[k] = i % 2 ? special_fraction(i / 2 + 3 * k) : unit_f();
        if (i % 37 == 5) m[next_u32() % 8] = NAN;
        if (i % 41 == 7) m[next_u32() % 8] = INFINITY;
        if (i % 43 == 9) m[next_u32() % 8] = -INFINITY;
        const bool ok3 = mvs_ar::sample3(m, fr[0], fr[1], fr[2], &v, g);
        printf("S3");
        for (int k = 0; k < 8; ++k) printf(" %08x", bits_f(m[k]));
        printf(" %08x %08x %08x %d %08x %08x %08x %08x\n", bits_f(fr[0]), bits_f(fr[1]), bits_f(fr[2]), ok3 ? 1 : 0,
               bits_f(ok3 ? v : 0.f), bits_f(ok3 ? g[0] : 0.f), bits_f(ok3 ? g[1] : 0.f), bits_f(ok3 ? g[2] : 0.f));
        float v2 = 0.f, g2[2] = {0.f, 0.f};
        const bool ok2 = mvs_ar::sample2(m, fr[1], fr[2], &v2, g2);
        printf("S2 %08x %08x %08x %08x %08x %08x %d %08x %08x %08x\n", bits_f(m[0]), bits_f(m[1]), bits_f(m[2]), bits_f(m[3]), bits_f(fr[1]),
               bits_f(fr[2]), ok2 ? 1 : 0, bits_f(ok2 ? v2 : 0.f), bits_f(ok2 ? g2[0] : 0.f), bits_f(ok2 ? g2[1] : 0.f));
    }
    // coordinates: whole numbers (fraction 0), the last admissible cell (upper tap = last voxel), the ends, outside, NaN
    const long long lens[4] = {2, 7, 44, 130};
    for (int i = 0; i < 400; ++i) {
        const long long n = lens[i % 4];
        double p;
        switch (i % 8) {
            case 0: p = (double)(next_u32() % (unsigned)n); break;                      // whole: n - 1 itself is outside
            case 1: p = (double)(n - 2) + unit_d(); break;                               // upper tap is the last voxel
            case 2: p = (double)(n - 1); break;
            case 3: p = -unit_d() * 1e-9; break;
            case 4: p = (double)(n - 1) - 1e-12; break;
            case 5: p = i % 16 == 5 ? NAN : (i % 32 == 13 ? 1e300 : -1e300); break;
            default: p = unit_d() * (double)(n + 2) - 1.0; break;
        }
        long long i0 = 0;
        float f = 0.f;
        const bool ok = mvs_ar::split(p, n, &i0, &f);
        printf("P %016llx %lld %d %lld %08x\n", bits_d(p), n, ok ? 1 : 0, ok ? i0 : 0ll, bits_f(ok ? f : 0.f));
    }
    for (int i = 0; i < 300; ++i) {
        double a[3], d[3], o = unit_d() * 100.0;
        for (int k = 0; k < 3; ++k) {
            a[k] = (k == i % 3 ? 1.0 : 0.0) + (unit_d() - 0.5) * 0.1;
            d[k] = (double)(next_u32() % 401) / 2.0 - 100.0;          // half-integers, as x - c is
        }
        printf("C3");
        for (int k = 0; k < 3; ++k) printf(" %016llx", bits_d(a[k]));
        for (int k = 0; k < 3; ++k) printf(" %016llx", bits_d(d[k]));
        printf(" %016llx %016llx\n", bits_d(o), bits_d(mvs_ar::coord3(a, d[0], d[1], d[2], o)));
        printf("C2 %016llx %016llx %016llx %016llx %016llx %016llx\n", bits_d(a[0]), bits_d(a[1]), bits_d(d[0]), bits_d(d[1]), bits_d(o),
               bits_d(mvs_ar::coord2(a, d[0], d[1], o)));
    }
    printf("done\n");
    return 0;
}
