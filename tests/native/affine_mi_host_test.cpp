// Host-side run of csrc/mvs_affine_mi_dev.h (its functions are __host__ __device__): the window functions on a grid of
// arguments and the bins, weights and gradient weight of swept values are printed bit for bit.  tests/test_affine_mi_host.py
// builds this with hipcc (no GPU needed), feeds the printed inputs to the float32 mode of tests/affine_mi_oracle.py and
// compares the bits.  Lines (float32 as 8 hex digits):
//   T <t> <beta3(t)> <beta3'(t)> <quantised beta3(t)>                      t = -2.5 .. 2.5 in steps of 1 / 1024
//   R <B> <lo> <f_scale> <m_scale>                                         the range of the V lines that follow for this B
//   V <B> <v> <fixed bin of v> <u> <first tap> <q_0 q_1 q_2 q_3> <w>       w = gradient_weight over the row of row_value()
#include <cmath>
#include <cstdio>
#include <cstring>

#include "mvs_affine_mi_dev.h"

static unsigned s_state = 20250311u;
static unsigned next_u32() {
    s_state = s_state * 1664525u + 1013904223u;
    return s_state;
}
static float unit_f() { return (float)(next_u32() >> 8) / (float)(1 << 24); }
static unsigned bits_f(float v) {
    unsigned u;
    memcpy(&u, &v, 4);
    return u;
}
static float row_value(int b) { return ((float)((b * 37) % 11) - 5.0f) * 0.25f; }

int main() {
    for (int i = 0; i <= 5120; ++i) {
        const float t = (float)(i - 2560) / 1024.0f;
        const float w = mvs_mi::beta3(t);
        printf("T %08x %08x %08x %lld\n", bits_f(t), bits_f(w), bits_f(mvs_mi::beta3_prime(t)), mvs_mi::quantise(w));
    }
    const int bins[3] = {8, 32, 64};
    const float lo = -0.25f, hi = 3.7f;
    for (int ib = 0; ib < 3; ++ib) {
        const int B = bins[ib];
        const float f_scale = (float)((double)(B - 1) / ((double)hi - (double)lo));
        const float m_scale = (float)((double)(B - 4) / ((double)hi - (double)lo));
        printf("R %d %08x %08x %08x\n", B, bits_f(lo), bits_f(f_scale), bits_f(m_scale));
        float row[mvs_mi::MAX_BINS];
        for (int b = 0; b < B; ++b) row[b] = row_value(b);
        for (int i = 0; i < 10000; ++i) {
            float v;
            if (i == 0) v = lo;
            else if (i == 1) v = hi;
            else if (i % 10 == 2) v = lo + (hi - lo) * ((float)(next_u32() % (unsigned)(2 * B)) / (float)(2 * B));      // bin centres and edges
            else v = lo + (hi - lo) * unit_f();
            const int a = mvs_mi::fixed_bin(v, lo, f_scale, B);
            const float u = mvs_mi::moving_coord(v, lo, m_scale, B);
            long long q[4];
            const int b0 = mvs_mi::hist_weights(u, q);
            printf("V %d %08x %d %08x %d %lld %lld %lld %lld %08x\n", B, bits_f(v), a, bits_f(u), b0, q[0], q[1], q[2], q[3],
                   bits_f(mvs_mi::gradient_weight(u, row)));
        }
    }
    printf("done\n");
    return 0;
}
