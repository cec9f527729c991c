// mvs_stack_select.h -- the arithmetic of the per-pixel order statistics of a stack (mvs_stack_quantiles, mvs_shading.hip),
// host/device: the order-preserving key of a sample and its inverse, the rank rule, the walk over the 256 bins of one radix digit,
// and how a row is cut into the strips the workgroups own.  The kernel includes it, tests/native/stack_select_host_test.cpp runs the
// whole selection on the host through it, and _shading_ops.rank_of mirrors stack_rank.
//
// Selection: most-significant-digit radix select with 8-bit digits.  A sample's key is an unsigned integer of 8 * sizeof(T) bits
// whose order is the order of the values.  Per digit, from the top, a pixel counts its samples whose higher digits equal its
// prefix so far into 256 bins, walks the bins up to the one that holds its rank, appends that digit to the prefix and keeps the
// rank inside the bin.  After the last digit the prefix is the key of the sample of that rank.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#ifndef MVS_HD
#define MVS_HD __host__ __device__ __forceinline__
#endif

namespace mvs_stack_select {

constexpr int kStripBytes = 128;             // a strip spans this many bytes of a row: whole cache lines per plane where the row allows
constexpr int kWordBytes = 4;                // a lane takes this many bytes of the strip: 4 / 2 / 1 consecutive pixels
constexpr int kStripLanes = kStripBytes / kWordBytes;   // 32: half a wave per plane

// ---- keys ----------------------------------------------------------------------------------------------------------------------------
MVS_HD uint32_t float_bits(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}
MVS_HD float bits_float(uint32_t b) {
    float v;
    memcpy(&v, &b, 4);
    return v;
}

// a float32 NaN is not a sample; every other value of the three types is
MVS_HD bool stack_is_sample(unsigned char) { return true; }
MVS_HD bool stack_is_sample(unsigned short) { return true; }
MVS_HD bool stack_is_sample(float v) { return v == v; }

// key(a) < key(b) iff a < b; -0 takes the key of +0
MVS_HD uint32_t stack_key(unsigned char v) { return v; }
MVS_HD uint32_t stack_key(unsigned short v) { return v; }
MVS_HD uint32_t stack_key(float v) {
    uint32_t b = float_bits(v);
    if ((b << 1) == 0u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <typename T> MVS_HD T stack_value(uint32_t key);
template <> MVS_HD unsigned char stack_value<unsigned char>(uint32_t key) { return (unsigned char)key; }
template <> MVS_HD unsigned short stack_value<unsigned short>(uint32_t key) { return (unsigned short)key; }
template <> MVS_HD float stack_value<float>(uint32_t key) { return bits_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

// digit `pass` (0: the most significant) of a key of `digits` digits, and the digits above it
MVS_HD uint32_t stack_digit(uint32_t key, int digits, int pass) { return (key >> (8 * (digits - 1 - pass))) & 255u; }
MVS_HD uint32_t stack_prefix(uint32_t key, int digits, int pass) { return pass == 0 ? 0u : key >> (8 * (digits - pass)); }

// ---- the rank rule ---------------------------------------------------------------------------------------------------------------------
// ascending 0-based rank of quantile q among n >= 1 samples: floor((n - 1) * q) in double (numpy's method="lower")
MVS_HD uint32_t stack_rank(uint32_t n, double q) {
    const double r = floor((double)(n - 1u) * q);
    return r <= 0.0 ? 0u : (r >= (double)(n - 1u) ? n - 1u : (uint32_t)r);
}

// ---- the bin walk ------------------------------------------------------------------------------------------------------------------------
// counts[d * stride], d = 0..255: the bins of one digit, more than `rank` samples in all.  *digit: the bin that holds the sample of
// ascending rank `rank`; returns its rank within that bin.
MVS_HD uint32_t stack_bin_walk(const uint32_t* counts, int stride, uint32_t rank, int* digit) {
    int d = 0;
    for (; d < 255; ++d) {
        const uint32_t c = counts[(long long)d * stride];
        if (rank < c) break;
        rank -= c;
    }
    *digit = d;
    return rank;
}

// ---- strips --------------------------------------------------------------------------------------------------------------------------------
// A row of W pixels of `es` bytes is cut into strips of strip_px = kStripBytes / es pixels (the last one may be shorter).  Within a
// strip, lane l of kStripLanes takes the vec = kWordBytes / es pixels l * vec .. l * vec + vec - 1, and pixel p's bins live in
// column (p % vec) * kStripLanes + p / vec of the histogram: the lanes of one update then fall into kStripLanes different banks.
struct StackPlan {
    int strip_px, vec, n_strips;
};
MVS_HD StackPlan stack_plan(long long W, int es) {
    StackPlan p;
    p.strip_px = kStripBytes / es;
    p.vec = kWordBytes / es;
    p.n_strips = (int)((W + p.strip_px - 1) / p.strip_px);
    return p;
}
// pixels [*x0, *x1) of strip s
MVS_HD void stack_strip_range(const StackPlan& p, long long W, int s, long long* x0, long long* x1) {
    *x0 = (long long)s * p.strip_px;
    *x1 = *x0 + p.strip_px < W ? *x0 + p.strip_px : W;
}
MVS_HD int stack_column(int px, int vec) { return (px % vec) * kStripLanes + px / vec; }
MVS_HD int stack_column_pixel(int col, int vec) { return (col % kStripLanes) * vec + col / kStripLanes; }

}  // namespace mvs_stack_select
