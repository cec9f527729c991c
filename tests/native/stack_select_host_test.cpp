// Host-side run of csrc/mvs_stack_select.h (__host__ __device__): the whole radix select of mvs_stack_quantiles for one pixel --
// keys, digits, prefixes, 32-bit bins, the bin walk, the rank rule and the inverse key, passes in the kernel's order -- against
// std::sort, plus the order of the float keys, the rank rule and the strip plan.  tests/test_shading_host.py builds this with hipcc
// (no GPU needed).  Lines:
//   S <dtype> <stacks checked> <results wrong>        one per dtype (u8, u16, f32)
//   K <pairs of the ordered float list wrong>          key order, key(-0) == key(+0), the inverse key
//   R <rank rule cases wrong>
//   P <widths checked> <widths wrong>                  the strips tile every row exactly once, columns are a bijection
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <type_traits>
#include <vector>

#include "mvs_stack_select.h"

namespace {
using namespace mvs_stack_select;

const double kQ[5] = {0.0, 0.02, 0.5, 0.73, 1.0};

template <typename T> bool same(T a, T b) { return a == b; }
template <> bool same<float>(float a, float b) { return float_bits(a) == float_bits(b); }

// the kernel's passes for one pixel: returns false when the pixel has no samples
template <typename T>
bool radix_select(const std::vector<T>& stack, double q, T* result, uint32_t* n_out) {
    constexpr int D = (int)sizeof(T);
    uint32_t prefix = 0, rank = 0;
    for (int pass = 0; pass < D; ++pass) {
        std::vector<uint32_t> bins(256, 0u);
        for (const T v : stack) {
            if (!stack_is_sample(v)) continue;
            const uint32_t key = stack_key(v);
            if (stack_prefix(key, D, pass) != prefix) continue;
            ++bins[stack_digit(key, D, pass)];
        }
        if (pass == 0) {
            uint32_t n = 0;
            for (uint32_t c : bins) n += c;
            *n_out = n;
            if (!n) return false;
            rank = stack_rank(n, q);
        }
        int digit = 0;
        rank = stack_bin_walk(bins.data(), 1, rank, &digit);
        prefix = (prefix << 8) | (uint32_t)digit;
    }
    *result = stack_value<T>(prefix);
    return true;
}

template <typename T>
long long check_stack(const std::vector<T>& stack) {
    std::vector<T> sorted;
    for (const T v : stack)
        if (stack_is_sample(v)) sorted.push_back(v == T(0) ? T(0) : v);          // (-0 counts as +0)
    std::sort(sorted.begin(), sorted.end());
    long long wrong = 0;
    for (const double q : kQ) {
        T got = T(0);
        uint32_t n = 0;
        const bool any = radix_select(stack, q, &got, &n);
        if (n != sorted.size() || any != !sorted.empty()) { ++wrong; continue; }
        if (!any) continue;
        const size_t r = (size_t)std::floor((double)(sorted.size() - 1) * q);
        if (!same(got, sorted[r])) ++wrong;
    }
    return wrong;
}

template <typename T> T random_value(std::mt19937& g, int kind);
template <> unsigned char random_value<unsigned char>(std::mt19937& g, int) { return (unsigned char)(g() & 255u); }
template <> unsigned short random_value<unsigned short>(std::mt19937& g, int kind) {
    return (unsigned short)(kind == 0 ? g() & 65535u : (kind == 1 ? g() & 255u : 0x1200u + (g() & 255u)));
}
template <> float random_value<float>(std::mt19937& g, int kind) {
    if (kind == 0) return bits_float(g());                                       // every bit pattern: NaNs, infinities, denormals
    const uint32_t pick = g() % 16u;
    if (pick == 0) return std::numeric_limits<float>::quiet_NaN();
    if (pick == 1) return -0.0f;
    if (pick == 2) return std::numeric_limits<float>::infinity() * (g() & 1u ? 1.f : -1.f);
    if (pick == 3) return FLT_MIN / 4.f * (g() & 1u ? 1.f : -1.f);
    return ((float)(g() & 0xffffu) - 32768.f) / (kind == 1 ? 7.f : 4096.f);
}

// two values whose keys differ only in digit `pass`
template <typename T>
void digit_pair(int pass, T* a, T* b) {
    constexpr int D = (int)sizeof(T);
    const uint32_t base = D == 4 ? 0xC1234567u : (D == 2 ? 0x4567u : 0x67u);
    const uint32_t flip = 0x5au << (8 * (D - 1 - pass));
    *a = stack_value<T>(base);
    *b = stack_value<T>(base ^ flip);
}

template <typename T>
void run_dtype(const char* name) {
    std::mt19937 g(12345u + (unsigned)sizeof(T));
    const int sizes[7] = {1, 2, 3, 255, 256, 257, 70000};
    long long stacks = 0, wrong = 0;
    for (const int n : sizes) {
        for (int kind = 0; kind < 3; ++kind) {                                    // random
            std::vector<T> s((size_t)n);
            for (T& v : s) v = random_value<T>(g, kind);
            wrong += check_stack(s), ++stacks;
        }
        {                                                                         // all equal
            std::vector<T> s((size_t)n, random_value<T>(g, 2));
            if (!stack_is_sample(s[0])) std::fill(s.begin(), s.end(), T(1));
            wrong += check_stack(s), ++stacks;
        }
        for (const int pass : {(int)sizeof(T) - 1, 0}) {                          // two values that differ in the lowest / highest digit only
            T a, b;
            digit_pair<T>(pass, &a, &b);
            for (const unsigned share : {2u, 3u, 97u}) {
                std::vector<T> s((size_t)n);
                for (T& v : s) v = g() % share ? a : b;
                wrong += check_stack(s), ++stacks;
            }
        }
    }
    if constexpr (std::is_same<T, float>::value) {                                // no samples at all, and one among NaNs
        std::vector<T> s(300, std::numeric_limits<float>::quiet_NaN());
        wrong += check_stack(s), ++stacks;
        s[123] = -2.5f;
        wrong += check_stack(s), ++stacks;
    }
    printf("S %s %lld %lld\n", name, stacks, wrong);
}

long long check_keys() {
    const float inf = std::numeric_limits<float>::infinity();
    const float list[8] = {-inf, -FLT_MAX, -FLT_MIN / 8.f, -0.0f, 0.0f, FLT_MIN / 8.f, FLT_MAX, inf};
    long long wrong = 0;
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) {
            const bool zeros = (i == 3 || i == 4) && (j == 3 || j == 4);
            const uint32_t a = stack_key(list[i]), b = stack_key(list[j]);
            if (zeros ? a != b : ((a < b) != (i < j) || (a == b) != (i == j))) ++wrong;
        }
    for (int i = 0; i < 8; ++i) {
        const float back = stack_value<float>(stack_key(list[i]));
        if (float_bits(back) != float_bits(i == 3 ? 0.0f : list[i])) ++wrong;
    }
    if (stack_is_sample(std::numeric_limits<float>::quiet_NaN()) || !stack_is_sample(inf) || !stack_is_sample(-inf)) ++wrong;
    for (uint32_t v = 0; v < 65536u; ++v) {
        if (stack_value<unsigned short>(stack_key((unsigned short)v)) != v) ++wrong;
        if (v < 256u && stack_value<unsigned char>(stack_key((unsigned char)v)) != v) ++wrong;
    }
    return wrong;
}

long long check_ranks() {
    long long wrong = 0;
    const uint32_t ns[12] = {1, 2, 3, 4, 7, 255, 256, 257, 70000, 1000003, 0x7ffffffeu, 0x7fffffffu};
    for (const uint32_t n : ns)
        for (const double q : kQ)
            if ((double)stack_rank(n, q) != std::floor((double)(n - 1) * q)) ++wrong;
    return wrong;
}

bool plan_tiles(long long W, int es) {
    const StackPlan p = stack_plan(W, es);
    if (p.strip_px * es != kStripBytes || p.vec * es != kWordBytes || p.vec * kStripLanes != p.strip_px) return false;
    std::vector<int> hits((size_t)W, 0);
    for (int s = 0; s < p.n_strips; ++s) {
        long long x0, x1;
        stack_strip_range(p, W, s, &x0, &x1);
        if (x0 < 0 || x1 > W || x1 <= x0 || x1 - x0 > p.strip_px) return false;
        std::vector<int> cols((size_t)p.strip_px, 0);
        for (long long x = x0; x < x1; ++x) {
            const int c = stack_column((int)(x - x0), p.vec);
            if (c < 0 || c >= p.strip_px || stack_column_pixel(c, p.vec) != (int)(x - x0)) return false;
            ++cols[(size_t)c];
            ++hits[(size_t)x];
        }
        for (const int c : cols)
            if (c > 1) return false;
    }
    for (const int h : hits)
        if (h != 1) return false;
    return true;
}
}  // namespace

int main() {
    run_dtype<unsigned char>("u8");
    run_dtype<unsigned short>("u16");
    run_dtype<float>("f32");
    printf("K %lld\n", check_keys());
    printf("R %lld\n", check_ranks());
    long long widths = 0, wrong = 0;
    for (long long W = 1; W <= 1100; ++W)
        for (const int es : {1, 2, 4}) {
            ++widths;
            if (!plan_tiles(W, es)) ++wrong;
        }
    printf("P %lld %lld\n", widths, wrong);
    printf("done\n");
    return 0;
}
