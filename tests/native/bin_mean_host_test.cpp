// Host-side run of csrc/mvs_bin_dev.h (mvs_bin::mean_cast is __host__ __device__).  tests/test_bin_mean_host.py builds this with
// hipcc (no GPU needed).  The exact multiples are checked here (3.0e8 of them) and reported as counts; the non-multiples are
// printed for the driver to compare with Python's integer division.  Lines:
//   X <type> <acc> <n checked> <n wrong> <first wrong count> <first wrong mean> <result there>
//                                 sum = k * count must give exactly k.  type u16: every k in 0..65535 for every count in 1..4096
//                                 and for 32768 = 2 * 16384 (the largest count of the 32-bit accumulators), every 61st k for the
//                                 counts between; type u8: every k in 0..255 for every count in 1..512.  acc: the accumulator type
//                                 the kernels pass, u32 (vector kernels) or f64 (generic kernels)
//   N <type> <sum> <count> <result>     40000 sums that are no multiple of their count (xorshift sample)
//   F <sum> <count> <result>            float32 output: the quotient in double, rounded once to float32
#include <cstdint>
#include <cstdio>

#include "mvs_bin_dev.h"

namespace {
struct Wrong {
    long long checked = 0, wrong = 0, count = 0, mean = 0, got = 0;
};

template <typename T, typename S>
void multiples(Wrong& w, long long count, long long kmax, long long kstep) {
    for (long long k = 0; k <= kmax; k += kstep) {
        const T got = mvs_bin::mean_cast<T>((S)(k * count), (double)count);
        ++w.checked;
        if ((long long)got != k) {
            if (!w.wrong) { w.count = count; w.mean = k; w.got = (long long)got; }
            ++w.wrong;
        }
    }
}

template <typename T, typename S>
void report(const char* type, const char* acc, long long kmax, long long full_to, long long sparse_to) {
    Wrong w;
    for (long long count = 1; count <= full_to; ++count) multiples<T, S>(w, count, kmax, 1);
    for (long long count = full_to + 1; count < sparse_to; ++count) multiples<T, S>(w, count, kmax, 61);
    if (sparse_to > full_to) multiples<T, S>(w, sparse_to, kmax, 1);
    printf("X %s %s %lld %lld %lld %lld %lld\n", type, acc, w.checked, w.wrong, w.count, w.mean, w.got);
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t next() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
}  // namespace

int main() {
    report<unsigned short, unsigned int>("u16", "u32", 65535, 4096, 32768);
    report<unsigned short, double>("u16", "f64", 65535, 4096, 32768);
    report<unsigned char, unsigned int>("u8", "u32", 255, 512, 512);
    report<unsigned char, double>("u8", "f64", 255, 512, 512);
    for (int i = 0; i < 20000; ++i) {
        const long long count = 2 + (long long)(next() % 32767), k = (long long)(next() % 65535), r = 1 + (long long)(next() % (uint64_t)(count - 1));
        const long long sum = k * count + r;
        const long long got = (i & 1) ? (long long)mvs_bin::mean_cast<unsigned short>((unsigned int)sum, (double)count)
                                      : (long long)mvs_bin::mean_cast<unsigned short>((double)sum, (double)count);
        printf("N u16 %lld %lld %lld\n", sum, count, got);
    }
    for (int i = 0; i < 20000; ++i) {
        const long long count = 2 + (long long)(next() % 511), k = (long long)(next() % 255), r = 1 + (long long)(next() % (uint64_t)(count - 1));
        const long long sum = k * count + r;
        const long long got = (i & 1) ? (long long)mvs_bin::mean_cast<unsigned char>((unsigned int)sum, (double)count)
                                      : (long long)mvs_bin::mean_cast<unsigned char>((double)sum, (double)count);
        printf("N u8 %lld %lld %lld\n", sum, count, got);
    }
    for (int i = 0; i < 2000; ++i) {
        const long long count = 1 + (long long)(next() % 4096);
        const double sum = (double)(next() % (1ull << 40)) / 1024.0;       // exact in double
        printf("F %.17g %lld %.9g\n", sum, count, (double)mvs_bin::mean_cast<float>(sum, (double)count));
    }
    printf("done\n");
    return 0;
}
