// Host-side run of tile_row_split (csrc/mvs_tile_apply.h, __host__ __device__): how intensity_apply_kernel and plane_apply_kernel
// cut a row into a scalar head, whole vectors and a scalar tail.  For every type pair the library instantiates, every byte
// misalignment 0..31 of the source and of the destination, every row length 0..70 and both values of vectors_allowed.
// tests/test_tile_apply_host.py builds this with hipcc (no GPU needed).  One line per type pair:
//   T <in> <out> <cases> <cases with vectors> <order> <short tail> <misaligned> <forbidden> <rule>
// order:      0 <= head <= tail <= nx and tail == head + nvec * V violated
// short tail: nvec > 0 and V or more elements left after the vectors
// misaligned: nvec > 0 and the first vector of the source or of the destination not aligned to V elements -- what faults a GPU
// forbidden:  nvec > 0 although vectors_allowed is false or the source is not element-aligned
// rule:       differs from the rule as the kernels spelled it before they shared it, restated below
#include <cstdio>

#include "mvs_tile_apply.h"

namespace {

// the rule of the apply kernels before tile_row_split, with the element sizes as types and the addresses as integers
template <typename TIn, typename TOut, int V>
TileRowSplit spelled_out(unsigned long long src, unsigned long long dst, int nx, bool vectors_allowed) {
    const unsigned long long mis = src % (V * sizeof(TIn));
    int head = mis ? (int)((V * sizeof(TIn) - mis) / sizeof(TIn)) : 0;
    if (head > nx || mis % sizeof(TIn) || (dst + head * sizeof(TOut)) % (V * sizeof(TOut)) || !vectors_allowed) head = nx;
    const int nvec = (nx - head) / V, tail = head + nvec * V;
    return TileRowSplit{head, nvec, tail};
}

template <typename TIn, typename TOut>
long long run_pair(const char* in_name, const char* out_name) {
    constexpr int V = tile_vec_len<TIn, TOut>();
    constexpr int in_es = (int)sizeof(TIn), out_es = (int)sizeof(TOut);
    static_assert(V * (in_es > out_es ? in_es : out_es) == 16, "16 bytes on the wider side");
    const unsigned long long src_base = 1ull << 20, dst_base = 3ull << 32;      // 4 GiB apart: the sum of an address and a row stays exact
    long long cases = 0, vectors = 0, order = 0, short_tail = 0, misaligned = 0, forbidden = 0, rule = 0;
    for (int ms = 0; ms < 32; ++ms)
        for (int md = 0; md < 32; ++md)
            for (int nx = 0; nx <= 70; ++nx)
                for (int allowed = 0; allowed < 2; ++allowed) {
                    const unsigned long long src = src_base + ms, dst = dst_base + md;
                    const TileRowSplit s = tile_row_split(src, dst, nx, in_es, out_es, V, allowed != 0);
                    ++cases;
                    if (!(0 <= s.head && s.head <= s.tail && s.tail <= nx && s.tail == s.head + s.nvec * V) || s.nvec < 0) ++order;
                    if (s.nvec > 0) {
                        ++vectors;
                        if (nx - s.tail >= V) ++short_tail;
                        if ((src + (unsigned long long)s.head * in_es) % (unsigned long long)(V * in_es) ||
                            (dst + (unsigned long long)s.head * out_es) % (unsigned long long)(V * out_es))
                            ++misaligned;
                        if (!allowed || src % in_es) ++forbidden;
                    }
                    const TileRowSplit w = spelled_out<TIn, TOut, V>(src, dst, nx, allowed != 0);
                    if (s.head != w.head || s.nvec != w.nvec || s.tail != w.tail) ++rule;
                }
    printf("T %s %s %lld %lld %lld %lld %lld %lld %lld\n", in_name, out_name, cases, vectors, order, short_tail, misaligned, forbidden, rule);
    return order + short_tail + misaligned + forbidden + rule;
}
}  // namespace

int main() {
    long long wrong = 0;
    wrong += run_pair<unsigned char, unsigned char>("u8", "u8");
    wrong += run_pair<unsigned short, unsigned short>("u16", "u16");
    wrong += run_pair<float, float>("f32", "f32");
    wrong += run_pair<unsigned char, float>("u8", "f32");
    wrong += run_pair<unsigned short, float>("u16", "f32");
    printf("done\n");
    return wrong ? 1 : 0;
}
