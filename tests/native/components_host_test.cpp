// Stand-alone host program of connected-component labelling: csrc/mvs_components_plan.h and csrc/mvs_unionfind.h compiled with the
// host compiler (tests/test_components_host.py builds it with -fsanitize=address,undefined and, where the compiler has it, a second
// time with -fsanitize=thread, and runs it directly).
//
//   components_host_test
//       prints the plan: "O ndim connectivity offsets groups" per neighbourhood, "P n blocks span covered" per scan partition,
//       "V nz ny nx voxels" per shape, then "done".
//   components_host_test label ndim nz ny nx connectivity min_voxels threads per maskfile
//       labels the uint8 mask of the file with the launches of mvs_components.hip restated lane by lane -- the same chunk walk, the
//       same ballots as bit loops, the same head lanes -- the unions running on `threads` std::threads through the shared
//       union / find.  per: chunks per wave (0: the geometry of the plan).  Prints "N n_labels" and the labels as "L v v v ...".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "mvs_components_plan.h"
#include "mvs_unionfind.h"

using namespace mvs_components_plan;
using namespace mvs_unionfind;

namespace {

struct Walk {
    int nz, ny, nx;
    long long chunks, items, per, waves;
};

// run `body(wave)` for every wave, wave w on thread w % threads, all threads at once
template <typename F>
void for_waves(long long waves, int threads, F body) {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([=] {
            for (long long w = t; w < waves; w += threads) body(w);
        });
    for (auto& th : pool) th.join();
}

void rows(const Walk& W, const unsigned char* mask, int* parent, int threads) {
    for_waves(W.waves, threads, [&](long long wave) {
        const long long first = wave * W.per, last = std::min(first + W.per, W.items);
        int carry = kBackground;
        for (long long item = first; item < last; ++item) {
            const long long row = item / W.chunks;
            const int x0 = (int)(item % W.chunks) * 64, n = std::min(64, W.nx - x0);
            if (x0 == 0) carry = kBackground;
            const int base = (int)(row * W.nx + x0);
            unsigned long long m = 0;
            for (int lane = 0; lane < n; ++lane) m |= (unsigned long long)(mask[base + lane] != 0) << lane;
            for (int lane = 0; lane < n; ++lane) {
                const unsigned long long below = ~m & ((1ull << lane) - 1ull);
                const int start = below ? base + 64 - __builtin_clzll(below) : (carry >= 0 ? carry : base);
                parent[base + lane] = ((m >> lane) & 1ull) ? start : kBackground;
            }
            if (n == 64 && (m >> 63)) {
                if (m != ~0ull) carry = base + 64 - __builtin_clzll(~m);
                else if (carry < 0) carry = base;
            } else {
                carry = kBackground;
            }
        }
    });
}

// foreground of the n voxels at base as bits (the sign of parent[] never changes: a relaxed load decides it)
unsigned long long fg_bits(const int* parent, int base, int n) {
    unsigned long long m = 0;
    for (int lane = 0; lane < n; ++lane) m |= (unsigned long long)(uf_load(parent + base + lane) >= 0) << lane;
    return m;
}

void merge(const Walk& W, const RowGroup* groups, int n_groups, int* parent, int threads) {
    for_waves(W.waves, threads, [&](long long wave) {
        const long long first = wave * W.per, last = std::min(first + W.per, W.items);
        for (long long item = first; item < last; ++item) {
            const long long row = item / W.chunks;
            const int z = (int)(row / W.ny), y = (int)(row % W.ny);
            const int x0 = (int)(item % W.chunks) * 64, n = std::min(64, W.nx - x0);
            const int base = (int)(row * W.nx + x0);
            const unsigned long long fgp = fg_bits(parent, base, n);
            if (!fgp) continue;
            if (item == first && x0 > 0 && (fgp & 1ull) && uf_load(parent + base - 1) >= 0) uf_unite(parent, uf_load(parent + base), base - 1);
            for (int g = 0; g < n_groups; ++g) {
                const int qz = z + groups[g].dz, qy = y + groups[g].dy;
                if (qz < 0 || qz >= W.nz || qy < 0 || qy >= W.ny) continue;
                const int qbase = (int)(((long long)qz * W.ny + qy) * W.nx + x0);
                const unsigned long long centre = fg_bits(parent, qbase, n);
                unsigned long long edge = 0;
                if (x0 > 0 && uf_load(parent + qbase - 1) >= 0) edge |= 1ull;
                if (x0 + 64 < W.nx && uf_load(parent + qbase + 64) >= 0) edge |= 2ull;
                if (!(centre | edge)) continue;
                const unsigned long long across = fgp & centre;
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!((groups[g].dx_mask >> (dx + 1)) & 1u)) continue;
                    unsigned long long both;
                    if (dx == 0) both = across;
                    else if (dx < 0) both = fgp & ((centre << 1) | (edge & 1ull)) & ~across & ~(fgp << 1);
                    else both = fgp & ((centre >> 1) | ((edge >> 1) << 63)) & ~across & ~(fgp >> 1);
                    const unsigned long long heads = both & ~(both << 1);
                    for (int lane = 0; lane < 64; ++lane)      // (the chase starts from the parents loaded, as the kernel's does)
                        if ((heads >> lane) & 1ull)
                            uf_unite(parent, uf_load(parent + base + lane), dx == 0 ? uf_load(parent + qbase + lane) : qbase + lane + dx);
                }
            }
        }
    });
}

int label(int argc, char** argv) {
    if (argc != 11) return 2;
    const int ndim = atoi(argv[2]);
    Walk W{};
    W.nz = atoi(argv[3]); W.ny = atoi(argv[4]); W.nx = atoi(argv[5]);
    const int connectivity = atoi(argv[6]);
    const long long min_voxels = atoll(argv[7]);
    const int threads = atoi(argv[8]);
    const int64_t shape[3] = {W.nz, W.ny, W.nx};
    const long long n = voxel_count(shape);
    if (n < 1 || threads < 1) return 2;
    W.chunks = row_chunks(W.nx);
    W.items = (long long)W.nz * W.ny * W.chunks;
    W.per = atoll(argv[9]);
    if (W.per < 1) W.per = chunks_per_wave(W.items, (long long)grid_blocks(W.items, kWaves) * kWaves);
    W.waves = (W.items + W.per - 1) / W.per;
    std::vector<unsigned char> mask((size_t)n);
    FILE* f = fopen(argv[10], "rb");
    if (!f || fread(mask.data(), 1, (size_t)n, f) != (size_t)n) return 3;
    fclose(f);
    RowGroup groups[kMaxRowGroups];
    const int n_groups = row_groups(ndim, connectivity, groups);
    if (!n_groups) return 2;

    std::vector<int> parent((size_t)n), out((size_t)n, -7);
    rows(W, mask.data(), parent.data(), threads);
    for (long long p = 0; p < n; ++p)
        if (parent[p] > p) return 4;      // the invariant, after the rows ...
    merge(W, groups, n_groups, parent.data(), threads);
    for (long long p = 0; p < n; ++p)
        if (parent[p] > p) return 4;      // ... and after the unions
    // flatten (and sizes)
    std::vector<unsigned int> sizes(min_voxels > 1 ? (size_t)n : 0);
    for (long long p = 0; p < n; ++p) {
        if (parent[p] < 0) continue;
        parent[p] = uf_find(parent.data(), parent[p]);
        if (!sizes.empty()) ++sizes[parent[p]];
    }
    // number: counts per block, scan, ranks at the roots
    const ScanPlan scan = scan_plan(n);
    auto kept = [&](long long p) { return parent[p] == (int)p && (sizes.empty() || sizes[p] >= (unsigned long long)min_voxels); };
    std::vector<int> counts((size_t)scan.blocks + 1, 0);
    for (int b = 0; b < scan.blocks; ++b)
        for (long long p = b * scan.span; p < std::min((b + 1) * scan.span, n); ++p) counts[b] += kept(p);
    int running = 0;
    for (int b = 0; b <= scan.blocks; ++b) {
        const int cnt = counts[b];
        counts[b] = running;
        running += cnt;
    }
    for (int b = 0; b < scan.blocks; ++b) {
        int rank = counts[b];
        for (long long p = b * scan.span; p < std::min((b + 1) * scan.span, n); ++p)
            if (parent[p] == (int)p) out[p] = kept(p) ? ++rank : 0;
    }
    // relabel
    for (long long p = 0; p < n; ++p) out[p] = parent[p] < 0 ? 0 : out[parent[p]];
    printf("N %d\nL", counts[scan.blocks]);
    for (long long p = 0; p < n; ++p) printf(" %d", out[p]);
    printf("\n");
    return 0;
}

int plan() {
    for (int ndim = 2; ndim <= 3; ++ndim)
        for (int connectivity = 0; connectivity <= ndim + 1; ++connectivity) {
            RowGroup groups[kMaxRowGroups];
            const int n_groups = row_groups(ndim, connectivity, groups);
            if (n_groups > kMaxRowGroups) return 1;
            for (int g = 0; g < n_groups; ++g) {
                if (!groups[g].dz && !groups[g].dy) return 1;      // the x-only offset belongs to the row launch
                if (!groups[g].dx_mask || groups[g].dx_mask > 7u) return 1;
                if (ndim == 2 && groups[g].dz) return 1;
            }
            printf("O %d %d %d %d\n", ndim, connectivity, n_groups ? offsets_of(groups, n_groups) : 0, n_groups);
        }
    const long long ns[] = {1, 255, 256, 257, 4847, 366800, 524287, 524288, 524289, 134217728LL, kMaxVoxels};
    for (long long n : ns) {
        const ScanPlan s = scan_plan(n);
        // the ranges [b * span, min((b + 1) * span, n)) cover 0 .. n - 1 once: the last one is not empty, the one after it would be
        const bool covered = s.blocks >= 1 && s.blocks <= kMaxScanBlocks && s.span % kThreads == 0 && (long long)(s.blocks - 1) * s.span < n &&
                             (long long)s.blocks * s.span >= n;
        long long seen = 0;
        if (n <= 600000)
            for (int b = 0; b < s.blocks; ++b) seen += std::min((b + 1) * s.span, n) - b * s.span;
        printf("P %lld %d %lld %d\n", n, s.blocks, s.span, (int)(covered && (n > 600000 || seen == n)));
    }
    const int64_t shapes[][3] = {{1, 1, 1}, {5, 1, 9}, {512, 512, 512}, {1, 46341, 46341}, {1, 1, 0x7fffffffLL}, {2, 1, 0x40000000LL}, {1290, 1291, 1290}};
    for (const auto& s : shapes) printf("V %lld %lld %lld %lld\n", (long long)s[0], (long long)s[1], (long long)s[2], voxel_count(s));
    if (parent_bytes(100) != 512 || sizes_bytes(100, 1) != 0 || sizes_bytes(100, 2) != 512 || scan_bytes() % 256 || scan_bytes() < 4 * (kMaxScanBlocks + 1)) return 1;
    printf("done\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "label")) return label(argc, argv);
    return plan();
}
