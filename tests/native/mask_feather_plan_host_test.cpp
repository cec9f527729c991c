// Stand-alone host program of csrc/mvs_mask_feather_plan.h (tests/test_mask_feather_host.py builds it with the host compiler under the
// address and undefined-behaviour sanitizers): the integer scale for every width triple's extremes, and for a table of volumes the
// slabs -- they tile the planes, their halos stay inside the mask and inside the plane set -- and the scratch bound.
//   S wz wy wx D Pz Py Px worst        worst = D + w^2 P of the largest term a pass adds (must stay below 2^32)
//   L nz ny nx halo forced budget planes slabs set_bytes ok
#include "mvs_mask_feather_plan.h"

#include <cstdio>
#include <initializer_list>

using namespace mvs_mask_feather_plan;

static int check_slabs(long long nz, long long ny, long long nx, int halo, long long forced, size_t budget) {
    const long long planes = slab_planes(nz, ny, nx, halo, forced, budget);
    const long long n = n_slabs(nz, planes);
    const size_t set_bytes = plane_set_bytes(nz, ny, nx, planes, halo);
    int ok = planes >= 1 && planes <= nz;
    long long next = 0;
    for (long long k = 0; k < n; ++k) {
        const Slab s = slab(k, nz, planes, halo);
        ok = ok && s.z0 == next && s.z1 > s.z0 && s.z1 <= nz;                               // the slabs tile the planes in order
        ok = ok && s.h0 >= 0 && s.h1 <= nz && s.h0 <= s.z0 && s.h1 >= s.z1;                 // the halo stays inside the mask ...
        ok = ok && (s.h0 == 0 || s.h0 == s.z0 - halo) && (s.h1 == nz || s.h1 == s.z1 + halo);      // ... and is whole where the mask allows
        ok = ok && (size_t)(s.h1 - s.h0) * (size_t)ny * (size_t)nx * sizeof(uint32_t) <= set_bytes;      // ... and inside the plane set
        next = s.z1;
    }
    ok = ok && next == nz;
    if (forced <= 0 && planes > 1) ok = ok && 2 * set_bytes <= budget;                      // the scratch bound
    std::printf("L %lld %lld %lld %d %lld %zu %lld %lld %zu %d\n", nz, ny, nx, halo, forced, budget, planes, n, set_bytes, ok);
    return ok;
}

int main() {
    const int ws[] = {1, 2, 3, 7, 31, 32};
    for (int wz : ws)
        for (int wy : ws)
            for (int wx : ws) {
                const int w[3] = {wz, wy, wx};
                const Scale s = scale_of(w);
                unsigned long long worst = 0;
                for (int k = 0; k < 3; ++k) {
                    const unsigned long long term = (unsigned long long)s.D + (unsigned long long)w[k] * w[k] * s.P[k];
                    worst = term > worst ? term : worst;
                }
                std::printf("S %d %d %d %u %u %u %u %llu\n", wz, wy, wx, s.D, s.P[0], s.P[1], s.P[2], worst);
            }
    int ok = 1;
    const long long vols[][3] = {{1, 33, 70}, {12, 20, 37}, {7, 5, 3}, {256, 256, 256}, {40, 1, 67}, {1000, 2048, 2048}, {3, 4, 5}};
    for (const auto& v : vols)
        for (int halo : {0, 1, 3, 32})
            for (long long forced : {0LL, 1LL, 2LL, 5LL, 1000000LL}) ok &= check_slabs(v[0], v[1], v[2], halo, forced, kSlabBudget);
    ok &= check_slabs(64, 100, 100, 8, 0, (size_t)1 << 20);      // a small budget: several automatic slabs
    ok &= check_slabs(64, 100, 100, 8, 0, 1000);                  // a budget below one plane: slabs of one plane
    std::printf("P %d %d %d %d\n", (int)pass_needed(1, 32), (int)pass_needed(5, 1), (int)pass_needed(2, 2), grid_blocks(0, 256));
    std::printf(ok ? "done\n" : "FAILED\n");
    return ok ? 0 : 1;
}
