// Host program for tests/test_masks_host.py: csrc/mvs_masks_plan.h compiled with the host compiler.  Prints
//   "O <ndim> <connectivity> <count> <bad>"      the half neighbourhood: its size and the number of rule violations
//   "G <nx> <groups> <pitch> <blocks of nx rows x groups> <chunk blocks>"   launch geometry of a row of nx voxels
//   "H <rows> <max_nx> <blocks> <voxels per block at most>"                 the histogram grid
// and "done".
#include <cstdio>
#include <set>
#include <tuple>

#include "mvs_masks_plan.h"

using namespace mvs_masks_plan;

int main() {
    for (int ndim = 2; ndim <= 3; ++ndim)
        for (int conn = 0; conn <= 4; ++conn) {
            Offset off[kMaxOffsets];
            const int n = half_neighbourhood(ndim, conn, off);
            int bad = 0;
            std::set<std::tuple<int, int, int>> seen;
            for (int i = 0; i < n; ++i) {
                const Offset o = off[i];
                const int nonzero = (o.dz != 0) + (o.dy != 0) + (o.dx != 0);
                bad += nonzero < 1 || nonzero > conn;
                bad += ndim == 2 && o.dz != 0;
                bad += o.dz < -1 || o.dz > 1 || o.dy < -1 || o.dy > 1 || o.dx < -1 || o.dx > 1;
                bad += seen.count({o.dz, o.dy, o.dx}) != 0;       // listed twice
                bad += seen.count({-o.dz, -o.dy, -o.dx}) != 0;    // an offset and its negative
                seen.insert({o.dz, o.dy, o.dx});
            }
            // every admissible offset or its negative is there
            for (int dz = (ndim == 3 ? -1 : 0); dz <= (ndim == 3 ? 1 : 0); ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int nonzero = (dz != 0) + (dy != 0) + (dx != 0);
                        if (nonzero < 1 || nonzero > conn || conn > ndim) continue;
                        bad += seen.count({dz, dy, dx}) + seen.count({-dz, -dy, -dx}) != 1;
                    }
            std::printf("O %d %d %d %d\n", ndim, conn, n, bad);
        }
    const long long lengths[] = {1, 15, 16, 17, 63, 64, 65, 70, 4096, 4097};
    for (long long nx : lengths) {
        const long long rows = nx;      // a square plane
        std::printf("G %lld %lld %lld %d %d\n", nx, row_groups(nx), padded_pitch(nx), grid_blocks(rows * row_groups(nx), kThreads),
                    grid_blocks(rows * ((nx + 63) / 64), kWaves));
    }
    std::printf("G 0 0 0 %d %d\n", grid_blocks(0, kThreads), grid_blocks(1LL << 40, kThreads));
    const long long cases[][2] = {{1, 1}, {63, 70}, {8192, 1 << 20}, {1LL << 24, 1 << 20}, {1LL << 31, 1LL << 29}, {5, 1LL << 29}, {(1LL << 31) - 1, 3}};
    for (const auto& cs : cases) {
        const long long blocks = hist_blocks(cs[0], cs[1]);
        std::printf("H %lld %lld %lld %lld\n", cs[0], cs[1], blocks, hist_rows_per_block(cs[0], blocks) * cs[1]);
    }
    std::printf("done\n");
    return 0;
}
