// Host-side run of csrc/mvs_detect_dev.h (its functions are __host__ __device__).  tests/test_detection_host.py builds this
// with hipcc (no GPU needed) and compares the printed indices with numpy's.  Lines:
//   R <len> <p> <reflect(p, len)>          lengths 1, 2, 3, 7; p from -40 to 40
//   W <n> <i> <lo> <hi>                    window sizes 1 .. 6; i from 8 to 12
#include <cstdio>

#include "mvs_detect_dev.h"

int main() {
    const int lens[4] = {1, 2, 3, 7};
    for (int len : lens)
        for (int p = -40; p <= 40; ++p) printf("R %d %d %d\n", len, p, mvs_det::reflect(p, len));
    for (int n = 1; n <= 6; ++n)
        for (int i = 8; i <= 12; ++i) {
            int lo, hi;
            mvs_det::window(i, n, &lo, &hi);
            printf("W %d %d %d %d\n", n, i, lo, hi);
        }
    printf("done\n");
    return 0;
}
