// Stand-alone host program of csrc/mvs_deconv_plan.h and csrc/mvs_stack_frame.h, with the work-area layout of csrc/mvs_multiband_plan.h
// (tests/test_mv_deconv_host.py builds it with -fsanitize=address,undefined and runs it directly).  It prints what the test compares
// with its numpy restatement, one record per line, and writes the tap tables as raw float32 to the file named by its argument, in the
// order of the "T" lines.  The last line is "done".
//   T V kz ky kx kxp         one tap case: the file gets the general table (2 V kz ky kxp floats), the separable table (2 V (kz + ky + kx))
//                            and sep_cval (2 V)
//   A k a                    the anchor of extent k
//   F name value             a plan fact
//   W nz ny nx sep ero host  a deconvolution work area, then psi wr a b m0 m1 bm pk tp out total, then out_bytes taps S
//   M id V out_bytes top     a multi-band work area, then size[0 .. top], then flag f0 win d[0 .. top] a[1 .. top] r[1 .. top] out total
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mvs_deconv_plan.h"
#include "mvs_multiband_plan.h"
#include "mvs_stack_frame.h"

namespace dp = mvs_deconv_plan;
namespace mp = mvs_multiband_plan;

static void require(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        std::exit(1);
    }
}

static const int64_t kNoTrim[3] = {0, 0, 0};

static void dump(std::FILE* f, const std::vector<float>& v) { require(std::fwrite(v.data(), 4, v.size(), f) == v.size(), "write"); }

// kernels of distinct values (an arange per set) and factors whose sums are not 1; the test restates both
static void tap_case(std::FILE* f, int V, int kz, int ky, int kx) {
    const int64_t shape[3] = {1, 8, 8}, ksize[3] = {kz, ky, kx};
    const long long kvol = (long long)kz * ky * kx, ksep = kz + ky + kx;
    std::vector<float> k1(V * kvol), k2(V * kvol), s1(V * ksep), s2(V * ksep);
    for (long long i = 0; i < V * kvol; ++i) k1[i] = (float)(i + 1), k2[i] = (float)(i + 1 + V * kvol);
    for (int v = 0; v < V; ++v)
        for (long long j = 0; j < ksep; ++j) s1[v * ksep + j] = (float)(0.25 + 0.01 * j + v), s2[v * ksep + j] = (float)(0.5 + 0.03 * j + 0.1 * v);
    dp::Plan p;
    std::vector<float> taps, cval;
    require(dp::make_plan(shape, ksize, V, false, false, kNoTrim, mvs_stack_frame::kF32, false, &p) == dp::kOk, "general plan");
    require(p.kxp % 4 == 0 && p.kxp >= kx && p.kxp < kx + 4, "kxp");
    std::printf("T %d %d %d %d %d\n", V, kz, ky, kx, p.kxp);
    dp::make_taps(p, V, k1.data(), k2.data(), s1.data(), s2.data(), &taps, &cval);
    require(taps.size() == p.taps && taps.size() == (size_t)(2 * V * p.kvolp) && cval.empty(), "general table size");
    dump(f, taps);
    require(dp::make_plan(shape, ksize, V, true, false, kNoTrim, mvs_stack_frame::kF32, false, &p) == dp::kOk, "separable plan");
    dp::make_taps(p, V, k1.data(), k2.data(), s1.data(), s2.data(), &taps, &cval);
    require(taps.size() == p.taps && taps.size() == (size_t)(2 * V * ksep) && cval.size() == (size_t)(2 * V), "separable table size");
    dump(f, taps);
    dump(f, cval);
}

static void deconv_area(const int64_t shape[3], bool sep, bool ero, bool host) {
    const int64_t ksize[3] = {1, 5, 7}, trim[3] = {0, 1, 1};
    dp::Plan p;
    require(dp::make_plan(shape, ksize, 2, sep, ero, trim, mvs_stack_frame::kU16, host, &p) == dp::kOk, "plan");
    std::printf("W %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %lld\n", p.nz, p.ny, p.nx, (int)sep, (int)ero, (int)host, p.off_psi,
                p.off_wr, p.off_a, p.off_b, p.off_m0, p.off_m1, p.off_bm, p.off_pk, p.off_tp, p.off_out, p.total, p.box.out_bytes, p.taps, p.S);
}

static void multiband_area(int id, const int32_t levels[3], const int64_t origin[3], const int64_t shape[3], const int64_t trim[3], int V, bool host) {
    mp::Plan p;
    require(mp::make_plan(levels, origin, shape, &p), "multi-band plan");
    const mvs_stack_frame::OutBox box = mvs_stack_frame::out_box(shape, trim, mvs_stack_frame::kU8);
    const mp::WorkArea w = mp::work_area(p, V, host ? box.out_bytes : 0);
    std::printf("M %d %d %zu %d", id, V, host ? box.out_bytes : (size_t)0, p.top);
    for (int l = 0; l <= p.top; ++l) std::printf(" %lld", p.size[l]);
    std::printf(" %zu %zu %zu", w.flag, w.f0, w.win);
    for (int l = 0; l <= p.top; ++l) std::printf(" %zu", w.d[l]);
    for (int l = 1; l <= p.top; ++l) std::printf(" %zu", w.a[l]);
    for (int l = 1; l <= p.top; ++l) std::printf(" %zu", w.r[l]);
    std::printf(" %zu %zu\n", w.out, w.total);
}

int main(int argc, char** argv) {
    require(argc == 2, "usage: deconv_plan_host_test <file for the tap tables>");
    std::FILE* f = std::fopen(argv[1], "wb");
    require(f != nullptr, "open");
    const int extents[][3] = {{1, 1, 1}, {1, 3, 3}, {4, 6, 8}, {5, 1, 12}, {1, 63, 5}, {1, 62, 4}, {1, 7, 12}};
    for (int V : {1, 3})
        for (const auto& k : extents) tap_case(f, V, k[0], k[1], k[2]);
    tap_case(f, 1, 63, 63, 63);
    require(std::fclose(f) == 0, "close");

    for (int k = 1; k <= dp::KMAX; ++k) std::printf("A %d %d\n", k, dp::anchor(k));

    dp::Plan p;
    {
        const int64_t shape[3] = {1, 100, 100}, k63[3] = {1, 63, 63}, k64[3] = {1, 3, 64}, k0[3] = {1, 0, 3};
        require(dp::make_plan(shape, k63, 1, false, false, kNoTrim, mvs_stack_frame::kF32, false, &p) == dp::kOk, "63 x 63 plan");
        std::printf("F lds_bytes_63 %zu\n", p.lds_bytes);
        std::printf("F grid_100x100 %u %u %u\n", p.grid_x, p.grid_y, p.grid_z);
        std::printf("F extent_64 %s\n", dp::make_plan(shape, k64, 1, false, false, kNoTrim, mvs_stack_frame::kF32, false, &p) == dp::kUnsupported ? "UNSUPPORTED" : "other");
        std::printf("F extent_0 %s\n", dp::make_plan(shape, k0, 1, false, false, kNoTrim, mvs_stack_frame::kF32, false, &p) == dp::kInvalidArg ? "INVALID_ARG" : "other");
    }
    std::printf("F grid_for %d %d %d\n", dp::grid_for(0), dp::grid_for(257), dp::grid_for(1LL << 40));
    std::printf("F tile %d %d %d %d %d %d\n", dp::GX, dp::GY, dp::RX, dp::RY, dp::TX, dp::TY);
    std::printf("F kmax %d\nF init_blocks %d\n", dp::KMAX, dp::kInitBlocks);

    const int64_t shapes[][3] = {{1, 4, 4}, {1, 37, 53}, {5, 6, 7}};
    for (const auto& s : shapes)
        for (int sep = 0; sep < 2; ++sep)
            for (int ero = 0; ero < 2; ++ero)
                for (int host = 0; host < 2; ++host) deconv_area(s, sep, ero, host);

    {
        const int32_t lv[3] = {0, 2, 2};
        const int64_t o[3] = {0, -7, 5}, s[3] = {1, 37, 53}, t[3] = {0, 2, 3};
        for (int host = 0; host < 2; ++host) multiband_area(2, lv, o, s, t, 3, host);
    }
    {
        const int32_t lv[3] = {1, 2, 2};
        const int64_t o[3] = {3, 0, -4}, s[3] = {5, 22, 31}, t[3] = {1, 2, 3};
        for (int host = 0; host < 2; ++host) multiband_area(3, lv, o, s, t, 2, host);
    }
    std::printf("done\n");
    return 0;
}
