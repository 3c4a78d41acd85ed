// CPU check of gemv_wide_route (csrc/gemv_route.h), the dispatch of a decode-step Linear over 1..80 rows (built and run
// by tests/test_host_gemv_wide.py; `--table` prints the wide kernel of every (K, LayerNorm prologue), which DESIGN.md
// §3 quotes beside gemv_route's table):
//   (a) for every M = 1..80 at every (K, LN) of DESIGN.md's table: ceil(M / 16) row groups; every group, the tail
//       included, on what gemv_route(16, ...) gives -- the kernel family a <= 16-row launch of that (K, LN) runs, on
//       its 16-slot instantiation; the LDS of a full group within the raised limit; the grid = groups x column blocks
//       in either order; the name spells the group's fields;
//   (b) M = 0 and M = 81 have no route, and neither has a shape gemv_route rejects;
//   (c) gemv_route itself still ends at 16 rows.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "gemv_route.h"

static int failures = 0;
#define EXPECT(c, ...)                                   \
    do {                                                 \
        if (!(c)) {                                      \
            if (++failures <= 20) {                      \
                std::fprintf(stderr, "FAIL %s: ", #c);   \
                std::fprintf(stderr, __VA_ARGS__);       \
                std::fprintf(stderr, "\n");              \
            }                                            \
        }                                                \
    } while (0)

static const int WIDTHS[] = {128, 256, 384, 768, 1024, 1280, 1536, 2048, 3072, 4096, 5120};

static long check_all_rows() {
    long n = 0;
    for (int K : WIDTHS)
        for (int ln = 0; ln < 2; ++ln) {
            if (ln && K > GV_LN_MAXK) continue;
            for (int N : {100, 1280, 3840, 51904}) {
                const GemvRoute g16 = gemv_route(16, N, K, ln != 0);
                const GemvRoute g1 = gemv_route(1, N, K, ln != 0);
                for (int M = 1; M <= GV_WIDE_ROWS; ++M, ++n)
                    for (int fast = 0; fast < 2; ++fast) {
                        const GemvWideRoute w = gemv_wide_route(M, N, K, ln != 0, fast != 0);
#define AT "M %d N %d K %d ln %d fast %d: %s", M, N, K, ln, fast, w.name
                        EXPECT(w.groups == (M + 15) / 16, AT);
                        EXPECT(w.group.kernel != GemvKernel::Invalid && w.group.kernel == g16.kernel &&
                                   w.group.kernel == g1.kernel, AT);
                        EXPECT(w.group.maxm == g16.maxm && w.group.wv == g16.wv && w.group.nj == g16.nj &&
                                   w.group.cpw == g16.cpw && w.group.ks == g16.ks && w.group.waves == g16.waves &&
                                   w.group.block == g16.block && w.group.cols == g16.cols && w.group.ln == (ln != 0), AT);
                        if (w.group.kernel == GemvKernel::Dot) EXPECT(w.group.maxm == 16 && w.group.wv == 8, AT);
                        EXPECT(w.group.lds == g16.lds && w.group.lds <= (size_t)GD_LDS16, AT);
                        EXPECT(w.group.kernel != GemvKernel::Mfma || w.group.lds + 16 * 64 * 16 <= (size_t)GV_LDS_DEFAULT, AT);
                        EXPECT((long)w.group.grid * w.group.cols >= N && (long)(w.group.grid - 1) * w.group.cols < N, AT);
                        EXPECT(w.grid_x == (fast ? w.groups : w.group.grid) && w.grid_y == (fast ? w.group.grid : w.groups), AT);
                        EXPECT(w.grid_y <= 65535, AT);
                        char want[96];
                        if (w.group.kernel == GemvKernel::Mfma)
                            std::snprintf(want, sizeof want, "gemv_wide_kernel<%s>", ln ? "true" : "false");
                        else
                            std::snprintf(want, sizeof want, "gemv_dot_wide_kernel<%s, %d, %d, %d, %d, %d>",
                                          ln ? "true" : "false", w.group.nj, w.group.cpw, w.group.maxm, w.group.ks,
                                          w.group.wv);
                        EXPECT(!std::strcmp(want, w.name), "M %d K %d ln %d: name %s, fields spell %s", M, K, ln, w.name, want);
#undef AT
                    }
            }
        }
    return n;
}

static void check_rejections() {
    for (int K : WIDTHS) {
        EXPECT(gemv_wide_route(0, 100, K, false).groups == 0, "M 0, K %d", K);
        EXPECT(gemv_wide_route(GV_WIDE_ROWS + 1, 100, K, false).groups == 0, "M 81, K %d", K);
        EXPECT(!std::strcmp(gemv_wide_route(GV_WIDE_ROWS + 1, 100, K, false).name, ""), "no name without a route");
        EXPECT(gemv_route(17, 100, K, false).kernel == GemvKernel::Invalid, "gemv_route still ends at 16 rows, K %d", K);
    }
    EXPECT(GV_WIDE_ROWS == 80, "80 rows");
    EXPECT(gemv_wide_route(40, 100, 1296, false).groups == 0, "K %% 32");
    EXPECT(gemv_wide_route(40, 102, 1280, false).groups == 0, "N %% 4");
    EXPECT(gemv_wide_route(40, 100, 1312, true).groups == 0, "LN, K > 1280");
    EXPECT(gemv_wide_route(40, 100, 1536, true).groups == 0, "K 1536 has no LayerNorm prologue");
}

static void print_table() {
    std::printf("| K | prologue | 1-80 rows, per group of 16 | LDS per group |\n|---|---|---|---|\n");
    for (int K : WIDTHS)
        for (int ln = 0; ln < 2; ++ln) {
            if (ln && K > GV_LN_MAXK) continue;
            const GemvWideRoute w = gemv_wide_route(80, 1280, K, ln != 0);
            std::printf("| %d | %s | `%s` | %zu |\n", K, ln ? "LayerNorm" : "none", w.name, w.group.lds);
        }
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--table")) {
        print_table();
        return 0;
    }
    const long points = check_all_rows();
    check_rejections();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("%ld (rows, Linear) points: all checks passed\n", points);
    return 0;
}
