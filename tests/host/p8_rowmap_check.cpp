// Brute-force check of csrc/p8_rowmap.h on the CPU (built and run by tests/test_host_p8_rowmap.py):
//   (a) p8_row_pixel is a bijection of the logical rows [0, M) onto the output pixels;
//   (b) for every tile, every kernel row outside p8_kh_range's [kh_lo, kh_hi) is padding for every row of the tile,
//       by the kernel's own ih = oh sh - ph + kh, and the range is never empty;
//   (c) a tile inside one image row of one group gets exactly that row's valid kernel rows (the skip happens).
// N 1..9, Ho 1..5, Wo 1..7, tiles of 8 rows, G in {1, 2, 3, N, N + 5}, 3x3 pad 1 at strides 1 and 2.
#include <cstdio>
#include <vector>

#include "p8_rowmap.h"

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

int main() {
    const int BM = 8, KH = 3, ph = 1;
    long tiles = 0, pure = 0, skipped = 0;
    for (int N = 1; N <= 9; ++N)
        for (int Ho = 1; Ho <= 5; ++Ho)
            for (int Wo = 1; Wo <= 7; ++Wo) {
                const int M = N * Ho * Wo;
                const int Gs[5] = {1, 2, 3, N, N + 5};
                for (int G : Gs) {
                    // (a) bijection, groups of G pairs, image rows ascending inside a group
                    std::vector<int> hit(M, 0), oh_of(M), grp_of(M);
                    for (int L = 0; L < M; ++L) {
                        int n, oh, ow, grp;
                        p8_row_pixel(L, N, Ho, Wo, G, n, oh, ow, grp);
                        const bool in = n >= 0 && n < N && oh >= 0 && oh < Ho && ow >= 0 && ow < Wo;
                        EXPECT(in, "N %d Ho %d Wo %d G %d L %d -> (%d, %d, %d)", N, Ho, Wo, G, L, n, oh, ow);
                        if (!in) continue;
                        EXPECT(grp == n / (G > N ? N : G), "group of pair %d: %d (G %d)", n, grp, G);
                        ++hit[(n * Ho + oh) * Wo + ow];
                        oh_of[L] = oh;
                        grp_of[L] = grp;
                    }
                    for (int m = 0; m < M; ++m) EXPECT(hit[m] == 1, "N %d Ho %d Wo %d G %d: pixel %d hit %d times", N, Ho, Wo, G, m, hit[m]);
                    // (b), (c) per stride and input height
                    for (int sh = 1; sh <= 2; ++sh)
                        for (int H = sh * Ho - (sh - 1); H <= sh * Ho; ++H)   // every H with (H + 2 - 3) / sh + 1 == Ho
                            for (int m0 = 0; m0 < M; m0 += BM) {
                                const int last = (m0 + BM < M ? m0 + BM : M) - 1;
                                int lo, hi;
                                p8_kh_range(oh_of[m0], oh_of[last], grp_of[m0] == grp_of[last], H, sh, ph, KH, lo, hi);
                                ++tiles;
                                EXPECT(0 <= lo && lo < hi && hi <= KH, "range [%d, %d)", lo, hi);
                                bool one_row = true;
                                for (int L = m0; L <= last; ++L) {
                                    one_row = one_row && oh_of[L] == oh_of[m0] && grp_of[L] == grp_of[m0];
                                    for (int kh = 0; kh < KH; ++kh) {
                                        if (kh >= lo && kh < hi) continue;
                                        const int ih = oh_of[L] * sh - ph + kh;
                                        EXPECT(ih < 0 || ih >= H,
                                               "N %d Ho %d Wo %d G %d sh %d H %d tile %d: row %d (oh %d) reads ih %d at "
                                               "the dropped kh %d", N, Ho, Wo, G, sh, H, m0, L, oh_of[L], ih, kh);
                                    }
                                }
                                skipped += KH - (hi - lo);
                                if (one_row) {
                                    ++pure;
                                    for (int kh = 0; kh < KH; ++kh) {
                                        const int ih = oh_of[m0] * sh - ph + kh;
                                        EXPECT((kh >= lo && kh < hi) == (ih >= 0 && ih < H),
                                               "one-row tile (oh %d, sh %d, H %d): kh %d walked %d", oh_of[m0], sh, H, kh,
                                               kh >= lo && kh < hi);
                                    }
                                }
                            }
                }
            }
    EXPECT(pure > 0 && skipped > 0, "no tile inside one image row / nothing dropped");
    EXPECT(p8_default_rowgroup(24, 256) == 32 && p8_default_rowgroup(47, 256) == 49 && p8_default_rowgroup(94, 512) == 49,
           "default groups %d %d %d", p8_default_rowgroup(24, 256), p8_default_rowgroup(47, 256),
           p8_default_rowgroup(94, 512));
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("all checks passed: %ld tiles, %ld inside one image row, %ld kernel rows dropped\n", tiles, pure, skipped);
    return 0;
}
