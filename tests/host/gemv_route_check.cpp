// CPU check of csrc/gemv_route.h, the decode-step GEMV's dispatch (built and run by tests/test_host_gemv_route.py;
// `--table` prints the kernel of every (K, LayerNorm prologue, row range), which DESIGN.md §3 quotes):
//   (a) for every row count 1..16 and every (K, LN) the decoders of synth.WHISPER_DECODERS produce (d_model with and
//       without the prologue, ffn_dim without; plus K 2048, which no dot kernel takes): the route is launchable -- LDS
//       within the 64 KB default unless the route raises the limit, then within GD_LDS16; the loads per lane one of
//       wait_vm's counts; the grid covers N and no workgroup lies wholly past it; the name spells the fields;
//   (b) for a given (K, LN) every row count gets the same kernel family (MFMA gemv_kernel or dot gemv_dot_kernel): what
//       cbw_decoder_step_rows' bit-for-bit sentence needs.  The LDS test `M * (K + 8) * 2 <= limit` for the DMA'd rows
//       (which take M * K * 2 / KS) sent (K 4096, 8 rows) and (K 5120, 7 / 8 / 16 rows) to the MFMA kernel;
//   (c) the routes of 1, 5, 10 and 15 rows, field for field, as cbw_gemv launched them before the dispatch moved into
//       the header: the table below was written from that launcher, not from gemv_route.h;
//   (d) what cbw_gemv rejects has no route.
#include <cstdio>
#include <cstring>
#include <string>

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

// name, vocabulary, d_model, ffn_dim of synth.WHISPER_DECODERS (large-v3-2l has large-v3's widths)
struct Decoder {
    const char* name;
    int vocab, d, ffn;
};
static const Decoder DECODERS[] = {{"micro", 51865, 128, 256},    {"tiny.en", 51864, 384, 1536},
                                   {"small", 51865, 768, 3072},   {"medium", 51865, 1024, 4096},
                                   {"large-v3", 51866, 1280, 5120}};

// every Linear of a decode step as (N, K, LN): qkv, cross q, fc1 and the vocabulary projection behind a LayerNorm;
// the two out-projections and fc2 on bf16 rows; and the unfused forms of the first four
template <class F>
static void for_each_linear(F&& f) {
    for (const Decoder& d : DECODERS) {
        const int vpad = (d.vocab + 63) / 64 * 64;
        for (int ln = 0; ln < 2; ++ln) {
            f(3 * d.d, d.d, ln != 0);
            f(d.d, d.d, ln != 0);
            f(d.ffn, d.d, ln != 0);
            f(vpad, d.d, ln != 0);
            f(100, d.d, ln != 0);   // the tests' N: a column tail in every instantiation
        }
        f(d.d, d.ffn, false);
        f(100, d.ffn, false);
    }
    f(100, 2048, false);
    f(2048, 2048, false);
}

static const int STATIC_LDS_MFMA = 16 * 64 * 16;   // gemv_kernel's red[16][64] f32x4

// ---------------------------------------------------------------- (a) launchable, (b) one family per (K, LN)
static void check_launchable(int M, int N, int K, bool ln, const GemvRoute& r) {
#define AT "M %d N %d K %d ln %d: %s", M, N, K, (int)ln, r.name
    EXPECT(r.kernel != GemvKernel::Invalid, AT);
    if (r.kernel == GemvKernel::Invalid) return;
    EXPECT(r.ln == ln && r.name[0], AT);
    EXPECT(r.grid >= 1 && (long)r.grid * r.cols >= N && (long)(r.grid - 1) * r.cols < N, AT);
    EXPECT(r.lds <= (size_t)(r.raise_lds ? GD_LDS16 : GV_LDS_DEFAULT), AT);
    char want[96];
    if (r.kernel == GemvKernel::Mfma) {
        EXPECT(r.waves == gemv_waves(K) && r.block == 64 * r.waves && r.block <= (ln ? 512 : 1024) && r.cols == 16, AT);
        EXPECT((K / 32 + r.waves - 1) / r.waves <= GV_BATCH || r.waves == 16, AT);
        EXPECT(!r.raise_lds && r.lds + STATIC_LDS_MFMA <= (size_t)GV_LDS_DEFAULT, AT);
        EXPECT(r.lds == (ln ? (size_t)M * (K + 8) * 2 : 0), AT);
        EXPECT(r.nj == 0 && r.cpw == 0 && r.maxm == 0 && r.ks == 0 && r.wv == 0, AT);
        std::snprintf(want, sizeof want, "gemv_kernel<%s>", ln ? "true" : "false");
    } else {
        EXPECT(r.nj * 256 == K && gemv_dot_width(K) && (r.cpw == 1 || r.cpw == 2) && r.waves == 0, AT);
        EXPECT(M <= r.maxm && (r.maxm == GD_MAXM || r.maxm == 16) && r.wv == (r.maxm == GD_MAXM ? 4 : 8), AT);
        EXPECT(r.block == 64 * r.wv && r.cols == r.wv * r.cpw, AT);
        EXPECT(!ln || (K <= GV_LN_MAXK && r.cpw == 2 && r.ks == 1), AT);
        const int nl = K / (512 / r.cpw);   // loads per lane
        bool counted = false;
        for (int c : GD_WAIT_COUNTS) counted |= c == nl;
        EXPECT(ln || counted, AT);
        EXPECT(r.ks >= 1 && nl % r.ks == 0, AT);
        // the bytes the variant stages: padded rows from the prologue, else whole 1 KB pieces of [M][K / KS]
        const size_t staged = ln ? (size_t)M * (K + 8) * 2 : ((size_t)M * (K / r.ks) * 2 + 1023) / 1024 * 1024;
        EXPECT(r.lds == staged, AT);
        std::snprintf(want, sizeof want, "gemv_dot_kernel<%s, %d, %d, %d, %d, %d>", ln ? "true" : "false", r.nj, r.cpw,
                      r.maxm, r.ks, r.wv);
    }
    EXPECT(!std::strcmp(want, r.name), "M %d N %d K %d ln %d: name %s, fields spell %s", M, N, K, (int)ln, r.name, want);
#undef AT
}

static long check_all_rows() {
    long n = 0;
    for_each_linear([&](int N, int K, bool ln) {
        if (ln && K > GV_LN_MAXK) return;
        const GemvRoute one = gemv_route(1, N, K, ln);
        for (int M = 1; M <= 16; ++M, ++n) {
            const GemvRoute r = gemv_route(M, N, K, ln);
            check_launchable(M, N, K, ln, r);
            EXPECT(r.kernel == one.kernel, "K %d ln %d: %d rows run %s, 1 row runs %s", K, (int)ln, M, r.name, one.name);
            if (r.kernel == GemvKernel::Dot)   // the instantiation may differ between <= 8 and >= 9 rows only
                EXPECT(r.nj == one.nj && r.cpw == one.cpw && r.maxm == (M <= 8 ? 8 : 16), "K %d ln %d M %d: %s", K,
                       (int)ln, M, r.name);
        }
    });
    return n;
}

// ---------------------------------------------------------------- (c) the routes that ran before
// One (K, LN) of the launcher this header replaced: the kernel of 1 / 5 rows and of 10 / 15 rows, the columns per
// workgroup and the block of each, and the dynamic LDS of 1, 5, 10 and 15 rows.  raise: the launch of 10 / 15 rows
// set the kernel's dynamic-LDS limit (1 / 5 rows never did).
struct Pinned {
    int K;
    bool ln;
    GemvKernel kernel;
    const char* name_lo;   // 1 and 5 rows
    const char* name_hi;   // 10 and 15 rows
    int cols_lo, block_lo, cols_hi, block_hi;
    size_t lds[4];
    bool raise_hi;
};
static const GemvKernel MF = GemvKernel::Mfma, DT = GemvKernel::Dot;
static const Pinned PINNED[] = {
    {128, false, MF, "gemv_kernel<false>", "gemv_kernel<false>", 16, 64, 16, 64, {0, 0, 0, 0}, false},
    {128, true, MF, "gemv_kernel<true>", "gemv_kernel<true>", 16, 64, 16, 64, {272, 1360, 2720, 4080}, false},
    {256, false, MF, "gemv_kernel<false>", "gemv_kernel<false>", 16, 64, 16, 64, {0, 0, 0, 0}, false},
    {256, true, MF, "gemv_kernel<true>", "gemv_kernel<true>", 16, 64, 16, 64, {528, 2640, 5280, 7920}, false},
    {384, false, MF, "gemv_kernel<false>", "gemv_kernel<false>", 16, 128, 16, 128, {0, 0, 0, 0}, false},
    {384, true, MF, "gemv_kernel<true>", "gemv_kernel<true>", 16, 128, 16, 128, {784, 3920, 7840, 11760}, false},
    {768, false, DT, "gemv_dot_kernel<false, 3, 2, 8, 1, 4>", "gemv_dot_kernel<false, 3, 2, 16, 1, 8>", 8, 256, 16, 512,
     {2048, 8192, 15360, 23552}, true},
    {768, true, DT, "gemv_dot_kernel<true, 3, 2, 8, 1, 4>", "gemv_dot_kernel<true, 3, 2, 16, 1, 8>", 8, 256, 16, 512,
     {1552, 7760, 15520, 23280}, true},
    {1024, false, DT, "gemv_dot_kernel<false, 4, 2, 8, 1, 4>", "gemv_dot_kernel<false, 4, 2, 16, 1, 8>", 8, 256, 16, 512,
     {2048, 10240, 20480, 30720}, true},
    {1024, true, DT, "gemv_dot_kernel<true, 4, 2, 8, 1, 4>", "gemv_dot_kernel<true, 4, 2, 16, 1, 8>", 8, 256, 16, 512,
     {2064, 10320, 20640, 30960}, true},
    {1280, false, DT, "gemv_dot_kernel<false, 5, 2, 8, 1, 4>", "gemv_dot_kernel<false, 5, 2, 16, 1, 8>", 8, 256, 16, 512,
     {3072, 13312, 25600, 38912}, true},
    {1280, true, DT, "gemv_dot_kernel<true, 5, 2, 8, 1, 4>", "gemv_dot_kernel<true, 5, 2, 16, 1, 8>", 8, 256, 16, 512,
     {2576, 12880, 25760, 38640}, true},
    {1536, false, MF, "gemv_kernel<false>", "gemv_kernel<false>", 16, 512, 16, 512, {0, 0, 0, 0}, false},
    {3072, false, DT, "gemv_dot_kernel<false, 12, 2, 8, 1, 4>", "gemv_dot_kernel<false, 12, 2, 16, 1, 8>", 8, 256, 16, 512,
     {6144, 30720, 61440, 92160}, true},
    {4096, false, DT, "gemv_dot_kernel<false, 16, 2, 8, 1, 4>", "gemv_dot_kernel<false, 16, 2, 16, 1, 8>", 8, 256, 16, 512,
     {8192, 40960, 81920, 122880}, true},
    {5120, false, DT, "gemv_dot_kernel<false, 20, 1, 8, 1, 4>", "gemv_dot_kernel<false, 20, 1, 16, 2, 8>", 4, 256, 8, 512,
     {10240, 51200, 51200, 76800}, true},
};

static void check_pinned() {
    static const int ROWS[4] = {1, 5, 10, 15};
    for (const Pinned& p : PINNED)
        for (int i = 0; i < 4; ++i)
            for (int N : {100, 1280, 3840, 51904}) {
                const int M = ROWS[i];
                const bool hi = M > 8;
                const GemvRoute r = gemv_route(M, N, p.K, p.ln);
#define AT "K %d ln %d M %d N %d: %s", p.K, (int)p.ln, M, N, r.name
                EXPECT(r.kernel == p.kernel && !std::strcmp(r.name, hi ? p.name_hi : p.name_lo), AT);
                EXPECT(r.cols == (hi ? p.cols_hi : p.cols_lo) && r.block == (hi ? p.block_hi : p.block_lo), AT);
                EXPECT(r.grid == (N + r.cols - 1) / r.cols, AT);
                EXPECT(r.lds == p.lds[i], "K %d ln %d M %d: lds %zu, was %zu", p.K, (int)p.ln, M, r.lds, p.lds[i]);
                EXPECT(r.raise_lds == (hi && p.raise_hi), AT);
                EXPECT(r.ln == p.ln, AT);
#undef AT
            }
    EXPECT(gemv_route(5, 1280, 1536, true).kernel == GemvKernel::Invalid, "K 1536 has no LayerNorm prologue");
}

// ---------------------------------------------------------------- (d) no route for what cbw_gemv rejects
static void check_rejections() {
    EXPECT(gemv_route(0, 100, 1280, false).kernel == GemvKernel::Invalid, "M 0");
    EXPECT(gemv_route(17, 100, 1280, false).kernel == GemvKernel::Invalid, "M 17");
    EXPECT(gemv_route(5, 100, 1296, false).kernel == GemvKernel::Invalid, "K %% 32");
    EXPECT(gemv_route(5, 102, 1280, false).kernel == GemvKernel::Invalid, "N %% 4");
    EXPECT(gemv_route(5, 0, 1280, false).kernel == GemvKernel::Invalid, "N 0");
    EXPECT(gemv_route(5, 100, 1312, true).kernel == GemvKernel::Invalid, "LN, K > 1280");
    EXPECT(!std::strcmp(gemv_route(17, 100, 1280, false).name, ""), "no name without a route");
    EXPECT(gemv_ln_ok(16, 1280) && !gemv_ln_ok(16, 1312) && !gemv_ln_ok(17, 128) && !gemv_ln_ok(0, 128), "gemv_ln_ok");
}

// ---------------------------------------------------------------- the table DESIGN.md quotes
static void print_table() {
    std::printf("| K | prologue | 1-8 rows | 9-16 rows | LDS at 8 / 16 rows |\n|---|---|---|---|---|\n");
    for (int K : {128, 256, 384, 768, 1024, 1280, 1536, 2048, 3072, 4096, 5120})
        for (int ln = 0; ln < 2; ++ln) {
            if (ln && K > GV_LN_MAXK) continue;
            const GemvRoute lo = gemv_route(8, 1280, K, ln != 0), hi = gemv_route(16, 1280, K, ln != 0);
            std::printf("| %d | %s | `%s` | `%s` | %zu / %zu |\n", K, ln ? "LayerNorm" : "none", lo.name, hi.name, lo.lds,
                        hi.lds);
        }
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--table")) {
        print_table();
        return 0;
    }
    const long points = check_all_rows();
    check_pinned();
    check_rejections();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("%ld (rows, Linear) points, %zu pinned (K, LN) rows: all checks passed\n", points,
                sizeof PINNED / sizeof PINNED[0]);
    return 0;
}
