// CPU check of csrc/conv_route.h, the bf16 conv family's dispatch policy (built and run by
// tests/test_host_conv_route.py; `--table` prints the workload's route table, which DESIGN.md §5 quotes):
//   (a) the route of every conv of the workload -- ResNet-50 LEF maps after stem and pool (19 x 188), 256 CUs, default
//       knobs: the bf16 tier at 1112 pairs with folded shortcuts (stage 1 is the fused bottleneck, not a conv
//       dispatch), the compensated tier at 400 pairs -- written out below; at 4 pairs (4 x 13 maps) nothing reaches
//       p8 or big2; the chained stage-2 junction; the split-K factors of the encoder's out-projection and fc2;
//   (b) each knob at its non-default value moves exactly the rows listed for it;
//   (c) invariants over a grid of shapes, epilogues and CU counts (for_each_point), at the default knobs and at each
//       non-default knob value.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "conv_route.h"

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

static int dummy;   // stands for every device pointer: the policy only asks whether one is there

enum Res { RES_NONE, RES_BF16, RES_F32, RES_SPLIT };

// One conv as the runtime builds it (launch_conv / launch_conv_x3): c channels in (x3: a [hi | lo] tensor read as
// 3 c K-channels), "same" padding, cin2 > 0 = a second K-source of cin2 channels sampled at stride s2.
static ConvArgs conv(int N, int H, int W, int c, int cout, int k, int stride, int flags, Res res, bool x3 = false,
                     int cin2 = 0, int s2 = 1) {
    ConvArgs a{};
    a.x = a.w = a.zero = a.y = &dummy;
    a.N = N, a.H = H, a.W = W, a.Cin = x3 ? 3 * c : c, a.Cout = cout, a.KH = a.KW = k;
    a.sh = a.sw = stride, a.ph = a.pw = k / 2;
    a.Ho = (H + 2 * (k / 2) - k) / stride + 1, a.Wo = (W + 2 * (k / 2) - k) / stride + 1;
    a.M = N * a.Ho * a.Wo;
    if (x3) a.xfold = c, a.x_ld = 2 * c;
    a.flags = flags | (res == RES_F32 ? CBW_EPI_RES_F32 : res == RES_SPLIT ? CBW_EPI_RES_SPLIT : 0);
    if (res != RES_NONE) a.res = &dummy;
    a.res_ld = res == RES_SPLIT ? 2 * cout : cout;
    a.y_ld = (flags & CBW_EPI_SPLIT3) ? 2 * cout : cout;
    if (cin2) a.x2 = &dummy, a.Cin2 = cin2, a.s2 = s2, a.H2 = a.Ho * s2, a.W2 = a.Wo * s2;
    return a;
}

// ---------------------------------------------------------------- (a) the workload
struct Row {
    std::string id;     // tier.stage.conv
    ConvArgs a;
    const char* want;   // the recorded kernel name
};

// ResNet-50 after the stem and pool: stage s has width w = 64 << s, 4 w channels out, stride 2 in the first block's
// 3x3 from stage 2 on (1-based names s1..s4).  Identical blocks of a stage are one row.
static std::vector<Row> workload(int N, int H0, int W0, bool names) {
    const int R = CBW_EPI_RELU, S3 = CBW_EPI_SPLIT3, F32 = CBW_EPI_OUT_F32;
    std::vector<Row> rows;
    const auto row = [&](const std::string& id, const ConvArgs& a, const char* want) {
        rows.push_back({id, a, names ? want : nullptr});
    };
    // bf16 tier, stages 2-4: the first block's expand carries the projection shortcut as its second K-source
    static const char* const bf16_want[3][7] = {
        {"conv_stream_kernel<8, 8, 1, 2, 1>", "conv_igemm_p8<3, 3, 128>", "conv_stream_kernel<12, 8, 2, 2, 0>",
         "conv_stream_kernel<16, 8, 2, 1, 0>", "conv_igemm_p8<3, 3, 128>", "conv_stream_kernel<4, 8, 2, 2, 1>"},
        {"conv_stream_kernel<16, 8, 2, 1, 0>", "conv_igemm_p8<3, 3, 256>", "conv_igemm_p8<1, 1, 256>",
         "conv_igemm_p8<1, 1, 256>", "conv_igemm_p8<3, 3, 256>", "conv_stream_kernel<8, 12, 1, 2, 0>"},
        {"conv_igemm_p8<1, 1, 256>", "conv_igemm_p8<3, 3, 256>", "conv_igemm_p8<1, 1, 256>",
         "conv_igemm_p8<1, 1, 256>", "conv_igemm_p8<3, 3, 256>", "conv_stream_kernel<16, 8, 2, 1, 0>"}};
    int H = H0, W = W0, in = 256;
    for (int s = 2; s <= 4; ++s) {
        const int w = 32 << s, out = 4 * w, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
        const std::string p = "bf16.s" + std::to_string(s) + ".";
        const char* const* want = bf16_want[s - 2];
        row(p + "first reduce", conv(N, H, W, in, w, 1, 1, R, RES_NONE), want[0]);
        row(p + "first 3x3", conv(N, H, W, w, w, 3, 2, R, RES_NONE), want[1]);
        row(p + "expand + shortcut", conv(N, Ho, Wo, w, out, 1, 1, R, RES_NONE, false, in, 2), want[2]);
        row(p + "reduce", conv(N, Ho, Wo, out, w, 1, 1, R, RES_NONE), want[3]);
        row(p + "3x3", conv(N, Ho, Wo, w, w, 3, 1, R, RES_NONE), want[4]);
        row(p + "expand", conv(N, Ho, Wo, w, out, 1, 1, R, RES_BF16), want[5]);
        H = Ho, W = Wo, in = out;
    }
    // compensated tier, stages 1-4: [hi | lo] inputs, split outputs, the shortcut in fp32 as the first block's residual
    static const char* const x3_want[4][7] = {
        {"conv_igemm_kernel<128, 128, 1, 1>", "conv_igemm_kernel<256, 64, 1, 1>", "conv_igemm_kernel<256, 64, 3, 3>",
         "conv_igemm_persist<128, 128, 1, 1>", "conv_igemm_kernel<256, 64, 1, 1>", "conv_igemm_kernel<256, 64, 3, 3>",
         "conv_igemm_persist<128, 128, 1, 1>"},
        {"conv_igemm_p8<1, 1, 256>", "conv_igemm_p8<1, 1, 128>", "conv_igemm_p8<3, 3, 128>",
         "conv_igemm_persist<128, 128, 1, 1>", "conv_igemm_p8<1, 1, 128>", "conv_igemm_p8<3, 3, 128>",
         "conv_igemm_persist<128, 128, 1, 1>"},
        {"conv_igemm_p8<1, 1, 256>", "conv_igemm_p8<1, 1, 256>", "conv_igemm_p8<3, 3, 256>", "conv_igemm_p8<1, 1, 256>",
         "conv_igemm_p8<1, 1, 256>", "conv_igemm_p8<3, 3, 256>", "conv_igemm_p8<1, 1, 256>"},
        {"conv_igemm_p8<1, 1, 256>", "conv_igemm_p8<1, 1, 256>", "conv_igemm_p8<3, 3, 256>", "conv_igemm_p8<1, 1, 256>",
         "conv_igemm_p8<1, 1, 256>", "conv_igemm_p8<3, 3, 256>", "conv_igemm_p8<1, 1, 256>"}};
    H = H0, W = W0, in = 64;
    for (int s = 1; s <= 4; ++s) {
        const int w = 32 << s, out = 4 * w, st = s > 1 ? 2 : 1, Ho = (H - 1) / st + 1, Wo = (W - 1) / st + 1;
        const std::string p = "x3.s" + std::to_string(s) + ".";
        const char* const* want = x3_want[s - 1];
        row(p + "shortcut", conv(N, H, W, in, out, 1, st, F32, RES_NONE, true), want[0]);
        row(p + "first reduce", conv(N, H, W, in, w, 1, 1, S3 | R, RES_NONE, true), want[1]);
        row(p + "first 3x3", conv(N, H, W, w, w, 3, st, S3 | R, RES_NONE, true), want[2]);
        row(p + "first expand", conv(N, Ho, Wo, w, out, 1, 1, S3 | R, RES_F32, true), want[3]);
        row(p + "reduce", conv(N, Ho, Wo, out, w, 1, 1, S3 | R, RES_NONE, true), want[4]);
        row(p + "3x3", conv(N, Ho, Wo, w, w, 3, 1, S3 | R, RES_NONE, true), want[5]);
        row(p + "expand", conv(N, Ho, Wo, w, out, 1, 1, S3 | R, RES_SPLIT, true), want[6]);
        H = Ho, W = Wo, in = out;
    }
    return rows;
}

static std::vector<Row> lef_rows() {   // both tiers at their pair counts
    std::vector<Row> rows = workload(1112, 19, 188, true), x3 = workload(400, 19, 188, true);
    for (size_t i = 0; i < rows.size(); ++i)
        if (rows[i].id[0] == 'x') rows[i] = x3[i];
    return rows;
}

// the stage-2 identity junction of the bf16 tier: block b's expand and block b + 1's reduce
static void junction(ConvArgs& a, ConvArgs& r) {
    a = conv(1112, 10, 94, 128, 512, 1, 1, CBW_EPI_RELU, RES_BF16);
    r = conv(1112, 10, 94, 512, 128, 1, 1, CBW_EPI_RELU, RES_NONE);
}

// the Whisper encoder's few-tile GEMMs at M = 1500 rows, width D: the out-projection D -> D and fc2 4 D -> D
static ConvArgs linear(int M, int K, int Nout) {
    return conv(1, 1, M, K, Nout, 1, 1, CBW_EPI_RES_F32 | CBW_EPI_OUT_F32, RES_F32);
}

static void check_workload(bool print) {
    const ConvKnobs knobs;
    if (print) std::printf("| conv | M | K | Cout | kernel | tile | tiles |\n|---|---|---|---|---|---|---|\n");
    for (const Row& r : lef_rows()) {
        const ConvRoute got = conv_route(r.a, 256, knobs);
        EXPECT(!std::strcmp(got.name, r.want), "%s: %s, expected %s", r.id.c_str(), got.name, r.want);
        if (print && got.BM)
            std::printf("| %s | %d | %d | %d | `%s` | %d x %d | %d |\n", r.id.c_str(), r.a.M, conv_ktot(r.a), r.a.Cout,
                        got.name, got.BM, got.BN, got.tiles);
        else if (print)
            std::printf("| %s | %d | %d | %d | `%s` | | |\n", r.id.c_str(), r.a.M, conv_ktot(r.a), r.a.Cout, got.name);
    }
    for (const Row& r : workload(4, 4, 13, false)) {   // the maps of tools/kws_dump.py
        const ConvRoute got = conv_route(r.a, 256, knobs);
        EXPECT(got.kernel != ConvKernel::Invalid && got.kernel != ConvKernel::P8 && got.kernel != ConvKernel::Big2,
               "4 pairs, %s: %s", r.id.c_str(), got.name);
    }
    ConvArgs a, r;
    junction(a, r);
    const ConvRoute chain = conv_junction_route(a, r, knobs);
    EXPECT(chain.kernel == ConvKernel::Chain && !std::strcmp(chain.name, "conv_stream_chain_kernel<4, 2, 4>"),
           "junction: %s", chain.name);
    // by the rule (2 blocks per CU filled, at least 4 K-steps per split): 120 tiles of 512 slots and 20 / 80 K-steps at
    // D 1280 give 4 and 4; 72 tiles and 12 / 48 K-steps at D 768 give 2 and 4
    const int sk[4] = {conv_splitk_factor(linear(1500, 1280, 1280), 256), conv_splitk_factor(linear(1500, 5120, 1280), 256),
                       conv_splitk_factor(linear(1500, 768, 768), 256), conv_splitk_factor(linear(1500, 3072, 768), 256)};
    EXPECT(sk[0] == 4 && sk[1] == 4 && sk[2] == 2 && sk[3] == 4, "split-K %d %d %d %d", sk[0], sk[1], sk[2], sk[3]);
    if (print) {
        std::printf("| bf16.s2.expand -> reduce junction | %d | 128, 512 | 512, 128 | `%s` | | |\n", a.M, chain.name);
        std::printf("| encoder out-projection / fc2, D 1280 | 1500 | 1280 / 5120 | 1280 | split-K %d / %d | 128 x 128 | 120 |\n",
                    sk[0], sk[1]);
        std::printf("| encoder out-projection / fc2, D 768 | 1500 | 768 / 3072 | 768 | split-K %d / %d | 128 x 128 | 72 |\n",
                    sk[2], sk[3]);
    }
}

// ---------------------------------------------------------------- (b) the knobs
struct Move {
    const char* id;
    const char* to;
};

static void check_knob(const char* what, const ConvKnobs& k, const std::vector<Move>& moves) {
    size_t seen = 0;
    for (const Row& r : lef_rows()) {
        const char* got = conv_route(r.a, 256, k).name;
        const char* want = r.want;
        for (const Move& m : moves)
            if (r.id == m.id) want = m.to, ++seen;
        EXPECT(!std::strcmp(got, want), "%s, %s: %s, expected %s", what, r.id.c_str(), got, want);
    }
    EXPECT(seen == moves.size(), "%s: %zu of %zu rows found", what, seen, moves.size());
}

static void check_knobs() {
    ConvKnobs k;
    const auto with = [](int ConvKnobs::*f, int v) {
        ConvKnobs x;
        x.*f = v;
        return x;
    };
    const char *T11 = "conv_igemm_kernel<128, 128, 1, 1>", *T33 = "conv_igemm_kernel<128, 128, 3, 3>",
               *P11 = "conv_igemm_persist<128, 128, 1, 1>", *B11 = "conv_igemm_big2<256, 1, 1>",
               *B33 = "conv_igemm_big2<256, 3, 3>", *P8 = "conv_igemm_p8<1, 1, 256>",
               *RING = "conv_ring_kernel<1, 1>";
    // p8 rows -> big2 where a round of 256-wide tiles fills and the epilogue is big2's, else the 4-wave kernels; the
    // K 768 folded expand -> the ring kernel
    check_knob("CBW_CONV_P8=0", with(&ConvKnobs::conv_p8, 0),
               {{"bf16.s2.first 3x3", T33}, {"bf16.s2.3x3", T33},
                {"bf16.s3.first 3x3", B33}, {"bf16.s3.expand + shortcut", RING}, {"bf16.s3.reduce", B11}, {"bf16.s3.3x3", B33},
                {"bf16.s4.first reduce", B11}, {"bf16.s4.first 3x3", B33}, {"bf16.s4.expand + shortcut", P11},
                {"bf16.s4.reduce", B11}, {"bf16.s4.3x3", B33},
                {"x3.s2.shortcut", T11}, {"x3.s2.first reduce", T11}, {"x3.s2.first 3x3", T33}, {"x3.s2.reduce", T11},
                {"x3.s2.3x3", T33},
                {"x3.s3.shortcut", T11}, {"x3.s3.first reduce", B11}, {"x3.s3.first 3x3", B33}, {"x3.s3.first expand", P11},
                {"x3.s3.reduce", B11}, {"x3.s3.3x3", B33}, {"x3.s3.expand", P11},
                {"x3.s4.shortcut", T11}, {"x3.s4.first reduce", B11}, {"x3.s4.first 3x3", T33}, {"x3.s4.first expand", P11},
                {"x3.s4.reduce", T11}, {"x3.s4.3x3", T33}, {"x3.s4.expand", P11}});
    check_knob("CBW_P8_N128=0", with(&ConvKnobs::p8_n128, 0),
               {{"bf16.s2.first 3x3", T33}, {"bf16.s2.3x3", T33}, {"x3.s2.first reduce", T11}, {"x3.s2.first 3x3", T33},
                {"x3.s2.reduce", T11}, {"x3.s2.3x3", T33}});
    check_knob("CBW_P8_X2=0", with(&ConvKnobs::p8_x2, 0),
               {{"bf16.s3.expand + shortcut", RING}, {"bf16.s4.expand + shortcut", P11}});
    // p8 wants K >= 512 and the streaming kernel K <= 512: the workload's streaming fold (stage 2, K 384) stays, a
    // fold of K 512 moves
    check_knob("CBW_P8_X2=2", with(&ConvKnobs::p8_x2, 2), {});
    const ConvArgs k512 = conv(1112, 10, 94, 256, 1024, 1, 1, CBW_EPI_RELU, RES_NONE, false, 256, 2);
    EXPECT(conv_route(k512, 256, k).kernel == ConvKernel::Stream, "K 512 fold: %s", conv_route(k512, 256, k).name);
    EXPECT(!std::strcmp(conv_route(k512, 256, with(&ConvKnobs::p8_x2, 2)).name, P8), "K 512 fold, CBW_P8_X2=2");
    // the tier rule's rows: expands and fp32 shortcuts to the 4-wave kernels, the rest to what the bf16 pass's rules
    // give a split conv (p8 from a full round of tiles, which stage 4's 226 are not)
    check_knob("CBW_P8_TIER=0", with(&ConvKnobs::p8_tier, 0),
               {{"x3.s2.shortcut", T11}, {"x3.s3.shortcut", T11}, {"x3.s3.first expand", P11}, {"x3.s3.expand", P11},
                {"x3.s4.shortcut", T11}, {"x3.s4.first 3x3", T33}, {"x3.s4.first expand", P11}, {"x3.s4.reduce", T11},
                {"x3.s4.3x3", T33}, {"x3.s4.expand", P11}});
    check_knob("CBW_CONV_STREAM=0", with(&ConvKnobs::conv_stream, 0),
               {{"bf16.s2.first reduce", RING}, {"bf16.s2.expand + shortcut", RING}, {"bf16.s2.reduce", RING},
                {"bf16.s2.expand", P11}, {"bf16.s3.first reduce", RING}, {"bf16.s3.expand", P11}, {"bf16.s4.expand", P11}});
    check_knob("CBW_CS_K512=0", with(&ConvKnobs::cs_k512, 0),
               {{"bf16.s2.reduce", RING}, {"bf16.s3.first reduce", RING}, {"bf16.s4.expand", P11}});
    // not routing: the same kernels
    check_knob("CBW_P8_ROWSKIP=0", with(&ConvKnobs::p8_rowskip, 0), {});
    check_knob("CBW_P8_ROWGROUP=7", with(&ConvKnobs::p8_rowgroup, 7), {});
    check_knob("CBW_CS_CHAIN=0", with(&ConvKnobs::cs_chain, 0), {});
    check_knob("CBW_CS_PREFETCH=0", with(&ConvKnobs::cs_prefetch, 0),
               {{"bf16.s2.first reduce", "conv_stream_kernel<8, 12, 1, 2, 0>"},
                {"bf16.s2.expand", "conv_stream_kernel<4, 12, 2, 2, 0>"}});
    check_knob("CBW_CS_PREFETCH=1", with(&ConvKnobs::cs_prefetch, 1),
               {{"bf16.s3.expand", "conv_stream_kernel<8, 8, 1, 2, 1>"}});
    ConvArgs a, r;
    junction(a, r);
    EXPECT(conv_junction_route(a, r, with(&ConvKnobs::cs_chain, 0)).kernel == ConvKernel::Invalid, "CBW_CS_CHAIN=0");
    EXPECT(conv_junction_route(a, r, with(&ConvKnobs::conv_stream, 0)).kernel == ConvKernel::Invalid, "chain without streaming");
    EXPECT(conv_junction_route(a, r, with(&ConvKnobs::cs_k512, 0)).kernel == ConvKernel::Invalid, "chain without the K 512 reduce");
    // the row group of p8's 3x3 tiles: Wo 47 on 256-row tiles -> 49 pairs, 7 by the knob, 0 = the flat order
    const ConvArgs c = conv(1112, 5, 47, 256, 256, 3, 1, CBW_EPI_RELU, RES_NONE);
    EXPECT(conv_route(c, 256, k).p8_g == 49, "row group %d", conv_route(c, 256, k).p8_g);
    EXPECT(conv_route(c, 256, with(&ConvKnobs::p8_rowgroup, 7)).p8_g == 7, "CBW_P8_ROWGROUP=7");
    EXPECT(conv_route(c, 256, with(&ConvKnobs::p8_rowskip, 0)).p8_g == 0, "CBW_P8_ROWSKIP=0");
    EXPECT(conv_route(conv(1112, 5, 47, 1024, 256, 1, 1, CBW_EPI_RELU, RES_NONE), 256, k).p8_g == 0, "1x1 row group");
}

// ---------------------------------------------------------------- (c) invariants over the grid
// every flag combination the runtime builds for a residual kind: launch_conv's (ResNet, encoder, decoder prefill)
// and launch_conv_x3's
template <class F>
static void for_each_epilogue(F f) {
    const int R = CBW_EPI_RELU, G = CBW_EPI_GELU, F32 = CBW_EPI_OUT_F32, S3 = CBW_EPI_SPLIT3, AFTER = CBW_EPI_RES_AFTER_ACT;
    for (int flags : {0, R, G, F32}) f(flags, RES_NONE, false);
    for (int flags : {0, R}) f(flags, RES_BF16, false);
    for (int flags : {F32, G | F32 | AFTER}) f(flags, RES_F32, false);
    for (Res res : {RES_NONE, RES_F32, RES_SPLIT})
        for (int flags : {S3, S3 | R, F32, F32 | R}) f(flags, res, true);
}

template <class F>
static long for_each_point(F f) {
    long n = 0;
    const int HW[4][2] = {{19, 188}, {10, 94}, {3, 24}, {1, 1500}};
    for (int N : {1, 4, 400, 1112})
        for (const auto& hw : HW)
            for (int c : {32, 64, 96, 128, 256, 512, 1024, 2048})
                for (int cout : {64, 128, 192, 256, 384, 512, 2048})
                    for (int k : {1, 3})
                        for (int stride : {1, 2})
                            for_each_epilogue([&](int flags, Res res, bool x3) {
                                for (int cin2 : {0, c, 2 * c}) {   // x2 off, and on as the stage-1 / stage-2-4 folds
                                    if (cin2 && x3) continue;      // (the compensated tier folds no shortcut)
                                    const ConvArgs a = conv(N, hw[0], hw[1], c, cout, k, stride, flags, res, x3, cin2, stride);
                                    for (int ncus : {1, 256, 304}) f(a, ncus), ++n;
                                }
                            });
    return n;
}

// what each kernel needs of a conv, whatever the policy prefers
static bool p8_runs(const ConvArgs& a, int BN) {
    return a.Cout % BN == 0 && a.Cin % 64 == 0 && a.xfold % 64 == 0 && !(a.flags & CBW_EPI_GELU) &&
           !(a.res && (a.flags & CBW_EPI_RES_AFTER_ACT)) &&
           (!a.x2 || (a.KH * a.KW == 1 && a.Cin2 % 64 == 0 && !a.xfold && !a.x_ld));
}
static bool big2_runs(const ConvArgs& a) {   // K-steps of 32 through a 4-stage ring
    return a.Cout % 256 == 0 && a.Cin % 32 == 0 && a.xfold % 32 == 0 && a.KH * a.KW * a.Cin >= 256 && !a.res && !a.x2 &&
           !(a.flags & (CBW_EPI_OUT_F32 | CBW_EPI_GELU | CBW_EPI_RES_SPLIT));
}
static bool tile_runs(const ConvArgs& a, int BN) {   // conv_igemm_kernel / conv_igemm_persist
    return a.Cout % BN == 0 && a.Cin % 64 == 0 && (!a.x2 || (BN == 128 && a.KH * a.KW == 1 && a.Cin2 % 64 == 0));
}

static void check_point(const ConvArgs& a, int ncus, const ConvKnobs& k) {
    const ConvRoute r = conv_route(a, ncus, k);
    const bool plain_epilogue = !(a.flags & ~CBW_EPI_RELU);
#define AT "N %d H %d W %d Cin %d Cout %d k %d s %d flags %d res %d x2 %d xfold %d ncus %d: %s", a.N, a.H, a.W, a.Cin, \
           a.Cout, a.KH, a.sh, a.flags, a.res != nullptr, a.x2 ? a.Cin2 : 0, a.xfold, ncus, r.name
    switch (r.kernel) {
        case ConvKernel::Stream:
            EXPECT(conv_stream_supported(a, k) && plain_epilogue && !a.xfold, AT);
            EXPECT(r.stream.ks * 32 == conv_ktot(a), AT);
            break;
        case ConvKernel::Ring: EXPECT(conv_ring_supported(a) && plain_epilogue && !a.res && !a.xfold, AT); break;
        case ConvKernel::P8: EXPECT((r.BN == 256 || r.BN == 128) && r.BM * r.BN == 65536 && p8_runs(a, r.BN), AT); break;
        case ConvKernel::Big2: EXPECT(r.BM == 256 && r.BN == 256 && big2_runs(a), AT); break;
        case ConvKernel::Persist: EXPECT(r.BM == 128 && r.BN == 128 && tile_runs(a, 128), AT); break;
        case ConvKernel::Tile:
            EXPECT(((r.BM == 128 && r.BN == 128) || (r.BM == 256 && r.BN == 64)) && tile_runs(a, r.BN), AT);
            break;
        case ConvKernel::Invalid:
            EXPECT(!conv_stream_wanted(a, k) && !conv_ring_supported(a) && !p8_runs(a, 256) && !p8_runs(a, 128) &&
                       !big2_runs(a) && !tile_runs(a, 128) && !tile_runs(a, 64), AT);
            break;
        default: EXPECT(false, AT);
    }
    if (r.BM) EXPECT(r.tiles == (a.M + r.BM - 1) / r.BM * (a.Cout / r.BN) && r.tiles > 0, AT);
    EXPECT(r.kernel == ConvKernel::Invalid || r.name[0], AT);
    EXPECT(r.p8_g == 0 || (r.kernel == ConvKernel::P8 && a.KH == 3 && r.p8_g <= a.N), AT);
#undef AT
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--table")) {
        check_workload(true);
        return failures != 0;
    }
    check_workload(false);
    check_knobs();
    std::vector<ConvKnobs> sets(1);
    for (int ConvKnobs::*f : {&ConvKnobs::conv_p8, &ConvKnobs::p8_tier, &ConvKnobs::p8_n128, &ConvKnobs::conv_stream,
                              &ConvKnobs::cs_k512, &ConvKnobs::p8_x2}) {
        sets.push_back(ConvKnobs{});
        sets.back().*f = 0;
    }
    sets.push_back(ConvKnobs{});
    sets.back().p8_x2 = 2;
    long points = 0;
    for (const ConvKnobs& k : sets) points += for_each_point([&](const ConvArgs& a, int ncus) { check_point(a, ncus, k); });
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("%zu workload rows, %ld grid points: all checks passed\n", lef_rows().size(), points);
    return 0;
}
