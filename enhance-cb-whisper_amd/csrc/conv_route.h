// Which kernel a bf16-family conv runs on, with which tiles, and why: the whole dispatch policy as pure host
// functions of (ConvArgs, number of CUs, knobs).  Plain C++17, no HIP include: tests/host/conv_route_check.cpp pins
// the routes of the workload on the CPU, and prints them (--table, quoted in DESIGN.md §5).  The launchers
// (cbw_conv_igemm, cbw_conv_stream, cbw_conv_ring, cbw_conv_chain) launch what these functions say; the kernel files
// tie the tile constants below to their own with one static_assert each.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "conv_args.h"
#include "p8_rowmap.h"

enum class ConvKernel { Invalid, Stream, Chain, Ring, P8, Big2, Persist, Tile };

// conv_stream_kernel<KS, WAVES, RD, PFD, PN>: K-steps of 32, waves, residual steps in flight, 32 >> PFD-pixel units
// (16 at K 512), next-unit row prefetch
struct ConvStreamVariant {
    int ks, waves, rd, pfd, pn;
};

struct ConvRoute {
    ConvKernel kernel = ConvKernel::Invalid;
    int BM = 0, BN = 0;   // tile shape (0: the row-stationary kernels, which have no output tiles)
    int tiles = 0;        // ceil(M / BM) * (Cout / BN)
    int p8_g = 0;         // P8, 3x3: ConvArgs::p8_g
    ConvStreamVariant stream = {};   // Stream
    // the kernel as rocprofv3 names it, template arguments included: a string literal, so the profile records keep
    // the pointer.  bench.py, tools/roofline_from_trace.py, tools/rowskip_table.py and tests match on these.
    const char* name = "";
};

// One field per dispatch knob, at its default; conv_knobs_from_env() is the only reader of the variables, called
// once per dispatch (tests flip them between two calls in one process).
struct ConvKnobs {
    int conv_p8 = 1;       // CBW_CONV_P8: 1 = the 8-phase kernel for the convs conv_igemm_big2 would run, and below
    int p8_x2 = 1;         // CBW_P8_X2: 0 never, 1 the x2 convs ring / persist would run, 2 also the streaming kernel's
    int p8_tier = 1;       // CBW_P8_TIER: 0 = the compensated tier's convs on the tile kernels
    int p8_n128 = 1;       // CBW_P8_N128: 0 = Cout 128 (the stage-2 3x3s) on the 4-wave 128 x 128 kernel
    int p8_rowskip = 1;    // CBW_P8_ROWSKIP: 0 = 3x3 tiles in (pair, oh, ow) order, all nine taps (the same bits)
    int p8_rowgroup = 0;   // CBW_P8_ROWGROUP: the row order's group size (0: p8_default_rowgroup; above N: one group)
    int conv_stream = 1;   // CBW_CONV_STREAM: 0 keeps the streaming kernel's convs on the tile kernels
    int cs_k512 = 1;       // CBW_CS_K512: 0 sends K 512 back to the tile kernels
    int cs_prefetch = -1;  // CBW_CS_PREFETCH: -1 policy, 0 off, 1 on wherever it fits the registers
    int cs_chain = 1;      // CBW_CS_CHAIN: 0 keeps the stage-2 identity junction as two launches
};

inline ConvKnobs conv_knobs_from_env() {
    ConvKnobs k;
    const auto read = [](const char* name, int& v) {
        if (const char* e = getenv(name)) v = atoi(e);
    };
    read("CBW_CONV_P8", k.conv_p8);
    read("CBW_P8_X2", k.p8_x2);
    read("CBW_P8_TIER", k.p8_tier);
    read("CBW_P8_N128", k.p8_n128);
    read("CBW_P8_ROWSKIP", k.p8_rowskip);
    read("CBW_P8_ROWGROUP", k.p8_rowgroup);
    read("CBW_CONV_STREAM", k.conv_stream);
    read("CBW_CS_K512", k.cs_k512);
    read("CBW_CS_PREFETCH", k.cs_prefetch);
    read("CBW_CS_CHAIN", k.cs_chain);
    return k;
}

// ---- tile constants (each kernel file asserts its own against these)
constexpr int CONV_BK = 64;                          // conv_igemm_kernel / _persist, conv_igemm_p8: K elements per step
constexpr int CONV_BIG_BM = 256, CONV_BIG_BK = 32;   // conv_igemm_big2
constexpr int CONV_RING_BM = 256, CONV_RING_BN = 128, CONV_RING_BK = 64, CONV_RING_MAXC = 2048;   // conv_ring_kernel
constexpr int CONV_CS_WBYTES = 131072, CONV_CS_MAXSLICE = 1024;   // conv_stream_kernel: weight slice bytes, bias slots
constexpr int CONV_CC_K = 128, CONV_CC_N = 512, CONV_CC_R = 128;  // the chain: expand K, expand Cout = reduce K, reduce Cout
constexpr int conv_p8_bm(int BN) { return 65536 / BN; }           // conv_igemm_p8: 256 x 256 or 512 x 128 tiles

inline int conv_ktot(const ConvArgs& a) { return a.KH * a.KW * a.Cin + (a.x2 ? a.Cin2 : 0); }
inline int conv_tiles(const ConvArgs& a, int BM, int BN) { return ((a.M + BM - 1) / BM) * (a.Cout / BN); }

// "base<..KH, KW..>" for the three tap shapes the family is instantiated for
#define CBW_NAME_BY_TAPS(a, pre, post) \
    ((a).KH == 3 ? pre "3, 3" post : (a).KW == 3 ? pre "1, 3" post : pre "1, 1" post)

// ---- the row-stationary streaming 1x1 kernel (conv_stream.hip)
// the weight slice: the largest divisor of Cout that is a multiple of 128 channels and fits the budget
inline int slice_channels(int cout, int ktot) {
    for (int nsl = 1; nsl <= cout / 128; ++nsl) {
        if (cout % nsl) continue;
        const int sn = cout / nsl;
        if (sn % 128 == 0 && sn <= CONV_CS_MAXSLICE && (int64_t)sn * ktot * 2 <= CONV_CS_WBYTES) return sn;
    }
    return 0;
}

// K 512 on the streaming kernel (16-pixel units, 8 waves; CBW_CS_K512=0 keeps the tile kernels).
// tools/layer_bench.py, LEF chunk of 500: stage-2 reduce 512 -> 128 140.7 -> 120.5 us, stage-3 first
// reduce 512 -> 256 227.0 -> 183.9 us, stage-4 identity expand 512 -> 2048 + res 163.4 -> 120.7 us
inline bool conv_stream_supported(const ConvArgs& a, const ConvKnobs& k) {
    const int ktot = a.Cin + (a.x2 ? a.Cin2 : 0);
    if (a.KH != 1 || a.KW != 1 || a.sh != 1 || a.sw != 1 || a.ph != 0 || a.pw != 0) return false;
    if (ktot != 128 && ktot != 256 && ktot != 384 && !(ktot == 512 && k.cs_k512)) return false;
    if (a.Cin % 32 || (a.x2 && a.Cin2 % 32)) return false;
    if (a.flags & ~CBW_EPI_RELU) return false;                   // bf16 residual / output, ReLU or none
    if (a.res && a.res_ld % 4) return false;
    if (a.y_ld % 4 || a.M <= 0) return false;
    const int64_t lim = 0x7ffffff0LL - 4096;   // 32-bit buffer offsets, out-of-range marker above
    if ((int64_t)a.M * a.y_ld * 2 >= lim || (int64_t)a.M * a.Cin * 2 >= lim) return false;
    if (a.res && (int64_t)a.M * a.res_ld * 2 >= lim) return false;
    if (a.x2 && (int64_t)a.N * a.H2 * a.W2 * a.Cin2 * 2 >= lim) return false;
    return slice_channels(a.Cout, ktot) > 0;
}

// policy: every supported conv -- at LEF sizes the identity expands (stage 2: 274 -> 244 us, stage 3: 182 ->
// 137 us), the folded-shortcut expands of stages 1-2 and the stage-2 first reduce (307 -> 284 us)
inline bool conv_stream_wanted(const ConvArgs& a, const ConvKnobs& k) {
    return k.conv_stream != 0 && conv_stream_supported(a, k);
}

// (tools/layer_bench.py, LEF chunk of 500: K 128 -- 12 waves, 2 residual steps in flight 244 us vs
// 16 waves, 1 step 256 us; K 256 -- 12 waves, 1 step 137 us vs 8 waves, 2 steps 143 us; 16-pixel units
// with 16 waves: within 2 % at K 128, 6 % slower at K 256)
// next-unit row prefetch (tools/layer_bench.py, LEF chunk of 500, LB_VAR=CBW_CS_PREFETCH): K 128 on 8 waves
// 243.6 -> 237.6 us (stage-2 expand); K 256 on 8 waves 283.9 -> 273.5 us without a residual (stage-2 first
// reduce) but 136.7 -> 142.5 us with one (stage-3 expand: the 12-wave residual latency hiding wins)
inline ConvRoute conv_stream_route(const ConvArgs& a, const ConvKnobs& k) {
    ConvRoute r;
    if (!conv_stream_supported(a, k)) return r;
    const int ktot = a.Cin + (a.x2 ? a.Cin2 : 0);
    const bool pn = k.cs_prefetch >= 0 ? k.cs_prefetch != 0 : (ktot == 128 || (ktot == 256 && !a.res));
    r.kernel = ConvKernel::Stream;
#define CBW_CS_VARIANT(KS, WAVES, RD, PFD, PN) \
    (r.stream = ConvStreamVariant{KS, WAVES, RD, PFD, PN},  \
     r.name = "conv_stream_kernel<" #KS ", " #WAVES ", " #RD ", " #PFD ", " #PN ">")
    switch (ktot) {
        case 128: pn ? CBW_CS_VARIANT(4, 8, 2, 2, 1) : CBW_CS_VARIANT(4, 12, 2, 2, 0); break;
        case 256: pn ? CBW_CS_VARIANT(8, 8, 1, 2, 1) : CBW_CS_VARIANT(8, 12, 1, 2, 0); break;
        case 512: CBW_CS_VARIANT(16, 8, 2, 1, 0); break;
        default: CBW_CS_VARIANT(12, 8, 2, 2, 0); break;   // (K 384 with the prefetch: 244 VGPRs spilled)
    }
#undef CBW_CS_VARIANT
    return r;
}

// ---- the stage-2 identity junction in one launch (conv_stream_chain_kernel)
inline bool conv_chain_supported(const ConvArgs& a, int red_cout, const ConvKnobs& k) {
    if (!conv_stream_supported(a, k) || a.x2 || a.Cin != CONV_CC_K || a.Cout != CONV_CC_N || red_cout != CONV_CC_R)
        return false;
    if (!a.res || a.flags != CBW_EPI_RELU || a.y_ld != CONV_CC_N) return false;
    return slice_channels(a.Cout, a.Cin) == a.Cout;   // one weight slice
}

// 4 waves x 64-pixel units, 2 residual steps in flight (isolated, 834 LEF pairs, whole grid: 448-465 us against
// 365 + 214 us for the two launches; 8 waves x 32-pixel units read Wr twice as often: 565-588 us, and 516 us
// with 2 residual steps in flight, which spills; Wr row-major instead of fragment order: 750 us)
inline ConvRoute conv_chain_route(const ConvArgs& a, int red_cout, const ConvKnobs& k) {
    ConvRoute r;
    if (!conv_chain_supported(a, red_cout, k)) return r;
    r.kernel = ConvKernel::Chain;
    r.name = "conv_stream_chain_kernel<4, 2, 4>";
    return r;
}

// a = block b's identity expand (residual, ReLU), r = block b + 1's 1x1 reduce as their own launches would see
// them: chained when both run on the streaming kernel today and the shapes are the chain's; Invalid = two launches
inline ConvRoute conv_junction_route(const ConvArgs& a, const ConvArgs& r, const ConvKnobs& k) {
    if (!k.cs_chain || r.Cin != a.Cout || r.flags != CBW_EPI_RELU) return {};
    if (!conv_stream_wanted(a, k) || !conv_stream_wanted(r, k)) return {};
    return conv_chain_route(a, r.Cout, k);
}

// ---- the persistent 8-wave ring kernel (conv_ring.hip)
inline bool conv_ring_supported(const ConvArgs& a) {
    if (a.Cout % CONV_RING_BN || a.Cout > CONV_RING_MAXC || a.Cin % CONV_RING_BK || a.M <= 0) return false;
    if (a.flags & ~CBW_EPI_RELU) return false;   // bf16 output, ReLU or none
    if (a.res) return false;                     // identity-residual expands: conv_igemm_persist
    if (a.y_ld % 4 || (int64_t)a.M * a.y_ld * 2 >= 0x7fffffffLL) return false;
    if (a.x2 && (a.KH * a.KW != 1 || a.Cin2 % CONV_RING_BK)) return false;
    return (a.KH == 1 && a.KW == 1) || (a.KH == 3 && a.KW == 3);
}

// The ring kernel wins where HBM and latency bound the conv: 1x1 convs with K <= 768 and no residual
// (tools/chunk_trace.py, chunk of 500 LEF pairs: stage-2 first-block reduce 366 -> 316 us, fused expand+shortcut
// 424 -> 368 us).  Identity-residual expands stay on conv_igemm_persist (2 blocks/CU hide the residual's HBM
// latency: ring 275 -> 315 us); the MFMA-bound ones (3x3, K >= 1024) keep the 256x256 tiles of conv_igemm_big
// (half the L2 -> LDS bytes per FLOP of the ring's 256x128 tile).
inline bool ring_wanted(const ConvArgs& a) {
    return conv_ring_supported(a) && a.KH * a.KW == 1 && a.res == nullptr && conv_ktot(a) <= 768;
}

inline ConvRoute conv_ring_route(const ConvArgs& a) {
    ConvRoute r;
    if (!conv_ring_supported(a)) return r;
    r.kernel = ConvKernel::Ring;
    r.BM = CONV_RING_BM, r.BN = CONV_RING_BN;
    r.tiles = conv_tiles(a, r.BM, r.BN);
    r.name = a.KH == 1 ? "conv_ring_kernel<1, 1>" : "conv_ring_kernel<3, 3>";
    return r;
}

// ---- the tile kernels' dispatch (conv_igemm.hip)
// conv_igemm_p8 at BN 256 / 128: what its K loop needs of the shape, and CBW_CONV_P8
inline bool p8_shape(const ConvArgs& a, const ConvKnobs& k, int BN) {
    return k.conv_p8 == 1 && a.Cout % 256 == BN % 256 && a.Cin % CONV_BK == 0 && a.xfold % CONV_BK == 0;
}
// its epilogue: no GELU, the residual (bf16, fp32 or [hi | lo]) before the activation only
inline bool p8_epilogue(const ConvArgs& a) { return !(a.flags & (CBW_EPI_GELU | CBW_EPI_RES_AFTER_ACT)); }

// CBW_P8_ROWSKIP (default 1): the 3x3 tiles in row order without their all-padding kernel rows (p8_rowmap.h); 0 = the
// (pair, oh, ow) order and all nine taps -- the same bits, the dropped K-tiles added exact zeros.  CBW_P8_ROWGROUP = G
// overrides the group size (0 / unset: p8_default_rowgroup; above N: one group, the flat order).
inline int p8_rowgroup(const ConvArgs& a, const ConvKnobs& k, int BM) {
    if (a.KH * a.KW == 1 || k.p8_rowskip == 0 || a.N <= 0 || (int64_t)a.N * a.Ho * a.Wo != a.M) return 0;
    const int G = k.p8_rowgroup > 0 ? k.p8_rowgroup : p8_default_rowgroup(a.Wo, BM);
    return G < a.N ? G : a.N;
}

inline ConvRoute conv_route(const ConvArgs& a, int ncus, const ConvKnobs& k) {
    const int taps = a.KH * a.KW;
    const auto tile_route = [&](ConvKernel kernel, int BM, int BN, const char* name) {
        ConvRoute r;
        r.kernel = kernel;
        r.BM = BM, r.BN = BN;
        r.tiles = conv_tiles(a, BM, BN);
        r.name = name;
        return r;
    };
    const auto p8_route = [&](int BN) {
        ConvRoute r = tile_route(ConvKernel::P8, conv_p8_bm(BN), BN,
                                 BN == 256 ? CBW_NAME_BY_TAPS(a, "conv_igemm_p8<", ", 256>")
                                           : CBW_NAME_BY_TAPS(a, "conv_igemm_p8<", ", 128>"));
        r.p8_g = p8_rowgroup(a, k, r.BM);
        return r;
    };
    const auto big2_route = [&] {
        return tile_route(ConvKernel::Big2, CONV_BIG_BM, 256, CBW_NAME_BY_TAPS(a, "conv_igemm_big2<256, ", ">"));
    };
    if (!((a.KH == 1 && a.KW == 1) || (a.KH == 3 && a.KW == 3) || (a.KH == 1 && a.KW == 3))) return {};
    if (a.x2 != nullptr && (taps != 1 || a.Cin2 % CONV_BK)) return {};
    // the tile kernels advance A through a 32-bit scalar offset (tap row/col + channel step): it must fit
    const int64_t xld = a.x_ld ? a.x_ld : a.Cin;
    if (((int64_t)(a.KH - 1) * a.W + (a.KW - 1)) * xld + a.Cin + (a.x2 ? a.Cin2 : 0) > INT32_MAX) return {};

    const int ktot = taps * a.Cin;   // without the second source
    // inputs or outputs only the tile kernels (and p8 / big2, which take x_ld, xfold and SPLIT3) understand
    const bool tile_only = a.xfold || (a.x_ld && a.x_ld != a.Cin) || (a.flags & (CBW_EPI_SPLIT3 | CBW_EPI_RES_SPLIT));
    // no residual, bf16 (or split) output, ReLU or none: the MFMA-bound routes of the bf16 pass
    const bool plain = a.res == nullptr && !(a.flags & (CBW_EPI_OUT_F32 | CBW_EPI_GELU | CBW_EPI_RES_SPLIT));
    const bool p8_256 = p8_shape(a, k, 256);
    const bool fills = conv_tiles(a, 256, 256) >= ncus;   // a round of 256 x 256 tiles (p8 256 and big2)

    // folded expand + shortcut (x2): ring / persist -> p8 (CBW_P8_X2 >= 1), streaming -> p8 (CBW_P8_X2 = 2)
    const bool x2_fit = a.x2 && plain && p8_256 && ktot + a.Cin2 >= 512 && !a.xfold && !a.x_ld && fills;
    if (x2_fit && k.p8_x2 >= 2) return p8_route(256);
    if (!tile_only && taps == 1 && conv_stream_wanted(a, k)) return conv_stream_route(a, k);
    if (x2_fit && k.p8_x2 >= 1) return p8_route(256);
    // the compensated tier's convs (CBW_EPI_SPLIT3) at 256 x 256 tiles ("run the tier's stages 3-4
    // at larger tiles"): its expand convs with the [hi | lo] / fp32 residual and its fp32-output shortcuts on p8's
    // residual epilogue, and deep-K convs (K >= 4096: stage 4 at ~400 band pairs, 226 tiles) from half a round of
    // tiles -- one p8 tile's long K loop outruns four 128 x 128 tiles there.  CBW_P8_TIER=0: the tile kernels.
    if (k.p8_tier && (a.flags & (CBW_EPI_SPLIT3 | CBW_EPI_OUT_F32)) && a.xfold && a.x2 == nullptr && p8_256 &&
        p8_epilogue(a) && ktot >= 512 && (fills || (ktot >= 4096 && 2 * conv_tiles(a, 256, 256) >= ncus)))
        return p8_route(256);
    if (!tile_only && ring_wanted(a)) return conv_ring_route(a);
    // MFMA-bound shapes (K >= 256, no residual, bf16 out, no second K-source) -> the 8-wave kernels
    // (conv_igemm_big2 and p8 also take the compensated tier's [hi | lo] inputs and split outputs -- x_ld, xfold,
    // CBW_EPI_SPLIT3 -- so its 3x3 and deep-K 1x1 convs run on the same kernel as the bf16 pass)
    const bool big_ok = plain && a.x2 == nullptr && a.Cin % CONV_BIG_BK == 0 && a.xfold % CONV_BIG_BK == 0 && ktot >= 256;
    // CBW_CONV_P8 (default 1): the 8-phase kernel for the convs conv_igemm_big2 would run (Cout % 256, Cin % 64).
    // tools/layer_bench.py, 625 LEF pairs, big2 -> p8: stage-3 reduce 136 -> 118 us, stage-4 first reduce 231 -> 185,
    // stage-3 first 3x3 230 -> 204, other 3x3s within +-1.5 %; bench.py 4.59 -> 4.72 utt/s (two rounds each)
    // (stage 4's 282 tiles fill 1.1 rounds, but the 4-wave kernel there loses more in the two-stream bench
    // than the tail costs: 5.57 vs 5.69 utt/s)
    // (a 128-wide tile for the few-tile stage-4 convs -- 282 tiles = 1.1 rounds at LEF -- fills the
    // rounds better but loses more per tile: 5.18 -> 5.05 utt/s in bench.py; not taken)
    // 256-wide tiles only: at Cout = 128 (the stage-2 3x3s) the 4-wave 128x128 kernel below is faster
    // (tools/layer_bench.py: 184 vs 202 us stride 1, 229 vs 237 us stride 2; bench.py +0.6 %)
    if (big_ok && fills && a.Cout % 256 == 0) return p8_256 ? p8_route(256) : big2_route();
    // Cout 128 (the stage-2 3x3s): the 8-phase schedule on 512 x 128 tiles (CBW_P8_N128=0: the 4-wave kernel below)
    if (big_ok && k.p8_n128 && p8_shape(a, k, 128) && ktot >= 512 && conv_tiles(a, 512, 128) >= ncus)
        return p8_route(128);
    // the 4-wave kernels step K by 64 and have no tile narrower than 64 channels: what they cannot run is left to
    // big2 (K-steps of 32) at any tile count, or is nobody's.  (No conv of the runtime comes here: every channel
    // count is a multiple of 64.  The chain of ifs this replaces launched a 4-wave kernel that dropped the K tail.)
    if (a.Cin % CONV_BK || a.Cout % 64) return big_ok && a.Cout % 256 == 0 ? big2_route() : ConvRoute{};
    // tile shape: keep BN <= Cout; prefer the 128x128 tile when it divides Cout
    if (a.Cout % 128 == 0) {
        // persistent cross-tile pipelining pays where the per-tile prologue/epilogue is not
        // amortised: a single K-stage, or a residual read in the epilogue (tools/layer_bench.py:
        // S1 expand 493 -> 404 us, S2 expand 298 -> 267 us); deep-K tiles keep the 1-tile kernel.
        const bool short_k = taps * (a.Cin / CONV_BK) == 1;
        if (a.x2 != nullptr || short_k || a.res != nullptr)
            return tile_route(ConvKernel::Persist, 128, 128, CBW_NAME_BY_TAPS(a, "conv_igemm_persist<128, 128, ", ">"));
        return tile_route(ConvKernel::Tile, 128, 128, CBW_NAME_BY_TAPS(a, "conv_igemm_kernel<128, 128, ", ">"));
    }
    if (a.x2 != nullptr) return {};   // dual-source needs Cout % 128 == 0
    return tile_route(ConvKernel::Tile, 256, 64, CBW_NAME_BY_TAPS(a, "conv_igemm_kernel<256, 64, ", ">"));
}

// ---- split-K for few-tile GEMMs (the Whisper encoder's out-projection and fc2 at M = 1500): the K-split factor that
// fills conv_igemm_kernel's 2 blocks per CU with at least 4 K-steps per split (1 = no split)
inline int conv_splitk_factor(const ConvArgs& a, int ncus) {
    if (a.KH != 1 || a.KW != 1 || a.x2 != nullptr || a.Cout % 128 || a.Cin % CONV_BK) return 1;
    const int tiles = conv_tiles(a, 128, 128), slots = 2 * ncus, nsteps = a.Cin / CONV_BK;
    int S = 1;
    while (S < 8 && tiles * (S * 2) <= slots && nsteps / (S * 2) >= 4) S *= 2;
    return S;
}
