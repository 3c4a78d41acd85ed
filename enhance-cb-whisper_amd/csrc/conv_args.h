// The bf16 conv family's launch arguments and epilogue flags.  Plain C++ (no HIP include), so the dispatch policy
// in conv_route.h and its CPU test see the same struct as the kernels.
#pragma once

enum {
    CBW_EPI_RELU = 1,
    CBW_EPI_GELU = 2,
    CBW_EPI_RES_F32 = 4,       // residual operand is fp32 (else bf16)
    CBW_EPI_OUT_F32 = 8,       // output is fp32 (else bf16)
    CBW_EPI_RES_AFTER_ACT = 16, // y = act(acc + bias) + res   (else act(acc + bias + res))
    // compensated bf16 output (the 3-term split re-scoring tier): y is bf16 [M][2*Cout] = [hi | lo] with
    // hi = bf16(v), lo = bf16(v - hi); a following conv reads it with xfold = Cout as the three K-segments
    // [hi | hi | lo] against weights [w_hi | w_lo | w_hi], summing x_hi.w_hi + x_hi.w_lo + x_lo.w_hi in
    // fp32; y32 (optional) receives v in fp32 [M][Cout].  Tile kernels only.
    CBW_EPI_SPLIT3 = 32,
    // residual given as such a [hi | lo] tensor (res_ld = 2*Cout): res = hi + lo
    CBW_EPI_RES_SPLIT = 64
};

struct ConvArgs {
    const void* x;      // [N][H][W][Cin] bf16
    const void* w;      // [Cout][KH][KW][Cin] bf16
    const float* bias;  // [Cout] or null
    const void* res;    // [M][res_ld] or null
    void* y;            // [M][y_ld]
    const void* zero;   // >= 16 bytes of zeros in device memory
    int N, H, W, Cin, Ho, Wo, Cout, KH, KW;
    int sh, sw, ph, pw;
    int M;              // N*Ho*Wo
    int res_ld, y_ld;
    int flags;
    // optional second K-source (1x1 convs only): y = act([x | x2(strided)] . w + bias) with
    // w [Cout][Cin + Cin2]; x2 is [N][H2][W2][Cin2] sampled at (oh*s2, ow*s2).  Used to fold a
    // ResNet shortcut conv into the expand conv of the same block (no shortcut tensor in HBM).
    const void* x2;
    int Cin2, H2, W2, s2;
    // split-K (conv_igemm_kernel only, set by cbw_conv_igemm_splitk): block z of grid.y accumulates K-steps
    // [z nsteps / ksplit, (z + 1) nsteps / ksplit) and stores raw fp32 sums to partial[z][M][Cout]
    int ksplit;
    float* partial;
    float* y32;         // CBW_EPI_SPLIT3: optional fp32 copy of the output, [M][Cout]
    // folded input (tile kernels only): x holds x_ld channels per pixel (0 = Cin); with xfold = C > 0 the K
    // channels [0, Cin = 3C) read physical channels c < C ? c : c - C, i.e. a [hi | lo] tensor (x_ld = 2C)
    // seen as [hi | hi | lo]
    int x_ld, xfold;
    // conv_igemm_p8's 3x3 tiles (ConvRoute::p8_g, see p8_rowmap.h): > 0 = tile rows in (group of p8_g pairs, oh,
    // pair, ow) order with the all-padding kernel rows dropped from each tile's K loop; 0 = (pair, oh, ow) order
    int p8_g;
};
