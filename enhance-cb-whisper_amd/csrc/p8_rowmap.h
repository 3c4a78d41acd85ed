// Row order and K-tile range of conv_igemm_p8's 3x3 tiles (CBW_P8_ROWSKIP).  Plain integer functions, host and
// device, so tests/host/p8_rowmap_check.cpp can brute-force them on the CPU.
//
// A 3x3 conv with padding 1 reads a padding row at kernel row 0 of the top image row and (usually) at kernel row 2 of
// the bottom one.  In (pair, oh, ow) order every 256- / 512-pixel tile holds all image rows of a few pairs, so it
// walks all nine taps and multiplies the zero page for the padding ones.  In the order
//     (group of G pairs, oh, pair within the group, ow)
// a tile lies (mostly) inside one image row of one group, and the kernel rows that are padding for every pixel of
// the tile are dropped from its K loop.  Only the map from a tile's logical row to the pixel changes: the tensors
// stay NHWC per pair.
#pragma once

#if defined(__HIPCC__)
#define CBW_HD __host__ __device__ __forceinline__
#else
#define CBW_HD inline
#endif

// Logical row L in [0, N Ho Wo) -> its pixel (n, oh, ow) and its group grp = n / G.  Groups hold G pairs (G >= 1; G > N
// counts as N: one group, the flat order), the last one the N - grp G that remain, and its rows decode with that count.
// A bijection of [0, N Ho Wo) onto the pixels: groups are contiguous row ranges of (pairs in group) Ho Wo rows each.
CBW_HD void p8_row_pixel(int L, int N, int Ho, int Wo, int G, int& n, int& oh, int& ow, int& grp) {
    if (G > N) G = N;
    grp = L / (G * Ho * Wo);
    const int l = L - grp * (G * Ho * Wo);
    const int left = N - grp * G;
    const int rowlen = (left < G ? left : G) * Wo;   // pixels of one image row of the group
    oh = l / rowlen;
    const int rem = l - oh * rowlen;
    const int p = rem / Wo;
    ow = rem - p * Wo;
    n = grp * G + p;
}

// The kernel rows [kh_lo, kh_hi) a tile has to walk, from its first and last valid logical rows (oh_first, oh_last;
// same_group: both in one group).  Inside a group the rows ascend in oh, so every row of the tile has oh in
// [oh_first, oh_last], and tap row kh reads input row ih = oh sh - ph + kh: it is padding for all of them when
// kh < ph - oh_last sh (above the image even for the lowest row) or kh >= H + ph - oh_first sh (below it even for
// the topmost).  Conservative: a tile over two groups, or one whose range would come out empty, walks all KH rows;
// the per-row tap masks still decide every load, so nothing depends on a tile being inside one image row.
CBW_HD void p8_kh_range(int oh_first, int oh_last, bool same_group, int H, int sh, int ph, int KH, int& kh_lo,
                        int& kh_hi) {
    kh_lo = 0;
    kh_hi = KH;
    if (!same_group) return;
    const int lo = ph - oh_last * sh, hi = H + ph - oh_first * sh;
    const int clo = lo > 0 ? lo : 0, chi = hi < KH ? hi : KH;
    if (clo < chi) {
        kh_lo = clo;
        kh_hi = chi;
    }
}

// Group size for a conv with rows of Wo output pixels on tiles of BM rows.  A tile over the boundary of the first or
// the last image row of a group loses its skip (about BM / (G Wo) of them), so G Wo should be a multiple of BM or
// large; a small G keeps the tiles of rows oh - 1, oh, oh + 1 of the same pairs close together on one XCD (they
// re-read the same input rows from its L2).  The smallest G <= 64 with G Wo a multiple of BM (Wo 24, BM 256: 32, three
// tiles per row exactly), else nine tiles per row (Wo 47, BM 256 and Wo 94, BM 512: 49).
inline int p8_default_rowgroup(int Wo, int BM) {
    for (int G = 1; G <= 64; ++G)
        if ((G * Wo) % BM == 0) return G;
    const int G = 9 * BM / Wo;
    return G > 0 ? G : 1;
}
