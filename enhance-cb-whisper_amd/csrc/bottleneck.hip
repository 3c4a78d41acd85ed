// Fused ResNet-50 stage-1 bottleneck blocks for gfx950: reduce 1x1 (CIN -> 64) + BN + ReLU,
// 3x3 (64 -> 64) + BN + ReLU, expand 1x1 (64 -> 256) + BN, residual, ReLU -- one persistent
// launch per block; the two 64-channel intermediates never leave LDS.  One template serves both
// block kinds of the stage:
//   CIN = 256  (blocks 2, 3)  identity residual: y = relu(T2 . We + be + x)
//   CIN = 64   (block 1)      projection shortcut folded into the expand as a second K-source:
//                             y = relu([T2 | x] . [We | Ws] + be + bs)  (load_fused_expand_shortcut)
//
// Reference: HF ResNetBottleNeckLayer as instantiated by efficient_kws/resnet.py:22-38 and run by
// Resnet.forward (resnet.py:51-58): stage 1.  The unfused path (three conv launches) moves 7.3 MB
// per pair through HBM per block at LEF sizes; this kernel reads the block input once (+ halo
// columns) and writes the block output once.
//
// Work unit: one pair x TH (19) output rows x TW (6) output columns.  One 512-thread workgroup per
// CU (two waves per SIMD) walks a contiguous range of tiles; consecutive column tiles share their
// halo columns, which the previous tile has just pulled into L2.  LDS: the tile's input window X
// (168 px, CIN channels; 16-byte chunk index ^ (row & SWM); double-buffered for CIN = 64), Wr (same
// layout), T1 (halo window x 64 ch) and T2 (128 px x 64 ch) (144-byte pixel pitch), biases.  Each
// wave keeps its Wm / We slices in registers.  Per tile:
//   phase R  T1 = relu(X . Wr + br), 0 outside the image (the 3x3's zero padding); wave (mq, nh):
//            32 channels x 3 pixel fragments.  (CIN = 256) the residual the wave adds in phase E is
//            copied from X to registers; then the NEXT tile's window is issued into X and lands
//            while phases M and E compute.
//   phase M  T2 = relu(conv3x3(T1) . Wm + bm); wave (mh, nq): 16 channels x 4 fragments.
//   phase E  y = relu(T2 . We + be (+ x)); wave w: 32 channels x 8 fragments (two passes).
// All MFMAs run transposed (C^T = W . X^T): a lane ends with 4 consecutive channels of one pixel.
//
// Round 2 (issue diet): the round-1 kernels spent ~1200 VALU per wave and tile on address and mask
// arithmetic against 152 MFMAs (VALU-issue bound).  Now every lane-dependent LDS address, window
// DMA offset and store offset is computed once per launch (tile-independent: the per-tile part is
// one scalar offset), LDS reads use immediate offsets, the window arrives by buffer DMA
// (raw_buffer_load_lds: rows past either end of the image read 0, rows wrapping into a
// neighbouring row are masked by T1's validity), biases seed the MFMA accumulators, and ReLU runs
// on packed bf16 (v_pk_max_i16 after rounding: max(bf16, +0) as int16 is relu for every non-NaN
// value).  Tiles away from the column edges of an LEF-shaped map (H = TH) take precomputed masks;
// the others (edge columns, other heights) compute them.
#include <algorithm>
#include <climits>
#include <cstdlib>

#include "cbw_common.h"
#include "cbw_kernels.h"
#ifndef BT_BIAS_EPI
#define BT_BIAS_EPI 0   // diagnostic: 1 adds the biases in the epilogues (the three-conv path's rounding order)
#endif

typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// raw buffer store / LDS-DMA load (LLVM intrinsics by asm label): lanes whose byte offset is past
// num_records are dropped (store) or read 0 (load), so every wave issues the same number of them
// per tile and the top-of-tile wait can be a counted vmcnt that leaves the stores in flight.
__device__ void raw_buffer_store_v2i32(i32x2 vdata, i32x4 rsrc, int voffset, int soffset, int aux)
    __asm("llvm.amdgcn.raw.buffer.store.v2i32");
__device__ void raw_buffer_store_v4i32(i32x4 vdata, i32x4 rsrc, int voffset, int soffset, int aux)
    __asm("llvm.amdgcn.raw.buffer.store.v4i32");
__device__ void raw_buffer_store_i32(int vdata, i32x4 rsrc, int voffset, int soffset, int aux)
    __asm("llvm.amdgcn.raw.buffer.store.i32");
__device__ void raw_buffer_load_lds(i32x4 rsrc, __attribute__((address_space(3))) void* lds, int size, int voffset,
                                    int soffset, int offset, int aux) __asm("llvm.amdgcn.raw.buffer.load.lds");

namespace {

constexpr int BT_TH = 19, BT_TW = 6;
constexpr int BT_COUT = 256;
constexpr int BT_WW = BT_TW + 2;                   // halo window width (8: row >> 3 = window row)
constexpr int BT_P1 = (BT_TH + 2) * BT_WW;         // 168 halo-window pixels
constexpr int BT_FR = ((BT_P1 + 15) / 16 + 3) / 4; // phase R fragments per pixel quarter: 3 (11 + a dummy)
constexpr int BT_P2 = BT_TH * BT_TW;               // 114 output pixels
constexpr int BT_F2 = (BT_P2 + 15) / 16;           // 8 fragments
constexpr int BT_FM = (BT_F2 + 1) / 2;             // phase M fragments per pixel half: 4
constexpr int BT_FE = (BT_F2 + 1) / 2;             // phase E fragments per half-pass: 4
constexpr int BT_PITCH = 144;                      // T1 / T2 bytes per pixel (64 ch + 16 pad)
constexpr int BT_T2ROWS = BT_F2 * 16;              // 128: phase M writes whole fragments, unmasked
constexpr int BT_FRAG = 16 * BT_PITCH;             // T1 / T2 bytes per 16-pixel fragment
constexpr uint32_t BT_OOB = 0x80000000u;           // a buffer offset past any num_records
static_assert(2 * BT_FE == 8, "top-of-tile vmcnt assumes 8 y stores per wave");

template <int CIN>
struct BtL {
    static constexpr int XROW = CIN * 2;                 // window bytes per pixel
    static constexpr int XC = CIN / 8;                   // 16-byte chunks per pixel
    static constexpr int SWM = XC >= 16 ? 15 : XC - 1;   // chunk swizzle mask
    static constexpr int UM = SWM >> 2;                  // swizzled chunk bits above the lane's 2 (3 / 1)
    static constexpr int NXB = CIN == 64 ? 2 : 1;        // window buffers
    static constexpr int X_BYTES = BT_P1 * XROW;         // 86016 / 21504
    static constexpr int WR = NXB * X_BYTES;             // Wr [64][CIN] bf16, swizzled like X
    static constexpr int T1 = WR + 64 * XROW;
    static constexpr int T2 = T1 + BT_P1 * BT_PITCH;     // + 24192
    static constexpr int BIAS = T2 + BT_T2ROWS * BT_PITCH;   // + 18432: br [64], bm [64], be [256] f32
    static constexpr int LDS = BIAS + (64 + 64 + 256) * 4;   // 162944 / 95360
    static constexpr int RPI = 1024 / XROW;              // window rows per DMA wave-instruction
    static constexpr int XG = (BT_P1 + 8 * RPI - 1) / (8 * RPI);   // window DMA rounds: 11 / 3
    static constexpr int KS = XC / 4;                    // phase-R k-steps: 8 / 2
    static constexpr int KE = CIN == 64 ? 4 : 2;         // phase-E k-steps: T2 (+ the shortcut's x)
    static_assert(LDS <= 163840, "LDS budget");
    static_assert((BT_P1 % RPI == 0 && BT_WW % RPI == 0) || RPI % BT_WW == 0, "window rows per wave-instruction");
};

CBW_DEV i32x4 buffer_rsrc(const void* base, uint32_t bytes) {
    const uint64_t a = (uint64_t)base;
    return i32x4{(int)(uint32_t)a, (int)(uint32_t)(a >> 32), (int)bytes, 0x00020000};
}

template <typename T>
CBW_DEV T lds_at(const char* smem, int byte) { return *(const T*)(smem + byte); }

// two fp32 -> bf16 (RNE) -> relu on the packed pair
CBW_DEV uint32_t relu_pk(float a, float b) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    s16x2 v = __builtin_bit_cast(s16x2, __builtin_convertvector((f32x2{a, b}), bf16x2));   // one v_cvt_pk_bf16_f32
    v = __builtin_elementwise_max(v, s16x2{0, 0});
    return __builtin_bit_cast(uint32_t, v);
}

CBW_DEV float bf_lo(uint32_t u) { return __builtin_bit_cast(float, u << 16); }
CBW_DEV float bf_hi(uint32_t u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

// Q8: the block output stored as e4m3(bf16(relu(.)) * q8_inv) (the fp8 tier's first tensor, conv_fp8.hip's
// pack8_fp8 arithmetic on the bf16 values the Q8 = false instance stores): the separate quantization pass over the
// stage-1 output (read bf16, write e4m3) and half the block's output bytes disappear
template <int CIN, bool Q8, bool MERGE = false>
__global__ __launch_bounds__(512, 1) void bottleneck_kernel(const bf16* __restrict__ x, void* __restrict__ y,
                                                            const bf16* __restrict__ wr, const float* __restrict__ br,
                                                            const bf16* __restrict__ wm, const float* __restrict__ bm,
                                                            const bf16* __restrict__ we, const float* __restrict__ be,
                                                            int N, int H, int W, int nrt, int nct, float q8_inv) {
    using L = BtL<CIN>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Bs = (float*)(smem + L::BIAS);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int mh = wid >> 2, nq = wid & 3;     // phase M: pixel half x channel quarter
    const int mq = wid >> 1, nh = wid & 1;     // phase R: pixel quarter x channel half
    const int ntiles = N * nrt * nct;
    const int G = gridDim.x;
    constexpr int YB = Q8 ? 1 : 2;   // output bytes per element
    const uint32_t x_bytes = (uint32_t)H * W * L::XROW, y_bytes = (uint32_t)H * W * BT_COUT * YB;

    // ---- once per workgroup: Wr and the biases -> LDS, this wave's Wm / We slices -> registers
#pragma unroll
    for (int k = 0; k < 64 * L::XC / 512; ++k) {
        const int e = k * 512 + tid;             // 16-byte chunk e of Wr: row e / XC, chunk e % XC
        const int row = (unsigned)e / L::XC, c = e & (L::XC - 1);
        *(bf16x8*)(smem + L::WR + row * L::XROW + ((c ^ (row & L::SWM)) << 4)) = *(const bf16x8*)(wr + row * CIN + c * 8);
    }
    if (tid < 64) Bs[tid] = br[tid];
    else if (tid < 128) Bs[tid] = bm[tid - 64];
    if (tid < 256) Bs[128 + tid] = be[tid];
    bf16x8 wmf[18];                // Wm [64][3][3][64]: out ch 16 nq + fr, k-step (tap, half)
#pragma unroll
    for (int s = 0; s < 18; ++s) wmf[s] = *(const bf16x8*)(wm + (nq * 16 + fr) * 576 + s * 32 + fq * 8);
    // We [256][32 KE]: MFMA row fr of channel tile j = out ch 32 w + 8 (fr >> 2) + 4 j + (fr & 3), so a lane's two
    // tiles give it 8 consecutive channels (32 w + 8 fq ..) of its pixel: 16-byte residual reads and stores (the
    // 8-byte store tail was issue-bound)
    bf16x8 wef[2][L::KE];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ks = 0; ks < L::KE; ++ks)
            wef[j][ks] = *(const bf16x8*)(we + (wid * 32 + 8 * (fr >> 2) + 4 * j + (fr & 3)) * (32 * L::KE) + ks * 32 +
                                          fq * 8);

    // ---- per-lane, tile-independent addresses
    // window DMA: wave-instruction g writes rows RPI (8 g + w) .. + RPI - 1 (lane / XC), chunk lane % XC
    // (source chunk pre-swizzled, LDS destination linear); byte offset from the window origin pixel
    int wo[L::XG];
#pragma unroll
    for (int g = 0; g < L::XG; ++g) {
        const int row = (g * 8 + wid) * L::RPI + (int)((unsigned)lane / L::XC);
        const int c = lane & (L::XC - 1);
        wo[g] = ((row >> 3) * W + (row & 7)) * L::XROW + ((c ^ (row & L::SWM)) << 4);
    }
    // phase R: chunk (4 s + fq) of rows 16 f + fr, swizzled by fr & SWM; the k-step's bits above the
    // lane's two select one of UM + 1 bases, the rest is an immediate
    const int fsw = fr & L::SWM;
    int xr_base[L::UM + 1], wr_base[L::UM + 1];
#pragma unroll
    for (int u = 0; u <= L::UM; ++u) {
        const int lo = ((fq ^ (fsw & 3)) << 4) + ((u ^ (fsw >> 2)) << 6);
        xr_base[u] = (mq * BT_FR * 16 + fr) * L::XROW + lo;
        wr_base[u] = L::WR + (nh * 32 + fr) * L::XROW + lo;
    }
    // T1 rows of phase R's fragments; their validity for an LEF-shaped tile (h0 = 0, H = TH, interior columns)
    const int t1w = L::T1 + (mq * BT_FR * 16 + fr) * BT_PITCH + (nh * 32 + fq * 4) * 2;
    bool okf[BT_FR];
#pragma unroll
    for (int i = 0; i < BT_FR; ++i) {
        const int ii = ((mq * BT_FR + i) * 16 + fr) >> 3;
        okf[i] = ii >= 1 && ii <= BT_TH;
    }
    // phase M: T1 pixel of output q's (0, 0) tap
    int pb[BT_FM];
#pragma unroll
    for (int i = 0; i < BT_FM; ++i) {
        const int q = (mh * BT_FM + i) * 16 + fr;    // q >= 114: dummy rows, results dropped
        pb[i] = L::T1 + ((q / BT_TW) * BT_WW + q % BT_TW) * BT_PITCH + fq * 16;
    }
    const int t2w = L::T2 + (mh * BT_FM * 16 + fr) * BT_PITCH + (nq * 16 + fq * 4) * 2;
    const int t2r = L::T2 + fr * BT_PITCH + fq * 16;
    // phase E: window pixel of output q -- CIN 256: residual channels 32 w + 8 fq .. + 7;
    // CIN 64: the shortcut's chunk fq (+4: ^ 64) -- and the y store offset from the tile origin
    int xa[BT_F2];
    uint32_t so[BT_F2];
#pragma unroll
    for (int k = 0; k < BT_F2; ++k) {
        const int q = k * 16 + fr;
        const int r = q / BT_TW, c = q - r * BT_TW;
        const int row = (r + 1) * BT_WW + c + 1;
        if (CIN == 256) xa[k] = row * L::XROW + (((wid * 4 + fq) ^ (row & L::SWM)) << 4);
        else xa[k] = row * L::XROW + ((fq ^ (row & L::SWM)) << 4);
        so[k] = q < BT_P2 ? (uint32_t)(((r * W + c) * BT_COUT + wid * 32 + fq * 8) * YB) : BT_OOB;
    }

    // contiguous tile range per workgroup: consecutive column tiles share their halo columns
    const int per = (ntiles + G - 1) / G;
    const int t0 = blockIdx.x * per, t1 = min(ntiles, t0 + per);
    if (t0 >= t1) return;
    int n = t0 / (nrt * nct), rt, ct;
    {
        const int rem = t0 - n * (nrt * nct);
        rt = rem / nct;
        ct = rem - rt * nct;
    }
    // the window of tile (nn, h0, w0) -> LDS byte offset xb (window rows outside the image are
    // don't-care: T1's validity zeroes their pixels; wave-instructions holding only such rows are skipped)
    auto issue_window = [&](int nn, int h0, int w0, int xb) {
        const i32x4 xr = buffer_rsrc(x + (int64_t)nn * H * W * CIN, x_bytes);
        const int toff = ((h0 - 1) * W + (w0 - 1)) * L::XROW;
        const bool top_pad = h0 == 0, bot_pad = h0 + BT_TH >= H;
#pragma unroll
        for (int g = 0; g < L::XG; ++g) {
            const int r0 = (g * 8 + wid) * L::RPI;
            if (r0 >= BT_P1) break;                                          // wave-uniform
            if ((r0 + L::RPI <= BT_WW && top_pad) || (r0 >= BT_P1 - BT_WW && bot_pad)) continue;
            raw_buffer_load_lds(xr, (__attribute__((address_space(3))) void*)(smem + xb + r0 * L::XROW), 16,
                                wo[g] + toff, 0, 0, 0);
        }
    };

    if constexpr (MERGE && CIN == 64) {
        // MERGE (CIN 64, the first block): tile t-1's phase E and tile t's phase R in one barrier interval (E reads T2 and
        // tile t-1's window buffer for the shortcut, R reads tile t's window buffer and writes T1: disjoint), two
        // barriers per tile instead of three; tile t+1's window goes into tile t-1's buffer after that interval and each
        // wave retires it at the end of phase M(t)
        issue_window(n, rt * BT_TH, ct * BT_TW, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        bool pend = false;
        int en = 0, eh0 = 0, ew0 = 0, exb = 0;
        auto phase_e = [&]() {
        // ---- phase E: wave w = channels 32 w .., two passes of BT_FE fragments
        {
            const i32x4 yr = buffer_rsrc((const char*)y + (int64_t)en * H * W * BT_COUT * YB, y_bytes);
            const uint32_t tso = (uint32_t)((eh0 * W + ew0) * BT_COUT * YB);
            const bool cols_in = ew0 + BT_TW <= W;   // rows past H fall past num_records by themselves
            const f32x4 bev[2] = {lds_at<f32x4>(smem, L::BIAS + (128 + wid * 32 + fq * 8) * 4),
                                  lds_at<f32x4>(smem, L::BIAS + (128 + wid * 32 + fq * 8 + 4) * 4)};
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f32x4 ae[BT_FE][2];
#pragma unroll
                for (int ks = 0; ks < L::KE; ++ks)
#pragma unroll
                    for (int i = 0; i < BT_FE; ++i) {
                        const int k = half * BT_FE + i;
                        const bf16x8 av = ks < 2 ? lds_at<bf16x8>(smem, t2r + k * BT_FRAG + ks * 64)
                                                 : lds_at<bf16x8>(smem, exb + (xa[k] ^ ((ks - 2) * 64)));
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            ae[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wef[j][ks], av, ks == 0 ? (BT_BIAS_EPI ? f32x4{0.f, 0.f, 0.f, 0.f} : bev[j]) : ae[i][j], 0, 0, 0);
                    }
#pragma unroll
                for (int i = 0; i < BT_FE; ++i) {
                    const int k = half * BT_FE + i;
                    uint32_t off = so[k] + tso;
                    if (!cols_in) {
                        const int q = k * 16 + fr;
                        if (ew0 + q % BT_TW >= W) off = BT_OOB;
                    }
                    uint32_t o[4];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        f32x4 v = ae[i][j];
                        if (BT_BIAS_EPI) v += bev[j];
                        o[2 * j] = relu_pk(v[0], v[1]);
                        o[2 * j + 1] = relu_pk(v[2], v[3]);
                    }
                    if constexpr (Q8) {
                        int pk[2];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const float q0 = fminf(fmaxf(bf_lo(o[2 * h]) * q8_inv, -448.f), 448.f);
                            const float q1 = fminf(fmaxf(bf_hi(o[2 * h]) * q8_inv, -448.f), 448.f);
                            const float q2 = fminf(fmaxf(bf_lo(o[2 * h + 1]) * q8_inv, -448.f), 448.f);
                            const float q3 = fminf(fmaxf(bf_hi(o[2 * h + 1]) * q8_inv, -448.f), 448.f);
                            pk[h] = __builtin_amdgcn_cvt_pk_fp8_f32(q0, q1, 0, false);
                            pk[h] = __builtin_amdgcn_cvt_pk_fp8_f32(q2, q3, pk[h], true);
                        }
                        raw_buffer_store_v2i32(i32x2{pk[0], pk[1]}, yr, (int)off, 0, 0);
                    } else {
                        raw_buffer_store_v4i32(i32x4{(int)o[0], (int)o[1], (int)o[2], (int)o[3]}, yr, (int)off, 0, 0);
                    }
                }
            }
        }
        };
        for (int t = t0; t < t1; ++t) {
            const int h0 = rt * BT_TH, w0 = ct * BT_TW;
            const int xb = ((t - t0) & 1) * L::X_BYTES;
            int nn = n, nrt_ = rt, nct_ = ct + 1;
            if (nct_ == nct) {
                nct_ = 0;
                if (++nrt_ == nrt) {
                    nrt_ = 0;
                    ++nn;
                }
            }
            const bool lef = h0 == 0 && H == BT_TH && w0 >= 1 && w0 + BT_WW - 1 <= W;
            if (pend) phase_e();
        // ---- phase R: wave (mq, nh) = fragments 3 mq .. 3 mq + 2 x channels 32 nh ..
        f32x4 ar[BT_FR][2];
        {
            const f32x4 brv[2] = {lds_at<f32x4>(smem, L::BIAS + (nh * 32 + fq * 4) * 4),
                                  lds_at<f32x4>(smem, L::BIAS + (nh * 32 + 16 + fq * 4) * 4)};
#pragma unroll
            for (int s = 0; s < L::KS; ++s) {
                const int u = s & L::UM, hi = (s & ~L::UM) * 64;
                bf16x8 bv[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) bv[j] = lds_at<bf16x8>(smem, wr_base[u] + j * 16 * L::XROW + hi);
#pragma unroll
                for (int i = 0; i < BT_FR; ++i) {   // rows past the window read other LDS: discarded
                    const bf16x8 av = lds_at<bf16x8>(smem, xb + xr_base[u] + i * 16 * L::XROW + hi);
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        ar[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bv[j], av, s == 0 ? (BT_BIAS_EPI ? f32x4{0.f, 0.f, 0.f, 0.f} : brv[j]) : ar[i][j], 0, 0, 0);
                }
            }
        }
        // T1 = relu(.), 0 outside the image; rows past the window (p >= 168) land in T2's first rows,
        // which phase M rewrites before anything reads them
#pragma unroll
        for (int i = 0; i < BT_FR; ++i) {
            bool ok = okf[i];
            if (!lef) {
                const int p = (mq * BT_FR + i) * 16 + fr;
                ok = (unsigned)(h0 - 1 + (p >> 3)) < (unsigned)H && (unsigned)(w0 - 1 + (p & 7)) < (unsigned)W;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f32x4 v = ar[i][j];
                if (BT_BIAS_EPI) v += lds_at<f32x4>(smem, L::BIAS + (nh * 32 + j * 16 + fq * 4) * 4);
                u32x2 o = {relu_pk(v[0], v[1]), relu_pk(v[2], v[3])};
                if (!ok) o = u32x2{0u, 0u};
                *(u32x2*)(smem + t1w + i * BT_FRAG + j * 32) = o;
            }
        }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (t + 1 < t1) issue_window(nn, nrt_ * BT_TH, nct_ * BT_TW, ((t - t0 + 1) & 1) * L::X_BYTES);
        // ---- phase M: wave (mh, nq) = fragments 4 mh .. 4 mh + 3 x channels 16 nq ..
        {
            const f32x4 bmv = lds_at<f32x4>(smem, L::BIAS + (64 + nq * 16 + fq * 4) * 4);
            f32x4 am[BT_FM];
            // fragment i of k-step ks + 1 is requested right after k-step ks's MFMA on fragment i (a rotating buffer of
            // BT_FM registers: one k-step of reads in flight at no register cost; before, each MFMA waited for its own
            // just-issued read)
            auto maddr = [&](int ks, int i) {
                const int tap = ks >> 1, hh = ks & 1;
                return pb[i] + ((tap / 3) * BT_WW + (tap % 3)) * BT_PITCH + hh * 64;
            };
            bf16x8 mv[BT_FM];
#pragma unroll
            for (int i = 0; i < BT_FM; ++i) mv[i] = lds_at<bf16x8>(smem, maddr(0, i));
#pragma unroll
            for (int ks = 0; ks < 18; ++ks)
#pragma unroll
                for (int i = 0; i < BT_FM; ++i) {
                    am[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wmf[ks], mv[i],
                                                                    ks == 0 ? (BT_BIAS_EPI ? f32x4{0.f, 0.f, 0.f, 0.f} : bmv) : am[i], 0, 0, 0);
                    if (ks + 1 < 18) mv[i] = lds_at<bf16x8>(smem, maddr(ks + 1, i));
                }
#pragma unroll
            for (int i = 0; i < BT_FM; ++i) {
                if (BT_BIAS_EPI) am[i] += bmv;
                *(u32x2*)(smem + t2w + i * BT_FRAG) = u32x2{relu_pk(am[i][0], am[i][1]), relu_pk(am[i][2], am[i][3])};
            }
        }
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            pend = true;
            en = n;
            eh0 = h0;
            ew0 = w0;
            exb = xb;
            n = nn;
            rt = nrt_;
            ct = nct_;
        }
        if (pend) phase_e();
        return;
    }
    issue_window(n, rt * BT_TH, ct * BT_TW, 0);
    for (int t = t0; t < t1; ++t) {
        const int h0 = rt * BT_TH, w0 = ct * BT_TW;
        const int xb = L::NXB == 2 ? ((t - t0) & 1) * L::X_BYTES : 0;   // this tile's window
        int nn = n, nrt_ = rt, nct_ = ct + 1;                            // the next tile
        if (nct_ == nct) {
            nct_ = 0;
            if (++nrt_ == nrt) {
                nrt_ = 0;
                ++nn;
            }
        }
        // this tile's window has landed (own DMAs; the previous tile's y stores may stay in flight),
        // every other wave's as well, and every wave is done with the previous tile
        if (t == t0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // double buffer: the next window streams in during this whole tile (issued before this tile's
        // 8 y stores, so the next top-of-tile vmcnt(8) still means "window landed")
        if (L::NXB == 2 && t + 1 < t1) issue_window(nn, nrt_ * BT_TH, nct_ * BT_TW, ((t - t0 + 1) & 1) * L::X_BYTES);
        const bool lef = h0 == 0 && H == BT_TH && w0 >= 1 && w0 + BT_WW - 1 <= W;   // precomputed masks hold

        // ---- phase R: wave (mq, nh) = fragments 3 mq .. 3 mq + 2 x channels 32 nh ..
        f32x4 ar[BT_FR][2];
        {
            const f32x4 brv[2] = {lds_at<f32x4>(smem, L::BIAS + (nh * 32 + fq * 4) * 4),
                                  lds_at<f32x4>(smem, L::BIAS + (nh * 32 + 16 + fq * 4) * 4)};
#pragma unroll
            for (int s = 0; s < L::KS; ++s) {
                const int u = s & L::UM, hi = (s & ~L::UM) * 64;
                bf16x8 bv[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) bv[j] = lds_at<bf16x8>(smem, wr_base[u] + j * 16 * L::XROW + hi);
#pragma unroll
                for (int i = 0; i < BT_FR; ++i) {   // rows past the window read other LDS: discarded
                    const bf16x8 av = lds_at<bf16x8>(smem, xb + xr_base[u] + i * 16 * L::XROW + hi);
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        ar[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bv[j], av, s == 0 ? (BT_BIAS_EPI ? f32x4{0.f, 0.f, 0.f, 0.f} : brv[j]) : ar[i][j], 0, 0, 0);
                }
            }
        }
        // (CIN 256) the residual this wave adds in phase E: channels 32 w + 8 fq .. + 7, pixel 16 k + fr
        u32x4 res[BT_F2];
        if (CIN == 256) {
#pragma unroll
            for (int k = 0; k < BT_F2; ++k) res[k] = lds_at<u32x4>(smem, xa[k]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();          // X is free: the next window streams in during M and E
            if (t + 1 < t1) issue_window(nn, nrt_ * BT_TH, nct_ * BT_TW, 0);
        }
        // T1 = relu(.), 0 outside the image; rows past the window (p >= 168) land in T2's first rows,
        // which phase M rewrites before anything reads them
#pragma unroll
        for (int i = 0; i < BT_FR; ++i) {
            bool ok = okf[i];
            if (!lef) {
                const int p = (mq * BT_FR + i) * 16 + fr;
                ok = (unsigned)(h0 - 1 + (p >> 3)) < (unsigned)H && (unsigned)(w0 - 1 + (p & 7)) < (unsigned)W;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f32x4 v = ar[i][j];
                if (BT_BIAS_EPI) v += lds_at<f32x4>(smem, L::BIAS + (nh * 32 + j * 16 + fq * 4) * 4);
                u32x2 o = {relu_pk(v[0], v[1]), relu_pk(v[2], v[3])};
                if (!ok) o = u32x2{0u, 0u};
                *(u32x2*)(smem + t1w + i * BT_FRAG + j * 32) = o;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();

        // ---- phase M: wave (mh, nq) = fragments 4 mh .. 4 mh + 3 x channels 16 nq ..
        {
            const f32x4 bmv = lds_at<f32x4>(smem, L::BIAS + (64 + nq * 16 + fq * 4) * 4);
            f32x4 am[BT_FM];
            // fragment i of k-step ks + 1 is requested right after k-step ks's MFMA on fragment i (a rotating buffer of
            // BT_FM registers: one k-step of reads in flight at no register cost; before, each MFMA waited for its own
            // just-issued read)
            auto maddr = [&](int ks, int i) {
                const int tap = ks >> 1, hh = ks & 1;
                return pb[i] + ((tap / 3) * BT_WW + (tap % 3)) * BT_PITCH + hh * 64;
            };
            bf16x8 mv[BT_FM];
#pragma unroll
            for (int i = 0; i < BT_FM; ++i) mv[i] = lds_at<bf16x8>(smem, maddr(0, i));
#pragma unroll
            for (int ks = 0; ks < 18; ++ks)
#pragma unroll
                for (int i = 0; i < BT_FM; ++i) {
                    am[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wmf[ks], mv[i],
                                                                    ks == 0 ? (BT_BIAS_EPI ? f32x4{0.f, 0.f, 0.f, 0.f} : bmv) : am[i], 0, 0, 0);
                    if (ks + 1 < 18) mv[i] = lds_at<bf16x8>(smem, maddr(ks + 1, i));
                }
#pragma unroll
            for (int i = 0; i < BT_FM; ++i) {
                if (BT_BIAS_EPI) am[i] += bmv;
                *(u32x2*)(smem + t2w + i * BT_FRAG) = u32x2{relu_pk(am[i][0], am[i][1]), relu_pk(am[i][2], am[i][3])};
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();

        // ---- phase E: wave w = channels 32 w .., two passes of BT_FE fragments
        {
            const i32x4 yr = buffer_rsrc((const char*)y + (int64_t)n * H * W * BT_COUT * YB, y_bytes);
            const uint32_t tso = (uint32_t)((h0 * W + w0) * BT_COUT * YB);
            const bool cols_in = w0 + BT_TW <= W;   // rows past H fall past num_records by themselves
            const f32x4 bev[2] = {lds_at<f32x4>(smem, L::BIAS + (128 + wid * 32 + fq * 8) * 4),
                                  lds_at<f32x4>(smem, L::BIAS + (128 + wid * 32 + fq * 8 + 4) * 4)};
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f32x4 ae[BT_FE][2];
#pragma unroll
                for (int ks = 0; ks < L::KE; ++ks)
#pragma unroll
                    for (int i = 0; i < BT_FE; ++i) {
                        const int k = half * BT_FE + i;
                        const bf16x8 av = ks < 2 ? lds_at<bf16x8>(smem, t2r + k * BT_FRAG + ks * 64)
                                                 : lds_at<bf16x8>(smem, xb + (xa[k] ^ ((ks - 2) * 64)));
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            ae[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wef[j][ks], av, ks == 0 ? (BT_BIAS_EPI ? f32x4{0.f, 0.f, 0.f, 0.f} : bev[j]) : ae[i][j], 0, 0, 0);
                    }
#pragma unroll
                for (int i = 0; i < BT_FE; ++i) {
                    const int k = half * BT_FE + i;
                    uint32_t off = so[k] + tso;
                    if (!cols_in) {
                        const int q = k * 16 + fr;
                        if (w0 + q % BT_TW >= W) off = BT_OOB;
                    }
                    uint32_t o[4];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        f32x4 v = ae[i][j];
                        if (BT_BIAS_EPI) v += bev[j];
                        if (CIN == 256) {
                            v[0] += bf_lo(res[k][2 * j]);
                            v[1] += bf_hi(res[k][2 * j]);
                            v[2] += bf_lo(res[k][2 * j + 1]);
                            v[3] += bf_hi(res[k][2 * j + 1]);
                        }
                        o[2 * j] = relu_pk(v[0], v[1]);
                        o[2 * j + 1] = relu_pk(v[2], v[3]);
                    }
                    if constexpr (Q8) {
                        int pk[2];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const float q0 = fminf(fmaxf(bf_lo(o[2 * h]) * q8_inv, -448.f), 448.f);
                            const float q1 = fminf(fmaxf(bf_hi(o[2 * h]) * q8_inv, -448.f), 448.f);
                            const float q2 = fminf(fmaxf(bf_lo(o[2 * h + 1]) * q8_inv, -448.f), 448.f);
                            const float q3 = fminf(fmaxf(bf_hi(o[2 * h + 1]) * q8_inv, -448.f), 448.f);
                            pk[h] = __builtin_amdgcn_cvt_pk_fp8_f32(q0, q1, 0, false);
                            pk[h] = __builtin_amdgcn_cvt_pk_fp8_f32(q2, q3, pk[h], true);
                        }
                        raw_buffer_store_v2i32(i32x2{pk[0], pk[1]}, yr, (int)off, 0, 0);
                    } else {
                        raw_buffer_store_v4i32(i32x4{(int)o[0], (int)o[1], (int)o[2], (int)o[3]}, yr, (int)off, 0, 0);
                    }
                }
            }
        }
        n = nn;
        rt = nrt_;
        ct = nct_;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Column-ring variant of the identity block (CIN = 256) for LEF-shaped stage-1 maps (H = 19 rows, the whole height
// in one tile).  bottleneck_kernel<256> holds one 168-pixel window (86 KB) per tile and can only issue the next tile's
// window after phase R has consumed the current one, so every tile waits for its window (PMC r05a: 738 us per
// 625-pair chunk against a 415 us HBM floor).  Here consecutive 4-column tiles of a pair share their window columns
// through a ring of 12 input columns in LDS (3 groups of 4 columns x 19 rows x 512 B = 114 KB): tile c (output
// columns 4c .. 4c+3) reads groups G(c-1) = columns 4c-3 .. 4c and G(c) = 4c+1 .. 4c+4 (its window is 4c-1 .. 4c+4),
// and while it computes, the DMA fills G(c+1) into the slots of G(c-2), which tile c-1 finished with before this
// tile's first barrier.  Every input column is fetched once (no halo re-reads) and the fetch runs one whole tile
// ahead.  Wr (64 x 256) moves to registers (the ring takes its LDS); each output element is computed exactly as in
// bottleneck_kernel (same operands, k-step order, bias seeding, rounding), so the two are bit-identical.
//   phase R  T1 = relu(X . Wr + br) on the 6 x 19 window pixels (0 outside the image; T1 rows 0 and 20 = the 3x3's
//            zero padding rows, written once); wave (mh2, nq): window fragments 4 mh2 .. +3 x channels 16 nq ..
//   phase M  T2 = relu(conv3x3(T1) . Wm + bm), 76 output pixels in 5 fragments; wave (mh, nq): fragments {0,1,2} /
//            {3,4} x channels 16 nq ..
//   phase E  y = relu(T2 . We + be + x); wave w: channels 32 w .. +31, 5 fragments; residual from the ring.
constexpr int BR_H = 19, BR_TW = 4, BR_RC = 12;
constexpr int BR_GPX = BR_TW * BR_H;                // 76 pixels per column group
constexpr int BR_RING = BR_RC * BR_H * 512;         // 116736
constexpr int BR_T1 = BR_RING;                      // T1 [6 columns][21 rows] x 144 B
constexpr int BR_T2 = BR_T1 + 6 * 21 * BT_PITCH;    // + 18144: T2 [80 pixels] x 144 B
constexpr int BR_BIAS = BR_T2 + 80 * BT_PITCH;      // + 11520
constexpr int BR_LDS = BR_BIAS + (64 + 64 + 256) * 4;   // 147936
static_assert(BR_LDS <= 163840, "LDS budget");

template <bool Q8, bool PIPE = true, bool MERGE = false>
__global__ __launch_bounds__(512, 1) void bottleneck_ring_kernel(const bf16* __restrict__ x, void* __restrict__ y,
                                                                 const bf16* __restrict__ wr, const float* __restrict__ br,
                                                                 const bf16* __restrict__ wm, const float* __restrict__ bm,
                                                                 const bf16* __restrict__ we, const float* __restrict__ be,
                                                                 int N, int W, int nct, float q8_inv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Bs = (float*)(smem + BR_BIAS);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int hi = wid >> 2, nq = wid & 3;   // phases R / M: pixel group x channel quarter
    constexpr int YB = Q8 ? 1 : 2;
    const int ntiles = N * nct;
    const uint32_t x_bytes = (uint32_t)BR_H * W * 512, y_bytes = (uint32_t)BR_H * W * BT_COUT * YB;

    // ---- once per workgroup: biases -> LDS, T1's padding rows = 0, this wave's Wr / Wm / We slices -> registers
    if (tid < 64) Bs[tid] = br[tid];
    else if (tid < 128) Bs[tid] = bm[tid - 64];
    if (tid < 256) Bs[128 + tid] = be[tid];
    if (tid < 6 * 2 * 8) {   // T1 rows 0 and 20 of the 6 window columns, 8 x 16 B each
        const int col = tid >> 4, row = ((tid >> 3) & 1) * 20, ch = tid & 7;
        *(uint4*)(smem + BR_T1 + (col * 21 + row) * BT_PITCH + ch * 16) = make_uint4(0u, 0u, 0u, 0u);
    }
    bf16x8 wrf[8];           // Wr [64][256]: out ch 16 nq + fr, k-step s
#pragma unroll
    for (int s = 0; s < 8; ++s) wrf[s] = *(const bf16x8*)(wr + (nq * 16 + fr) * 256 + s * 32 + fq * 8);
    bf16x8 wmf[18];          // Wm [64][3][3][64]: out ch 16 nq + fr, k-step (tap, half)
#pragma unroll
    for (int s = 0; s < 18; ++s) wmf[s] = *(const bf16x8*)(wm + (nq * 16 + fr) * 576 + s * 32 + fq * 8);
    // We [256][64]: MFMA row fr of channel tile j = out ch 32 w + 8 (fr >> 2) + 4 j + (fr & 3), so a lane's two tiles
    // give it 8 consecutive channels (32 w + 8 fq ..) of its pixel: one 16-byte residual read and one 16-byte store
    // per fragment (8-byte stores left the store tail issue-bound)
    bf16x8 wef[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            wef[j][ks] = *(const bf16x8*)(we + (wid * 32 + 8 * (fr >> 2) + 4 * j + (fr & 3)) * 64 + ks * 32 + fq * 8);

    // ---- per-lane, tile-independent
    // DMA: instruction k of this wave fills group pixels q = 2 (w + 8 k) + lane / 32 (column q / 19, row q % 19),
    // LDS chunk position lane % 32; the source chunk is pre-swizzled by the ring pixel index (tile-dependent part)
    int dq[5], doff[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int q = 2 * (wid + 8 * k) + (lane >> 5);
        dq[k] = q;
        doff[k] = ((q % BR_H) * W + q / BR_H) * 512;
    }
    // phase R: window pixel p = 16 f + fr (column p / 19 -> 4c - 1 + col, row p % 19), f = 4 hi + i
    int rp_col[4], rp_row[4], t1w[4];
    bool rp_ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = (4 * hi + i) * 16 + fr;
        rp_ok[i] = p < 6 * BR_H;
        const int pp = rp_ok[i] ? p : 0;
        rp_col[i] = pp / BR_H;
        rp_row[i] = pp % BR_H;
        t1w[i] = BR_T1 + (rp_col[i] * 21 + rp_row[i] + 1) * BT_PITCH + (nq * 16 + fq * 4) * 2;
    }
    // phase M: output pixel o = 16 f + fr (column o / 19, row o % 19); its T1 (0, 0) tap = T1[col][row]
    int pb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int o = min((3 * hi + i) * 16 + fr, BR_GPX - 1);   // hi = 1: fragments 3, 4 (i = 2 unused)
        pb[i] = BR_T1 + ((o / BR_H) * 21 + o % BR_H) * BT_PITCH + fq * 16;
    }
    const int t2w = BR_T2 + (3 * hi * 16 + fr) * BT_PITCH + (nq * 16 + fq * 4) * 2;
    const int t2r = BR_T2 + fr * BT_PITCH + fq * 16;
    // phase E: output pixel o = 16 f + fr -> y offset in the pair (+ the tile's column), residual ring pixel
    int eo_col[5], eo_row[5];
    uint32_t so[5];
#pragma unroll
    for (int f = 0; f < 5; ++f) {
        const int o = f * 16 + fr;
        const int oo = o < BR_GPX ? o : 0;
        eo_col[f] = oo / BR_H;
        eo_row[f] = oo % BR_H;
        so[f] = o < BR_GPX ? (uint32_t)((eo_row[f] * W + eo_col[f]) * BT_COUT + wid * 32 + fq * 8) * YB : BT_OOB;
    }

    const int per = (ntiles + gridDim.x - 1) / gridDim.x;
    const int t0 = blockIdx.x * per, t1 = min(ntiles, t0 + per);
    if (t0 >= t1) return;

    // group m of pair n -> ring group slot gs = (m + 1) mod 3 (columns 4m + 1 .. 4m + 4 at ring slots 4 gs ..)
    auto issue_group = [&](int n, int m) {
        const int gs = ((m + 1) % 3 + 3) % 3;
        const i32x4 xr = buffer_rsrc(x + (int64_t)n * BR_H * W * 256, x_bytes);
        const int coff = (4 * m + 1) * 512;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int i = wid + 8 * k;
            if (i >= BR_GPX / 2) break;   // wave-uniform
            const int P = gs * BR_GPX + dq[k];
            const int src = doff[k] + coff + (((lane & 31) ^ (P & 15)) << 4);
            raw_buffer_load_lds(xr, (__attribute__((address_space(3))) void*)(smem + (gs * BR_GPX + 2 * i) * 512), 16,
                                src, 0, 0, 0);
        }
    };

    // phases as functions of the tile (pair n, column tile c): R reads the ring window and writes T1, M reads T1 and
    // writes T2, E reads T2 and the ring's residual columns and stores y
    auto phase_r = [&](int c) {
        const int s0 = 4 * (c % 3) + 2;                         // ring slot of window column 0 (image column 4c - 1)
        // ---- phase R
        {
            f32x4 ar[4];
            const f32x4 brv = lds_at<f32x4>(smem, BR_BIAS + (nq * 16 + fq * 4) * 4);
            // chunk 4 s + fq of ring pixel P sits at position (4 s + fq) ^ (P & 15): the lane's two bits, then the
            // k-step's two low bits against P & 12, then the k-step's bit 2 (an immediate 256 B)
            int xb[4], p12[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int sl = s0 + rp_col[i];
                sl = sl >= BR_RC ? sl - BR_RC : sl;
                const int P = sl * BR_H + rp_row[i];
                xb[i] = P * 512 + ((fq ^ (P & 3)) << 4);
                p12[i] = P & 12;
            }
            // software-pipelined: k-step s + 1's four fragments are requested before k-step s's MFMAs (the compiler had
            // each MFMA wait for its own just-issued read, lgkmcnt(0) x 32 per tile)
            if constexpr (PIPE) {
            bf16x8 rb[2][4];
            auto rload = [&](int s, bf16x8 (&dst)[4]) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    dst[i] = lds_at<bf16x8>(smem, xb[i] + ((((4 * s) & 12) ^ p12[i]) << 4) + (s >> 2) * 256);
            };
            rload(0, rb[0]);
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                __builtin_amdgcn_sched_barrier(0);
                if (s + 1 < 8) rload(s + 1, rb[(s + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    ar[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wrf[s], rb[s & 1][i], s == 0 ? brv : ar[i], 0, 0, 0);
            }
            } else {
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int a = xb[i] + ((((4 * s) & 12) ^ p12[i]) << 4) + (s >> 2) * 256;
                    const bf16x8 av = lds_at<bf16x8>(smem, a);
                    ar[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wrf[s], av, s == 0 ? brv : ar[i], 0, 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!rp_ok[i]) continue;
                const int col = 4 * c - 1 + rp_col[i];
                const f32x4 v = ar[i];
                u32x2 o = {relu_pk(v[0], v[1]), relu_pk(v[2], v[3])};
                if ((unsigned)col >= (unsigned)W) o = u32x2{0u, 0u};
                *(u32x2*)(smem + t1w[i]) = o;
            }
        }
    };
    auto phase_m = [&]() {
        // ---- phase M
        {
            const f32x4 bmv = lds_at<f32x4>(smem, BR_BIAS + (64 + nq * 16 + fq * 4) * 4);
            f32x4 am[3];
            const int nf = hi == 0 ? 3 : 2;
            // software-pipelined like phase R: k-step (tap, half) ks + 1's fragments requested before ks's MFMAs
            if constexpr (PIPE) {
            bf16x8 mb[2][3];
            auto mload = [&](int ks, bf16x8 (&dst)[3]) {
                const int tap = ks >> 1, hh = ks & 1;
                const int toff = ((tap % 3) * 21 + tap / 3) * BT_PITCH;   // (dh, dw) = (tap / 3, tap % 3)
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (i < nf) dst[i] = lds_at<bf16x8>(smem, pb[i] + toff + hh * 64);
            };
            mload(0, mb[0]);
#pragma unroll
            for (int ks = 0; ks < 18; ++ks) {
                __builtin_amdgcn_sched_barrier(0);
                if (ks + 1 < 18) mload(ks + 1, mb[(ks + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (i >= nf) break;
                    am[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wmf[ks], mb[ks & 1][i], ks == 0 ? bmv : am[i], 0, 0, 0);
                }
            }
            } else {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int toff = ((tap % 3) * 21 + tap / 3) * BT_PITCH;   // (dh, dw) = (tap / 3, tap % 3)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        if (i >= nf) break;
                        const bf16x8 av = lds_at<bf16x8>(smem, pb[i] + toff + hh * 64);
                        am[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wmf[tap * 2 + hh], av,
                                                                        tap == 0 && hh == 0 ? bmv : am[i], 0, 0, 0);
                    }
            }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                if (i >= nf) break;
                *(u32x2*)(smem + t2w + i * BT_FRAG) = u32x2{relu_pk(am[i][0], am[i][1]), relu_pk(am[i][2], am[i][3])};
            }
        }
    };
    auto phase_e = [&](int n, int c) {
        const int s0 = 4 * (c % 3) + 2;
        // ---- phase E
        {
            const i32x4 yr = buffer_rsrc((const char*)y + (int64_t)n * BR_H * W * BT_COUT * YB, y_bytes);
            const uint32_t tso = (uint32_t)(4 * c * BT_COUT * YB);
            const f32x4 bev[2] = {lds_at<f32x4>(smem, BR_BIAS + (128 + wid * 32 + fq * 8) * 4),
                                  lds_at<f32x4>(smem, BR_BIAS + (128 + wid * 32 + fq * 8 + 4) * 4)};
            f32x4 ae[5][2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int f = 0; f < 5; ++f) {
                    const bf16x8 av = lds_at<bf16x8>(smem, t2r + f * BT_FRAG + ks * 64);
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        ae[f][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wef[j][ks], av, ks == 0 ? bev[j] : ae[f][j], 0, 0, 0);
                }
#pragma unroll
            for (int f = 0; f < 5; ++f) {
                int sl = s0 + 1 + eo_col[f];
                sl = sl >= BR_RC ? sl - BR_RC : sl;
                const int P = sl * BR_H + eo_row[f];
                const int ra = P * 512 + (((wid * 4 + fq) ^ (P & 15)) << 4);
                const u32x4 rv = lds_at<u32x4>(smem, ra);   // channels 32 w + 8 fq .. + 7
                uint32_t off = so[f] + tso;
                if (4 * c + eo_col[f] >= W) off = BT_OOB;
                uint32_t o[4];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    f32x4 v = ae[f][j];
                    v[0] += bf_lo(rv[2 * j]);
                    v[1] += bf_hi(rv[2 * j]);
                    v[2] += bf_lo(rv[2 * j + 1]);
                    v[3] += bf_hi(rv[2 * j + 1]);
                    o[2 * j] = relu_pk(v[0], v[1]);
                    o[2 * j + 1] = relu_pk(v[2], v[3]);
                }
                if constexpr (Q8) {
                    int pk[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float q0 = fminf(fmaxf(bf_lo(o[2 * h]) * q8_inv, -448.f), 448.f);
                        const float q1 = fminf(fmaxf(bf_hi(o[2 * h]) * q8_inv, -448.f), 448.f);
                        const float q2 = fminf(fmaxf(bf_lo(o[2 * h + 1]) * q8_inv, -448.f), 448.f);
                        const float q3 = fminf(fmaxf(bf_hi(o[2 * h + 1]) * q8_inv, -448.f), 448.f);
                        pk[h] = __builtin_amdgcn_cvt_pk_fp8_f32(q0, q1, 0, false);
                        pk[h] = __builtin_amdgcn_cvt_pk_fp8_f32(q2, q3, pk[h], true);
                    }
                    raw_buffer_store_v2i32(i32x2{pk[0], pk[1]}, yr, (int)off, 0, 0);
                } else {
                    raw_buffer_store_v4i32(i32x4{(int)o[0], (int)o[1], (int)o[2], (int)o[3]}, yr, (int)off, 0, 0);
                }
            }
        }
    };

    int prev_n = -1;
    if constexpr (!MERGE) {
        for (int t = t0; t < t1; ++t) {
            const int n = t / nct, c = t - n * nct;
            const bool cold = t == t0 || n != prev_n;
            if (cold) {   // first tile of a pair (or of this workgroup's range): G(c-1), G(c) now, exposed
                __builtin_amdgcn_s_barrier();    // every wave is done with the ring (previous pair's last tile)
                issue_group(n, c - 1);
                issue_group(n, c);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(5)" ::: "memory");    // G(c) landed; the previous tile's 5 stores may fly
            }
            __builtin_amdgcn_s_barrier();
            prev_n = n;
            if (c + 1 < nct && t + 1 < t1) issue_group(n, c + 1);   // into G(c-2)'s slots, a whole tile ahead
            phase_r(c);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            phase_m();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            phase_e(n, c);
        }
    } else {
        // MERGE: tile c - 1's phase E and tile c's phase R share one barrier interval (E reads T2 and the ring's
        // residual columns, R reads the ring window and writes T1: disjoint), two barriers per tile instead of three.
        // G(c + 1) is issued after that interval (it overwrites G(c - 2), whose column 4c - 4 E(c - 1) reads) and each
        // wave retires it at the end of phase M(c), before the barrier that makes it visible to R(c + 1).
        bool pend = false;
        int pn = 0, pc = 0;
        for (int t = t0; t < t1; ++t) {
            const int n = t / nct, c = t - n * nct;
            const bool cold = t == t0 || n != prev_n;
            if (cold) {
                if (pend) {   // the previous pair's last tile finishes before the ring is reloaded
                    phase_e(pn, pc);
                    pend = false;
                }
                __builtin_amdgcn_s_barrier();
                issue_group(n, c - 1);
                issue_group(n, c);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }
            if (pend) phase_e(pn, pc);
            phase_r(c);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            prev_n = n;
            if (c + 1 < nct && t + 1 < t1) issue_group(n, c + 1);
            phase_m();
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            pend = true;
            pn = n;
            pc = c;
        }
        if (pend) phase_e(pn, pc);
    }
}

int num_cus_bt() {   // the persistent grid; CBW_BT_CUS=N (A/B) sizes it for N CUs, leaving the rest to the other streams
    static const int cap = [] {
        const char* e = getenv("CBW_BT_CUS");
        return e && atoi(e) > 0 ? atoi(e) : INT_MAX;
    }();
    return std::min(cbw_num_cus(), cap);
}

template <int CIN, bool Q8 = false>
hipError_t launch_bottleneck(const uint16_t* x, void* y, const uint16_t* wr, const float* br, const uint16_t* wm,
                             const float* bm, const uint16_t* we, const float* be, int N, int H, int W, hipStream_t st,
                             float q8_inv = 1.f) {
    if (N <= 0 || H <= 0 || W <= 0) return hipSuccess;
    const int nrt = (H + BT_TH - 1) / BT_TH, nct = (W + BT_TW - 1) / BT_TW;
    const int64_t nt = (int64_t)N * nrt * nct;
    // 32-bit buffer offsets: every in-range offset (plus a tile's reach) stays below BT_OOB
    if (nt >= (1LL << 31) || (int64_t)H * W * BT_COUT * 2 >= (int64_t)(BT_OOB >> 1)) return hipErrorInvalidValue;
    const int G = (int)std::min<int64_t>(nt, num_cus_bt());
    const char* me = getenv("CBW_BT64_MERGE");   // default: the first block's merged E / R schedule; 0 = three barriers
    if (CIN == 64 && !(me && atoi(me) == 0))
        hipLaunchKernelGGL((bottleneck_kernel<CIN, Q8, true>), dim3(G), dim3(512), BtL<CIN>::LDS, st, (const bf16*)x, y,
                           (const bf16*)wr, br, (const bf16*)wm, bm, (const bf16*)we, be, N, H, W, nrt, nct, q8_inv);
    else
        hipLaunchKernelGGL((bottleneck_kernel<CIN, Q8>), dim3(G), dim3(512), BtL<CIN>::LDS, st, (const bf16*)x, y,
                           (const bf16*)wr, br, (const bf16*)wm, bm, (const bf16*)we, be, N, H, W, nrt, nct, q8_inv);
    return hipGetLastError();
}

// the column-ring identity block (LEF-shaped maps, H = 19); CBW_BT_RING=0 keeps bottleneck_kernel<256>
bool bt_ring_enabled() {
    const char* e = getenv("CBW_BT_RING");
    return !(e && atoi(e) == 0);
}

template <bool Q8>
hipError_t launch_bottleneck_ring(const uint16_t* x, void* y, const uint16_t* wr, const float* br, const uint16_t* wm,
                                  const float* bm, const uint16_t* we, const float* be, int N, int W, hipStream_t st,
                                  float q8_inv) {
    const int nct = (W + BR_TW - 1) / BR_TW;
    const int64_t nt = (int64_t)N * nct;
    if (nt >= (1LL << 31) || (int64_t)BR_H * W * BT_COUT * 2 >= (int64_t)(BT_OOB >> 1)) return hipErrorInvalidValue;
    const int G = (int)std::min<int64_t>(nt, num_cus_bt());
    const char* pe = getenv("CBW_BT_PIPE");   // 0: phases R / M without the read pipelining (A/B, bit-identical)
    const char* me = getenv("CBW_BT_MERGE");  // default: phase E of a tile and phase R of the next in one barrier interval
    if (!(me && atoi(me) == 0) && !(pe && atoi(pe) == 0))
        hipLaunchKernelGGL((bottleneck_ring_kernel<Q8, true, true>), dim3(G), dim3(512), BR_LDS, st, (const bf16*)x, y,
                           (const bf16*)wr, br, (const bf16*)wm, bm, (const bf16*)we, be, N, W, nct, q8_inv);
    else if (pe && atoi(pe) == 0)
        hipLaunchKernelGGL((bottleneck_ring_kernel<Q8, false>), dim3(G), dim3(512), BR_LDS, st, (const bf16*)x, y,
                           (const bf16*)wr, br, (const bf16*)wm, bm, (const bf16*)we, be, N, W, nct, q8_inv);
    else
        hipLaunchKernelGGL((bottleneck_ring_kernel<Q8, true>), dim3(G), dim3(512), BR_LDS, st, (const bf16*)x, y,
                           (const bf16*)wr, br, (const bf16*)wm, bm, (const bf16*)we, be, N, W, nct, q8_inv);
    return hipGetLastError();
}

}  // namespace

hipError_t cbw_bottleneck_s1(const uint16_t* x, uint16_t* y, const uint16_t* wr, const float* br, const uint16_t* wm,
                             const float* bm, const uint16_t* we, const float* be, const void* zero, int N, int H,
                             int W, hipStream_t st) {
    (void)zero;   // (round 1: the source of zero-filled halo rows; the window DMA no longer needs one)
    if (N <= 0 || W <= 0) return hipSuccess;
    if (H == BR_H && bt_ring_enabled()) return launch_bottleneck_ring<false>(x, y, wr, br, wm, bm, we, be, N, W, st, 1.f);
    return launch_bottleneck<256>(x, y, wr, br, wm, bm, we, be, N, H, W, st);
}

hipError_t cbw_bottleneck_s1_q8(const uint16_t* x, uint8_t* y, const uint16_t* wr, const float* br, const uint16_t* wm,
                                const float* bm, const uint16_t* we, const float* be, float inv_scale, int N, int H,
                                int W, hipStream_t st) {
    if (N <= 0 || W <= 0) return hipSuccess;
    if (H == BR_H && bt_ring_enabled())
        return launch_bottleneck_ring<true>(x, y, wr, br, wm, bm, we, be, N, W, st, inv_scale);
    return launch_bottleneck<256, true>(x, y, wr, br, wm, bm, we, be, N, H, W, st, inv_scale);
}

hipError_t cbw_bottleneck_s1_first(const uint16_t* x, uint16_t* y, const uint16_t* wr, const float* br,
                                   const uint16_t* wm, const float* bm, const uint16_t* wcat, const float* bcat,
                                   const void* zero, int N, int H, int W, hipStream_t st) {
    (void)zero;
    return launch_bottleneck<64>(x, y, wr, br, wm, bm, wcat, bcat, N, H, W, st);
}
