// Internal launcher declarations (host side) for the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <string>

#include "conv_args.h"

typedef __bf16 bf16;
struct ConvRoute;   // conv_route.h

// compute units of the current device (cached per device; 256 if the query fails): every grid and fill rule sizes by it
int cbw_num_cus();

// the bf16 family's dispatch: launches the route conv_route.h gives for (a, cbw_num_cus(), the CBW_* knobs read now)
hipError_t cbw_conv_igemm(const ConvArgs& a, hipStream_t st);
// the kernel (rocprofv3's short name, template arguments included) the last conv dispatch on this host thread
// launched: ConvRoute::name for the bf16 family, a per-instantiation static for the fp8 one, so the runtime's profile
// records keep the pointer.  Every dispatch that returns hipSuccess has set it.
extern thread_local const char* cbw_last_conv_kernel;
// the CUs cbw_conv_stream sizes its persistent grid for (0: all): set by the KWS runtime while keyword chunks run on
// several streams, so the HBM-bound streaming convs leave CUs to the other streams' MFMA-bound convs
extern thread_local int cbw_cs_grid_cus;
inline std::string kernel_name(const char* base, std::initializer_list<int> targs) {   // "base<a, b, c>"
    std::string s = std::string(base) + "<";
    bool first = true;
    for (int t : targs) {
        s += (first ? "" : ", ") + std::to_string(t);
        first = false;
    }
    return s + ">";
}
// split-K for few-tile GEMMs (the Whisper encoder's out-projection and fc2 at M = 1500): the K-split factor
// that fills the GPU (1 = no split), and the split launch + a deterministic fixed-order reduction with the
// epilogue (bias, residual, activation, output type); partial holds ksplit * M * Cout floats.
int cbw_conv_splitk_factor(const ConvArgs& a);
hipError_t cbw_conv_igemm_splitk(const ConvArgs& a, int ksplit, float* partial, hipStream_t st);
// skinny GEMM for M <= 16 rows (gemv.hip): y = act(x . W^T + bias (+ res)); x [M][ldx], W [N][K] bf16;
// one workgroup per 16 output columns, K split over its waves and reduced in LDS (deterministic)
struct GemvArgs {
    const bf16* x;
    int ldx;
    const bf16* w;
    const float* bias;
    const void* res;
    int res_ld;
    void* y;
    int ldy;
    int M, N, K, flags;
    // LayerNorm prologue (optional): x = LN(xf) over K with ln_g / ln_b (eps ln_eps), xf f32 rows of
    // stride ldx, computed exactly as layernorm_kernel does; x is then ignored
    const float* xf;
    const float* ln_g;
    const float* ln_b;
    float ln_eps;
    // K/V cache append (optional): output columns [kv_D, 2 kv_D) also go to kv_k + m kv_ld + (n - kv_D),
    // [2 kv_D, 3 kv_D) to kv_v (the decode step's fused qkv projection)
    bf16* kv_k;
    bf16* kv_v;
    int64_t kv_ld;
    int kv_D;
    const int* kv_pos;   // optional: the append position read on the device (kv_k/kv_v then point at position 0)
    int kv_pos_rows;     // with kv_pos: 1 = one position per row (kv_pos[m], a step over several windows)
    int wide_gx;         // cbw_gemv_wide only (it sets this): 1 = the row groups are grid x, 0 = grid y
};
int cbw_gemv_waves(int K);
bool cbw_gemv_ln_ok(int M, int K);   // whether the LayerNorm prologue applies to this shape
hipError_t cbw_gemv(const GemvArgs& a, hipStream_t st);
// the same Linear over 1 <= M <= CBW_DEC_WIDE_ROWS (80) rows: ceil(M / 16) row groups in one launch, each the
// 16-slot kernel of cbw_gemv's family on its rows, so a row carries the bits cbw_gemv gives it on its 16-row slice
// (gemv_wide_route, gemv_route.h).  groups_fast: the groups are the fast grid coordinate, else the column blocks.
hipError_t cbw_gemv_wide(const GemvArgs& a, hipStream_t st, bool groups_fast);

// fp8 (OCP e4m3) implicit-GEMM conv (conv_fp8.hip): the first tier of the exact-decision cascade.  x / res / y
// e4m3 NHWC with one static scale per tensor (folded into the weights / res_scale / y_inv_scale); w e4m3
// [Cout][KH][KW][Cin] quantized per output channel; y = act(acc * alpha + bias (+ res * res_scale)) as e4m3
// (value * y_inv_scale, saturated) or bf16 (out_bf16).  1x1 / 3x3, Cin % 128 == 0, Cout % 128 == 0.
struct F8ConvArgs {
    const uint8_t* x;
    const uint8_t* w;
    const float* alpha;
    const float* bias;
    const uint8_t* res;
    float res_scale;
    void* y;
    float y_inv_scale;
    int out_bf16;
    const void* zero;
    int N, H, W, Cin, Ho, Wo, Cout, KH, KW, sh, sw, ph, pw, M;
    int relu;
};
bool cbw_conv_fp8_supported(const F8ConvArgs& a);
// the fp8 streaming 1x1 kernel (conv_fp8_stream.hip): stride 1, Cin in {128, 256, 512}; cbw_conv_fp8 routes to it
bool cbw_conv_fp8_stream_supported(const F8ConvArgs& a);
hipError_t cbw_conv_fp8_stream(const F8ConvArgs& a, hipStream_t st);
hipError_t cbw_conv_fp8(const F8ConvArgs& a, hipStream_t st);
hipError_t cbw_quant_fp8(const uint16_t* x, uint8_t* y, int64_t n, float inv_scale, hipStream_t st);   // bf16 -> e4m3
int cbw_absmax_groups();
hipError_t cbw_absmax_f32(const float* x, int64_t n, float* part, hipStream_t st);   // part[cbw_absmax_groups()]
hipError_t cbw_mfma_fp8_probe(const uint8_t* A, const uint8_t* Bt, float* C, int mode, hipStream_t st);
hipError_t cbw_cvt_fp8_probe(const float* x, uint8_t* q, float* back, int n, hipStream_t st);

// persistent 8-wave ring kernel (conv_ring.hip): Cout % 128 == 0, Cin % 64 == 0, 1x1 / 3x3, bf16
// residual/output, ReLU or none; hipErrorNotSupported otherwise
bool cbw_conv_ring_supported(const ConvArgs& a);
hipError_t cbw_conv_ring(const ConvArgs& a, hipStream_t st);
hipError_t cbw_conv_ring(const ConvArgs& a, const ConvRoute& r, hipStream_t st);   // r: conv_ring_route's / conv_route's
// row-stationary streaming 1x1 kernel (conv_stream.hip): stride-1 1x1, K = Cin (+ Cin2) in {128, 256, 384, 512}
// (K 512 on 16-pixel units; CBW_CS_K512=0 sends K 512 back to the tile kernels), weights stationary in LDS,
// rows in registers; for the HBM-bound expand convs and the K 256 / 512 reduces
bool cbw_conv_stream_supported(const ConvArgs& a);
hipError_t cbw_conv_stream(const ConvArgs& a, hipStream_t st);
hipError_t cbw_conv_stream(const ConvArgs& a, const ConvRoute& r, hipStream_t st);   // r: conv_stream_route's / conv_route's
// the stage-2 identity junction in one launch (conv_stream.hip): a = the expand 128 -> 512 with its bf16 residual and
// ReLU (y as cbw_conv_stream writes it), and t1 [M][128] = relu(y . wr^T + br), the next block's 1x1 reduce,
// bit-identical to the two launches.  wr_packed: the reduce weights [128][512] in the kernel's fragment order
// (cbw_conv_chain_pack, 128 KB).  red_cout: the reduce's output channels (128).  CBW_CS_CHAIN=0 disables the chain
// per call; the grid obeys cbw_cs_grid_cus like cbw_conv_stream
bool cbw_conv_chain_supported(const ConvArgs& a, int red_cout);
hipError_t cbw_conv_chain_pack(const uint16_t* wr, uint16_t* packed, hipStream_t st);
hipError_t cbw_conv_chain(const ConvArgs& a, const uint16_t* wr_packed, const float* br, void* t1, hipStream_t st);

// fused ResNet-50 stage-1 identity bottleneck (bottleneck.hip): x, y NHWC bf16 [N][H][W][256];
// wr [64][256], wm [64][3][3][64], we [256][64] bf16 (BN folded), biases f32
hipError_t cbw_bottleneck_s1(const uint16_t* x, uint16_t* y, const uint16_t* wr, const float* br, const uint16_t* wm,
                             const float* bm, const uint16_t* we, const float* be, const void* zero, int N, int H,
                             int W, hipStream_t st);
// the same block with its output quantized for the fp8 tier: y e4m3 [N][H][W][256] = e4m3(bf16 block output *
// inv_scale) (cbw_quant_fp8's arithmetic)
hipError_t cbw_bottleneck_s1_q8(const uint16_t* x, uint8_t* y, const uint16_t* wr, const float* br, const uint16_t* wm,
                                const float* bm, const uint16_t* we, const float* be, float inv_scale, int N, int H,
                                int W, hipStream_t st);
// the stage's first block: x [N][H][W][64]; wr [64][64], wm [64][3][3][64], wcat [256][64 + 64] = [W_expand |
// W_shortcut] (BN folded), bcat = b_expand + b_shortcut (load_fused_expand_shortcut)
hipError_t cbw_bottleneck_s1_first(const uint16_t* x, uint16_t* y, const uint16_t* wr, const float* br,
                                   const uint16_t* wm, const float* bm, const uint16_t* wcat, const float* bcat,
                                   const void* zero, int N, int H, int W, hipStream_t st);

// ---- KWS path (kws_kernels.hip) ----
// f32 [B][L][T][D] -> bf16 [L][B][T][D] (layer-major so each layer's rows are contiguous)
hipError_t cbw_cast_permute_lbtd(const float* x, uint16_t* y, int B, int L, int T, int D, hipStream_t st);
// rows of E floats (fp32 or bf16 in) -> L2-normalised bf16 rows with clamp(norm, eps); optional output
// row permutation from [L][B][T] to [B][L][T]
hipError_t cbw_normalize_rows(const void* x, int x_is_f32, void* y, int y_is_f32, int L, int B, int T, int E,
                              float eps, int permute_lb, hipStream_t st);
hipError_t cbw_nchw_to_nhwc4(const float* x, uint16_t* y, int K, int L, int H, int W, hipStream_t st);
hipError_t cbw_l2norm_rows_f32(float* x, int64_t rows, int E, hipStream_t st);
// LEF time projector: conv1d(U->U,k3,p1) (BN folded) + MaxPool1d(3,2,1) + L2-normalise, fp32 math.
// x: f32 [L][B][T][U] (GEMM2 output), w: f32 [L][U][3][U] (o, k, i), b: f32 [L][U]
// y: bf16 [B][L][To][U];  mask_in f32 [B][L][T] -> mask_out f32 [B][L][To] (max-pooled)
hipError_t cbw_lef_time_project(const float* x, const float* w, const float* b, void* y, int y_is_f32,
                                const float* mask_in, float* mask_out,
                                int L, int B, int T, int U, float eps, hipStream_t st);
// masked cosine-similarity maps, NHWC [K][Tk][Tu][4] bf16 (channel l < L, rest zero), L <= 4.
// kwd: bf16 [K][L][Tk][E] normalised; utt: bf16 [L][Tu][E] normalised; masks f32.
hipError_t cbw_sim_maps(const uint16_t* kwd, const float* kwd_mask, const uint16_t* utt, const float* utt_mask,
                        uint16_t* out, int K, int L, int Tk, int Tu, int E, hipStream_t st);
// the same maps for a chunk of P (utterance, keyword) pairs, out [P][Tk][Tu][4]: utt bf16 [B][L][Tu][E],
// utt_mask f32 [B][L][Tu]; pair p = (pair_utt[p], pair_kwd[p]) (device int32 [P]), or with both null the
// global pair p0 + p = b * K + k.  Indices are clamped into [0, B) / [0, K) in the kernel.
hipError_t cbw_sim_maps_pairs(const uint16_t* kwd, const float* kwd_mask, int K, const uint16_t* utt,
                              const float* utt_mask, int B, const int32_t* pair_utt, const int32_t* pair_kwd, int p0,
                              uint16_t* out, int P, int L, int Tk, int Tu, int E, hipStream_t st);
// same maps as fp32 NCHW [K][L][Tk][Tu] (KWSOutput.features on request)
hipError_t cbw_sim_to_nchw(const uint16_t* maps, float* out, int K, int L, int Tk, int Tu, hipStream_t st);
// ResNet stem conv7x7 s2 p3 over NHWC4 input, BN folded, ReLU. w: bf16 [64][7][8][4] (kw padded to 8)
hipError_t cbw_stem_conv(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y,
                         int N, int H, int W, int Ho, int Wo, hipStream_t st);
// stem conv + BN + ReLU + MaxPool2d(3,2,1) in one kernel (no stem tensor in HBM); y: bf16 NHWC [N][Hp][Wp][64]
hipError_t cbw_stem_pool(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y, int N, int H, int W,
                         int Hs, int Ws, int Hp, int Wp, hipStream_t st);
// the same over NHWC16 input (12-layer maps of the original CB-Whisper CNN), w: bf16 [64][7][8][16]
hipError_t cbw_stem16_pool(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y, int N, int H,
                           int W, int Hs, int Ws, int Hp, int Wp, hipStream_t st);
// the compensated tier's stem: NHWC16 [hi | hi | lo | 0] input, [w_hi | w_lo | w_hi | 0] weights, fp32 stem tile and
// max-pool, output [N][Hp][Wp][128] bf16 = [hi | lo] of the pooled fp32 value
hipError_t cbw_stem16_pool_x3(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y, int N, int H,
                              int W, int Hs, int Ws, int Hp, int Wp, hipStream_t st);
hipError_t cbw_maps_split16(const float* x, uint16_t* y, int K, int L, int H, int W, hipStream_t st);
// bilinear (align_corners=False, no antialias) resize of per-keyword similarity matrices to NHWC16
// bf16 [K][Ho][Wo][16]: sim f32, layer l row r at sim + l*layer_stride + r*ld; keyword k rows
// [off[k0+k], off[k0+k+1]) relative to off[k0]
hipError_t cbw_sim_resize(const float* sim, int64_t layer_stride, int ld, const int* off_dev, int k0, int K, int L,
                          int Tu, int Ho, int Wo, uint16_t* out, hipStream_t st);
// the similarity rows of pairs [p0, p0 + pc) of a batch (pair p = b * K + k) for all L layers in one launch:
// utt bf16 [B][L][Tu][D], kwd bf16 [L][R][D] with keyword k on rows off[k] .. off[k+1]-1 (device int32 [K + 1]);
// rows f32 [L][chunk rows][ld], the chunk's keywords' frames in pair order, row t < Tk_k column u < Tu written.
// max_run_rows bounds the rows of one run (a keyword range of one utterance; R always does), rows_cap the chunk's
// rows: no row at or past it is written.  D % 64 == 0; bf16 MFMA, k placed as conv_igemm_kernel places it.
hipError_t cbw_sim_rows_bf16(const uint16_t* utt, const uint16_t* kwd, const int* off, int B, int K, int R, int L,
                             int Tu, int D, int p0, int pc, int max_run_rows, int64_t rows_cap, int ld, float* rows,
                             hipStream_t st);
// cbw_sim_resize over those rows: item i = pair p0 + i -> NHWC16 bf16 out [pc][Ho][Wo][16], in pair order
hipError_t cbw_sim_resize_batch(const float* rows, int ld, const int* off, int p0, int pc, int K, int R, int64_t rows_cap,
                                int L, int Tu, int Ho, int Wo, uint16_t* out, hipStream_t st);
hipError_t cbw_nchw_to_nhwc16(const float* x, uint16_t* y, int K, int L, int H, int W, hipStream_t st);
// MaxPool2d(3,2,1) NHWC bf16, C % 8 == 0
hipError_t cbw_maxpool3s2(const uint16_t* x, uint16_t* y, int N, int H, int W, int C, int Ho, int Wo, hipStream_t st);
// AdaptiveAvgPool(1) + Linear(C -> 2): logits f32 [N][2]
hipError_t cbw_pool_fc(const uint16_t* x, const float* w, const float* b, float* logits, int N, int HW, int C,
                       hipStream_t st);
// prob = softmax(logits)[:,1] * ghost; idx_out = sorted {i : prob >= thr}; n_out = count.  mode 1 = argmax rule,
// mode 2 = the near-threshold band {i : |prob - thr| <= band} (the pairs the fp32 re-scoring re-runs)
// 64-bit content checksum of a 16-byte aligned device byte range (kws_kernels.hip); scratch: cbw_checksum_scratch_bytes()
int cbw_checksum_scratch_bytes();
hipError_t cbw_checksum64(const void* data, int64_t bytes, uint64_t* out, uint64_t* scratch, hipStream_t st);
hipError_t cbw_spot(const float* logits, const float* ghost, int K, float thr, float band, int mode, float* prob_out,
                    int* idx_out, int* n_out, hipStream_t st);

// ---- fp32 re-scoring path (kws_exact.hip) ----
struct F32ConvArgs {
    const float* x;     // [N][H][W][Cin]
    const float* w;     // [Cout][KH][KW][Cin]
    const float* bias;  // [Cout] or null
    const float* res;   // [M][Cout] or null
    float* y;           // [M][Cout]
    int N, H, W, Cin, Ho, Wo, Cout, KH, KW, sh, sw, ph, pw, M, relu;
};
hipError_t cbw_conv_f32(const F32ConvArgs& a, hipStream_t st);   // Cout % 64 == 0
hipError_t cbw_sim_f32(const float* kwd, const float* kwd_mask, const float* utt, const float* utt_mask, const int* sel,
                       int p0, int P, float* out, int L, int Tk, int Tu, int E, hipStream_t st);
// the same maps for P pairs of a pair list: utt f32 [B][L][Tu][E], utt_mask f32 [B][L][Tu]; map p = pair
// sel[p0 + p] of the n_pairs pairs = (pair_utt[q], pair_kwd[q]) (device int32 [n_pairs]), or with both null
// q = b * K + k.  q, b and k are clamped into range in the kernel.
hipError_t cbw_sim_f32_pairs(const float* kwd, const float* kwd_mask, int K, const float* utt, const float* utt_mask,
                             int B, const int32_t* pair_utt, const int32_t* pair_kwd, int n_pairs, const int* sel, int p0,
                             int P, float* out, int L, int Tk, int Tu, int E, hipStream_t st);
// CB-Whisper's own spotter in fp32: utt f32 [B][L][Tu][D], kwd f32 [L][R][D] with keyword k on rows off[k] .. off[k+1]-1
// (device int32 [K + 1]); map p of the pass = keyword sel[p0 + p] (clamped into [0, K), its rows into [0, R) and
// its length to TkMax in the kernel).  rows f32 [P][L][TkMax][ld] (ld >= Tu): row t < Tk_k, column u < Tu written.
// D % 16 == 0; fp32-input MFMA, k ascending.  B = 1: one utterance, the kernels as they always ran; B > 1: sel indexes
// the B * K pairs s = b * K + k (clamped into range) and the _batch kernels resolve utterance s / K, keyword s % K.
hipError_t cbw_sim_rows_f32(const float* utt, int B, const float* kwd, const int* off, const int* sel, int p0, int P,
                            int K, int R, int L, int Tu, int D, int TkMax, int ld, float* rows, hipStream_t st);
// those rows resized bilinearly (cbw_sim_resize's arithmetic) to fp32 NHWC out [P][Ho][Wo][L]
hipError_t cbw_sim_resize_f32(const float* rows, int B, const int* off, const int* sel, int p0, int P, int K, int R,
                              int L, int Tu, int TkMax, int ld, int Ho, int Wo, float* out, hipStream_t st);
hipError_t cbw_maxpool_f32(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo, hipStream_t st);
hipError_t cbw_pool_fc_f32(const float* x, const float* w, const float* b, const int* sel, int p0, int P, float* logits,
                           int HW, int C, hipStream_t st);
hipError_t cbw_permute_lbtd_f32(const float* x, float* y, int B, int L, int T, int D, hipStream_t st);
// fp32 [M][C] -> bf16 [M][2C] = [hi | lo] (input of the 3-term split convs, CBW_EPI_SPLIT3)
hipError_t cbw_split3(const float* x, uint16_t* y, int64_t M, int C, hipStream_t st);
// part[g][c] += sum of x[r][c] over workgroup g's rows (g < cbw_channel_sum_groups()); bias-correction statistics
hipError_t cbw_channel_sum_f32(const float* x, int64_t M, int C, float* part, hipStream_t st);
int cbw_channel_sum_groups();

// ---- Whisper front end / encoder (whisper_kernels.hip) ----
constexpr int CBW_MEL_LONG_PARTS = 256;   // long-form: partial maxima in the scratch (>= 1 KB)
// frames <= 0 / L_pad <= 0: the 30 s window (3000 frames, zero padding to 480000 samples); else long-form
// features of the whole audio (L_pad = n_samples, frames = n_samples / 160)
hipError_t cbw_mel_frames(const float* pcm, int n_samples, const float* filters, const float* twiddle,
                          float* logmel, int n_mel, hipStream_t st, int L_pad = 0, int frames = 0);
hipError_t cbw_mel_finish(float* logmel, int n_mel, float* scratch, uint16_t* packed, int cpad, hipStream_t st,
                          int frames = 0);
// polyphase resampler with the downmix in its loads: pcm f32 [C][len] -> out f32 [out_len],
// out[f n + j] = sum_k mean_c(xpad)[f o + k] * tab[k n + j] (tab phase-minor: [T][n], T = 2 width + o; xpad = x behind
// `width` zeros, zero past its end too).  The table is staged in LDS where n * T <= CBW_RESAMPLE_LDS_FLOATS.
constexpr int CBW_RESAMPLE_LDS_FLOATS = 8192;   // 32 KB of the 160 KB LDS: several blocks still share a CU
hipError_t cbw_resample_taps(const float* pcm, int C, int64_t len, const float* tab, int o, int n, int width, int T,
                             float* out, int64_t out_len, hipStream_t st);
// out[i] = mean over the C rows of pcm [C][len]
hipError_t cbw_downmix(const float* pcm, int C, int64_t len, float* out, hipStream_t st);
hipError_t cbw_layernorm(const float* x, const float* g, const float* b, uint16_t* y, float* y32, int rows, int D,
                         float eps, hipStream_t st);
hipError_t cbw_attention(const uint16_t* qkv, uint16_t* out, int B, int T, int H, int hd, hipStream_t st);

// ---- Whisper decoder step (whisper_kernels.hip) ----
// pos_inc 0: every row at pos (decode step); 1: row r at pos + r (prefill of a prefix)
hipError_t cbw_dec_embed(const int* tok, const uint16_t* E, const float* P, int pos, float* h, int B, int D,
                         hipStream_t st, int pos_inc = 0, const int* pos_dev = nullptr, int pos_rows = 0);
hipError_t cbw_dec_kv_append(const uint16_t* qkv, uint16_t* kc, uint16_t* vc, int B, int D, int maxlen, int pos,
                             hipStream_t st);
// prefill: the k, v of T prefix tokens (fused qkv rows) -> positions 0..T-1 of all B cache rows
hipError_t cbw_dec_kv_prefill(const uint16_t* qkv, uint16_t* kc, uint16_t* vc, int T, int B, int D, int maxlen,
                              hipStream_t st);
// causal 1 (prefill): query row r sees keys 0..r
hipError_t cbw_dec_attention(const uint16_t* q, int ldq, const uint16_t* kc, const uint16_t* vc, int64_t kv_bstride,
                             int n_keys, int rows_per_kv, uint16_t* out, int B, int H, int D, hipStream_t st,
                             int causal = 0);
// cross-attention probabilities of head `head` for T query rows (q row pitch ldq, pre-scaled) against n_keys cross
// keys (row pitch D): out f32 [T][n_keys] (token-level timestamps)
hipError_t cbw_dec_cross_probs(const uint16_t* q, int ldq, const uint16_t* kc, int n_keys, int T, int D, int head,
                               float* out, hipStream_t st);
// token-level timestamps behind the probabilities.  align_matrix: probs f32 [n][T_all][1500] (cbw_dec_cross_probs'
// layout), positions [t0, t0 + T), the first F frames, odd width <= 7 -> matrix f32 [T][F], the negated head mean of
// the median-filtered normalised weights; *degenerate (zeroed by the caller) |= 1 on a zero / non-finite variance.
// dtw: matrix f32 [T][F], T <= 1024 -> first_frame int32 [T] and, where text_idx is given, the path as cbw_dtw writes
// it; trace: cbw_dtw_trace_words(T, F) words of scratch.
constexpr int CBW_DTW_MAX_F = 1500;   // the encoder frames of a window
int64_t cbw_dtw_trace_words(int T, int F);
hipError_t cbw_align_matrix_launch(const float* probs, int n, int T_all, int t0, int T, int F, int width,
                                   float* matrix, int* degenerate, hipStream_t st);
hipError_t cbw_dtw_launch(const float* matrix, int T, int F, int* first_frame, int* text_idx, int* time_idx, int* len,
                          uint32_t* trace, hipStream_t st);
// the same two for N <= CBW_TS_MAX_WINDOWS windows in one launch each: the windows' table goes to the kernel by value
// (no upload); window i's arithmetic is that of the single-window launch.  degenerate int32 [N] (zeroed by the
// caller), first_frame int32 [N][ld], ld >= the largest T; no path.
constexpr int CBW_TS_MAX_WINDOWS = 16;   // CBW_TOKEN_TS_MAX_WINDOWS (cbw.h)
struct cbw_ts_win {
    const float* probs;   // [n][T_all][1500]
    float* matrix;        // [T][F]
    uint32_t* trace;      // cbw_dtw_trace_words(T, F) words
    int T_all, t0, T, F;
};
struct cbw_ts_batch {
    cbw_ts_win w[CBW_TS_MAX_WINDOWS];
};
hipError_t cbw_align_matrix_batch_launch(const cbw_ts_batch& b, int N, int n, int width, int* degenerate,
                                         hipStream_t st);
hipError_t cbw_dtw_batch_launch(const cbw_ts_batch& b, int N, int* first_frame, int ld, hipStream_t st);
hipError_t cbw_dec_reorder_kv(uint16_t* ks, uint16_t* vs, const int* rows, int B, int n_layers, int64_t layer_elems,
                              int64_t row_elems, int64_t copy_elems, hipStream_t st);
// decode-step self-attention in one launch: row r (its own K/V batch r) over min(n_keys, n_keys_pos[nk_rows ? r : 0]
// + 1) keys when n_keys_pos is given, else n_keys; n_keys <= 448
hipError_t cbw_dec_self_attn(const uint16_t* q, int ldq, const uint16_t* kc, const uint16_t* vc, int64_t kv_bstride,
                             int n_keys, uint16_t* out, int B, int H, int D, hipStream_t st, const int* n_keys_pos,
                             int nk_rows);
// split-key decode attention; part = cbw_dec_attn_split_floats(B, H) floats of scratch
int cbw_dec_attn_split_floats(int B, int H);
// n_keys_pos (optional): the key count is *n_keys_pos + 1, read on the device; n_keys then bounds it (the grid
// covers ceil(n_keys / 64) chunks; chunks past the live count contribute nothing) -- graph-replayable steps
hipError_t cbw_dec_attn_split(const uint16_t* q, int ldq, const uint16_t* kc, const uint16_t* vc, int64_t kv_bstride,
                              int n_keys, int rows_per_kv, uint16_t* out, int B, int H, int D, float* part,
                              hipStream_t st, const int* n_keys_pos = nullptr, int nk_rows = 0);
hipError_t cbw_dec_gather_rows(const uint16_t* src, uint16_t* dst, const int* rows, int B, int64_t row_elems,
                               int64_t copy_elems, hipStream_t st);

// ---- Token choice from a row of logits (token_select.hip) ----
hipError_t cbw_beam_select_launch(const float* lp, const int* idx, int B, int k, int eos, double* beam_scores,
                                  double* cand_score, int* cand_row, int* cand_tok, int* tokens, int* parents, int* ok,
                                  int* ts_state, int* st_out, int ts_begin, int count, hipStream_t st);
hipError_t cbw_greedy_select_launch(const float* logits, int B, int V, int ld, const float* bias,
                                    const float* bias_begin, int ts_begin, int no_ts, int eos, int max_initial,
                                    int* ts_state, const int* pos_rows, const int* limit, int* active, int* tokens,
                                    float* logprob, hipStream_t st);
// cbw_greedy_select_launch's arguments, then the warpers and the race's noise f32 [B][noise_ld] (noise_ld >= V);
// V <= CBW_SAMPLE_MAX_V: a block of 1024 threads holds its row's scores in 51 registers per thread
constexpr int CBW_SAMPLE_MAX_V = 1024 * 51;
hipError_t cbw_sample_select_launch(const float* logits, int B, int V, int ld, const float* bias,
                                    const float* bias_begin, int ts_begin, int no_ts, int eos, int max_initial,
                                    int* ts_state, const int* pos_rows, const int* limit, int* active, int* tokens,
                                    float* logprob, float temperature, int top_k, const float* noise,
                                    int64_t noise_ld, hipStream_t st);
// the repetition penalty and the no-repeat n-gram bans on up to 16 rows' logits in place, from a per-row token history
// the kernel keeps itself (hist int32 [B][hist_ld], hist_len [B]); hist_ld <= CBW_HISTORY_MAX_LD: a block stages its
// row's history in LDS
constexpr int CBW_HISTORY_MAX_LD = 2048;
hipError_t cbw_history_rules_launch(float* logits, int B, int V, int ld, int* hist, int hist_ld, int* hist_len,
                                    const int* last_tokens, const int* pos_rows, const int* active,
                                    float repetition_penalty, int no_repeat_ngram_size, hipStream_t st);
hipError_t cbw_logprob_topk_launch(const float* logits, int B, int V, int ld, const float* bias, int64_t bias_ld,
                                   int k, float* lp, int* idx, hipStream_t st);
hipError_t cbw_timestamp_rules_launch(const float* logits, int B, int V, int ld, const float* bias, const int* state,
                                      int ts_begin, int no_ts, int eos, int max_initial, float* bias_out,
                                      hipStream_t st);
