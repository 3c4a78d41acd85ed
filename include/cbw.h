/*
 * cbw.h — C ABI of libcbw.so, the MI355X (gfx950) CB-Whisper hot path.
 *
 * The reference (Priberam/Enhance-CB-Whisper) is pure Python/PyTorch and has
 * no FFI; each entry point below replaces the reference call it names
 * (paths relative to the reference src/).  The Python shim in
 * enhance-cb-whisper_amd/{efficient_kws,cbw} binds these with ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every buffer argument is a DEVICE pointer owned by the caller (PyTorch
 *     caching allocator); host pointers appear only in *_set_param;
 *   - `stream` is a hipStream_t (NULL = legacy default stream); calls are
 *     asynchronous, never synchronise, never allocate (capturable in hipGraphs);
 *     scratch comes from a caller-provided workspace sized by *_workspace_bytes;
 *   - return 0 on success, a negative CBW_ERR_* code otherwise; the message of
 *     the last failure on the calling thread is cbw_last_error();
 *   - bf16 tensors are passed as uint16_t*; layouts are given per argument;
 *   - handles are per device and not thread-safe.
 */
#ifndef CBW_H
#define CBW_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CBW_OK 0
#define CBW_ERR_INVALID (-1)   /* bad argument / unsupported shape (cf. ValueError in the reference) */
#define CBW_ERR_HIP (-2)       /* HIP runtime error */
#define CBW_ERR_OOM (-3)       /* device allocation failed / workspace too small */
#define CBW_ERR_STATE (-4)     /* handle not finalized / parameter missing */
#define CBW_ERR_NOT_FOUND (-5) /* unknown parameter name */

typedef void* cbw_stream_t; /* hipStream_t */
typedef struct cbw_kws cbw_kws;
typedef struct cbw_encoder cbw_encoder;

int cbw_version(void);
const char* cbw_last_error(void);
/* first 16 hex digits of sha256 over the library's sources as built (csrc/Makefile SRC_ID): a stale libcbw.so shows */
const char* cbw_source_id(void);

/* ---------------------------------------------------------------- KWS classifier
 * Replaces efficient_kws.model.KWSModel (efficient_kws/model.py:18-221) and the
 * Resnet it owns (efficient_kws/resnet.py:7-58).                                */
typedef struct {
    int n_layers;       /* L: Whisper layers = ResNet input channels (<= 4; <= 16 for variant 0,
                           the 12-channel CB-Whisper CNN, model/model.py:55-58)  model.py:29,73 */
    int embedding_dim;  /* D                                                         model.py:32    */
    int variant;        /* 0 = L (no projection), 1 = LE (proj_mlp), 2 = LEF (+frames_conv)       */
    int proj_units;     /* proj_mlp_units (64)                                       model.py:37    */
    int resnet_depth;   /* 18 | 34 | 50 (resnet_version)                             resnet.py:23-30 */
} cbw_kws_config;

int cbw_kws_create(const cbw_kws_config* cfg, cbw_kws** out);
int cbw_kws_destroy(cbw_kws* h);
/* one reference state_dict entry (KWSModel.state_dict() naming, fp32 host data);
 * replaces load_state_dict / KWSModel.load_from_checkpoint (cb_whisper.py:60)  */
int cbw_kws_set_param(cbw_kws* h, const char* name, const float* host, int64_t numel);
/* fold BatchNorm (eval statistics) into conv weights, convert, upload */
int cbw_kws_finalize(cbw_kws* h);

/* projector (model.py:143-166): x f32 [B][L][T][D] (per-frame L2-normalised hs),
 * mask f32 [B][L][T] -> out bf16 [B][L][T'][E] rows L2-normalised with
 * clamp(norm, 1e-6) (the sim_matrix normalisation, model.py:210-218), E = proj_units
 * (LE/LEF) or D (L); T' = floor((T-1)/2)+1 for LEF else T.  mask_out f32 [B][L][T']
 * (LEF: max-pooled; else a copy).                                */
int64_t cbw_kws_project_workspace_bytes(cbw_kws* h, int B, int T);
int cbw_kws_project(cbw_kws* h, const float* x, const float* mask, int B, int T, uint16_t* out, float* mask_out,
                    void* ws, int64_t ws_bytes, cbw_stream_t stream);

/* forward tail (model.py:167-193 + resnet.py:51-58): masked cosine-similarity maps
 * of utt bf16 [L][Tu][E] vs kwd bf16 [K][L][Tk][E] -> ResNet -> logits f32 [K][2].
 * features (optional) f32 [K][L][Tk][Tu] = KWSOutput.features (model.py:202-208).
 * Keywords are processed in chunks of `chunk` pairs.                            */
int64_t cbw_kws_workspace_bytes(cbw_kws* h, int Tk, int Tu, int chunk);
int cbw_kws_score(cbw_kws* h, const uint16_t* utt, const float* utt_mask, const uint16_t* kwd, const float* kwd_mask,
                  int K, int Tk, int Tu, float* logits, float* features, int chunk, void* ws, int64_t ws_bytes,
                  cbw_stream_t stream);

/* forward tail for a list of (utterance, keyword) pairs (model.py:171-193 with utt batch == n_keywords, and
 * batches of utterances against one keyword set): utt bf16 [B][L][Tu][E], utt_mask f32 [B][L][Tu], kwd / kwd_mask
 * as cbw_kws_score; pair p scores utterance pair_utt[p] against keyword pair_kwd[p] (device int32 [P], clamped
 * into range on the device); both NULL = every utterance against every keyword, p = b * K + k, and P must be B * K.
 * logits f32 [P][2] in pair order; features (optional) f32 [P][L][Tk][Tu].  Chunks of `chunk` pairs may span
 * utterances.  P == 0 returns CBW_OK and writes nothing.  Workspace: cbw_kws_workspace_bytes. */
int cbw_kws_score_pairs(cbw_kws* h, const uint16_t* utt, const float* utt_mask, int B, const uint16_t* kwd,
                        const float* kwd_mask, int K, int Tk, int Tu, const int32_t* pair_utt, const int32_t* pair_kwd,
                        int P, float* logits, float* features, int chunk, void* ws, int64_t ws_bytes,
                        cbw_stream_t stream);

/* fp8 first tier of the exact-decision cascade (BASELINE C5 "fp8 MFMA"; the ResNet of efficient_kws/resnet.py:51-58
 * called at efficient_kws/model.py:193): the stem and stage 1 on the bf16 network, stages 2-4 of ResNet-50 on
 * e4m3 operands (v_mfma_scale_f32_16x16x128_f8f6f4), one static scale per activation tensor, per-channel weight
 * scales.  cbw_kws_calibrate_fp8 (setup, synchronises): the fp32 network over the calibration pairs (sel, inputs as
 * cbw_kws_rescore) measures every stage-2..4 tensor's absolute maximum, scale = amax * margin / 448, and quantizes
 * the weights; cbw_kws_score_fp8: as cbw_kws_score (no features), logits of every pair from the fp8 network;
 * cbw_kws_set_score_offset_fp8: that pass's classifier bias = reference bias + offset; cbw_kws_fp8_scales: the
 * calibrated scales [stage-1 output, then per fp8 block x, t1, t2, shortcut] (returns their count). */
int cbw_kws_calibrate_fp8(cbw_kws* h, const float* utt, const float* utt_mask, const float* kwd, const float* kwd_mask,
                          int K, int Tk, int Tu, const int32_t* sel, int n_sel, float margin, void* ws, int64_t ws_bytes,
                          cbw_stream_t stream);
int cbw_kws_score_fp8(cbw_kws* h, const uint16_t* utt, const float* utt_mask, const uint16_t* kwd,
                      const float* kwd_mask, int K, int Tk, int Tu, float* logits, int chunk, void* ws, int64_t ws_bytes,
                      cbw_stream_t stream);
int cbw_kws_set_score_offset_fp8(cbw_kws* h, const float* offset);
int cbw_kws_fp8_scales(cbw_kws* h, float* scales, int max_n);

/* Resnet.forward on caller-built maps (efficient_kws/resnet.py:51-58):
 * maps f32 NCHW [K][L][Tk][Tu] -> logits f32 [K][2]; same workspace as cbw_kws_score. */
int cbw_kws_classify(cbw_kws* h, const float* maps, int K, int Tk, int Tu, float* logits, int chunk, void* ws,
                     int64_t ws_bytes, cbw_stream_t stream);

/* CB-Whisper's own spotter (model/cb_whisper.py:93-129, :189-210; model/model.py:78-93):
 * per-layer similarity of keyword frames vs utterance frames (plain inner products of
 * L2-normalised hs, no masks), each keyword's [Tk_k x Tu] matrices bilinearly resized to
 * (Ho, Wo) (torchvision resize, antialias=False), the n_layers-channel ResNet -> logits f32 [K][2].
 * Needs variant 0 (raw hs).  utt bf16 [L][Tu][D]; kwd bf16 [L][R][D] with keyword k on rows
 * off[k] .. off[k+1]-1; off_dev / off_host: the same int32 [K+1] offsets on device and host. */
int64_t cbw_kws_score_resized_workspace_bytes(cbw_kws* h, const int32_t* off_host, int K, int Tu, int D, int Ho,
                                              int Wo, int chunk);
int cbw_kws_score_resized(cbw_kws* h, const uint16_t* utt, int Tu, const uint16_t* kwd, int R, int D,
                          const int32_t* off_dev, const int32_t* off_host, int K, int Ho, int Wo, float* logits,
                          int chunk, void* ws, int64_t ws_bytes, cbw_stream_t stream);

/* The same spotter for a batch of segments in one pass (model/cb_whisper.py:87-129, :189-210: keyword_spotting
 * receives [S, n_mel, 3000] and scores every segment against every keyword).  utt bf16 [B][L][Tu][D]; kwd, off_dev
 * and off_host as cbw_kws_score_resized; logits f32 [B][K][2], pair p = b * K + k (the layout of
 * cbw_kws_score_pairs without index arrays).  chunk counts pairs: a chunk may start and end inside an utterance and
 * span several.  Per chunk one launch computes the similarity rows of all n_layers layers straight from utt (no
 * padded copy of the utterances), one the resize, then the ResNet.  Row b of logits is bit-identical to what
 * cbw_kws_score_resized writes for utterance b alone, whatever chunk is and whatever else the batch holds.
 * Checked in cbw_kws_score_resized's order, B < 1 with the sizes (CBW_ERR_INVALID); K == 0 returns CBW_OK and
 * writes nothing; a short workspace is CBW_ERR_OOM.  No allocation, no synchronisation, one stream.              */
int64_t cbw_kws_score_resized_batch_workspace_bytes(cbw_kws* h, const int32_t* off_host, int K, int B, int Tu, int D,
                                                    int Ho, int Wo, int chunk);
int cbw_kws_score_resized_batch(cbw_kws* h, const uint16_t* utt, int B, int Tu, const uint16_t* kwd, int R, int D,
                                const int32_t* off_dev, const int32_t* off_host, int K, int Ho, int Wo, float* logits,
                                int chunk, void* ws, int64_t ws_bytes, cbw_stream_t stream);
/* its first stage alone (tests): the similarity rows (cb_whisper.py:196) of pairs [p0, p0 + pc) of the B * K into
 * rows f32 [L][chunk rows][ld], the chunk's keywords' frames one after another in pair order; row t < Tk_k and
 * column u < Tu of each pair written, nothing else.  bf16 MFMA, fp32 accumulation, k ascending.  Refused before
 * any launch (CBW_ERR_INVALID): a null pointer, D % 64, ld < Tu, L > 16, B < 1, pc < 1, p0 + pc > B * K.        */
int cbw_kws_sim_rows_bf16(const uint16_t* utt, int B, int Tu, const uint16_t* kwd, int R, int D, int L,
                          const int32_t* off_dev, int K, int p0, int pc, int ld, float* rows, cbw_stream_t stream);

/* fp32 re-scoring (exact decisions; the reference evaluates in fp32, eval-*-comp-*.yaml precision
 * 32-true).  Same forward as cbw_kws_project / cbw_kws_score, every tensor fp32 and every conv on the
 * fp32-input MFMA (exact products, fp32 accumulation), BN folded in fp32, no conv fusion:
 *   cbw_kws_project_f32: x f32 [B][L][T][D] -> out f32 [B][L][T'][E] (rows L2-normalised, clamp 1e-6);
 *   cbw_kws_rescore: logits[sel[i]] (f32 [K][2]) <- the fp32 ResNet logits of keyword sel[i] (device
 *     int32 [n_sel]) vs the utterance; utt f32 [L][Tu][E], kwd f32 [K][L][Tk][E], masks as cbw_kws_score.
 * Used on the pairs whose bf16 probability lies near the threshold (efficient_kws KWSModel exact_band).
 * n_layers <= 4 only.                                                                           */
int64_t cbw_kws_project_f32_workspace_bytes(cbw_kws* h, int B, int T);
int cbw_kws_project_f32(cbw_kws* h, const float* x, const float* mask, int B, int T, float* out, float* mask_out,
                        void* ws, int64_t ws_bytes, cbw_stream_t stream);
int64_t cbw_kws_rescore_workspace_bytes(cbw_kws* h, int Tk, int Tu);
int cbw_kws_rescore(cbw_kws* h, const float* utt, const float* utt_mask, const float* kwd, const float* kwd_mask, int K,
                    int Tk, int Tu, const int32_t* sel, int n_sel, float* logits, void* ws, int64_t ws_bytes,
                    cbw_stream_t stream);

/* compensated-bf16 re-scoring (the middle tier between the bf16 scores and cbw_kws_rescore): the same
 * arguments and result as cbw_kws_rescore, but the 52 ResNet convs run on the bf16 MFMA kernels over a
 * 3-term split (activations [x_hi | x_hi | x_lo], weights [w_hi | w_lo | w_hi], fp32 accumulation: the
 * products of fp32 values to ~2^-16 relative), similarity maps, stem, pooling and the classifier in fp32.
 * About 3x the bf16 cost per pair instead of 16x for fp32-input MFMA; the band it leaves within the
 * decision threshold goes to cbw_kws_rescore.  n_layers <= 4 only.                                    */
int64_t cbw_kws_rescore_x3_workspace_bytes(cbw_kws* h, int Tk, int Tu);
int cbw_kws_rescore_x3(cbw_kws* h, const float* utt, const float* utt_mask, const float* kwd, const float* kwd_mask,
                       int K, int Tk, int Tu, const int32_t* sel, int n_sel, float* logits, void* ws,
                       int64_t ws_bytes, cbw_stream_t stream);

/* the two re-scoring tiers for a list of (utterance, keyword) pairs: the exact decisions of the paired batch of
 * efficient_kws/model.py:171-184 (utt batch == n_keywords, pair i = (utterance i, keyword i)) and of batches of
 * utterances against one keyword list decided by model.py:782-813, where cbw_kws_rescore / cbw_kws_rescore_x3
 * take one utterance.  utt f32 [B][L][Tu][E], utt_mask f32 [B][L][Tu], kwd / kwd_mask as cbw_kws_rescore
 * (cbw_kws_project_f32's outputs); pair p = (pair_utt[p], pair_kwd[p]) (device int32 [P]); both NULL = every
 * utterance against every keyword, p = b * K + k, and P must be B * K (the layout of cbw_kws_score_pairs).
 *   logits[sel[i]] (f32 [P][2], one row per pair) <- the tier's logits of pair sel[i] (device int32 [n_sel],
 *   indices into the P pairs).  A pair's logits are bit-identical to the per-utterance call's for that utterance
 *   and keyword; rows not selected are not written.  sel and the pair indices are clamped into range on the
 *   device before an operand is read; the logits row written is sel[i] itself, so sel must be valid.
 * CBW_ERR_INVALID: B < 1, n_sel > P, one index array NULL and the other not, P != B * K without index arrays.
 * P == 0 or n_sel == 0 returns CBW_OK and writes nothing.  Workspace: cbw_kws_rescore_workspace_bytes /
 * cbw_kws_rescore_x3_workspace_bytes (a pass's size does not depend on B).  The host-blocking dispatch throttle
 * of cbw_kws_rescore applies to cbw_kws_rescore_pairs unchanged: outside graph capture, a call over more than
 * 256 selected pairs waits on the host so that at most 16 passes are in flight.  n_layers <= 4 only.         */
int cbw_kws_rescore_pairs(cbw_kws* h, const float* utt, const float* utt_mask, int B, const float* kwd,
                          const float* kwd_mask, int K, int Tk, int Tu, const int32_t* pair_utt, const int32_t* pair_kwd,
                          int P, const int32_t* sel, int n_sel, float* logits, void* ws, int64_t ws_bytes,
                          cbw_stream_t stream);
int cbw_kws_rescore_x3_pairs(cbw_kws* h, const float* utt, const float* utt_mask, int B, const float* kwd,
                             const float* kwd_mask, int K, int Tk, int Tu, const int32_t* pair_utt,
                             const int32_t* pair_kwd, int P, const int32_t* sel, int n_sel, float* logits, void* ws,
                             int64_t ws_bytes, cbw_stream_t stream);

/* The exact tiers for CB-Whisper's own spotter.  The reference runs it in fp32 from fp32 hidden states
 * (model/cb_whisper.py:110-128: per-layer inner products :196, resize to kws_features_size :206,
 * Resnet(num_channels=12) model/model.py:55-58, argmax(logits) == 1 :128); cbw_kws_score_resized is its bf16 pass.
 *
 * cbw_kws_build_exact: the fp32 and compensated networks for a finalized variant-0 handle of any n_layers
 * (cbw_kws_finalize builds them itself only for n_layers <= 4, so a 12-channel handle that never asks pays
 * nothing).  Setup call: synchronises the device.  CBW_OK and no work where they already exist.               */
int cbw_kws_build_exact(cbw_kws* h);
/* cbw_kws_rescore_resized (fp32-input MFMA throughout) / cbw_kws_rescore_resized_x3 (compensated bf16, the fp32
 * stem where 3 n_layers > 16): logits[sel[i]] (f32 [K][2]) <- the tier's logits of keyword sel[i] (device int32
 * [n_sel], any order, repeats allowed); rows not selected are not written.  utt f32 [L][Tu][D]; kwd f32 [L][R][D]
 * with keyword k on rows off[k] .. off[k+1]-1 (off_dev / off_host as cbw_kws_score_resized), both per-frame
 * L2-normalised (cb_whisper.py:106, utils.py:195) and 16-byte aligned.  Per pass of 32 (fp32) / 64 (x3) keywords:
 * similarity rows (cb_whisper.py:196; exact fp32 products, fp32 accumulation, k ascending), bilinear resize to
 * (Ho, Wo) (cb_whisper.py:206; PyTorch upsample_bilinear2d, align_corners=False, no antialias) into fp32 NHWC
 * maps, then the passes of cbw_kws_rescore / cbw_kws_rescore_x3 (shared code, its host-blocking dispatch throttle
 * included).  sel is clamped into [0, K) on the device before an operand is read; the row written is sel[i]
 * itself.  A keyword's logits do not depend on what else is selected.  Checked in this order: variant 0, D % 16,
 * offsets in range and increasing, Ho, Wo >= 7 (CBW_ERR_INVALID), cbw_kws_build_exact called (CBW_ERR_STATE);
 * n_sel == 0 then returns CBW_OK.  No allocation, no synchronisation outside the throttle.                     */
int64_t cbw_kws_rescore_resized_workspace_bytes(cbw_kws* h, const int32_t* off_host, int K, int Tu, int D, int Ho,
                                                int Wo);
int cbw_kws_rescore_resized(cbw_kws* h, const float* utt, int Tu, const float* kwd, int R, int D, const int32_t* off_dev,
                            const int32_t* off_host, int K, int Ho, int Wo, const int32_t* sel, int n_sel, float* logits,
                            void* ws, int64_t ws_bytes, cbw_stream_t stream);
int64_t cbw_kws_rescore_resized_x3_workspace_bytes(cbw_kws* h, const int32_t* off_host, int K, int Tu, int D, int Ho,
                                                   int Wo);
int cbw_kws_rescore_resized_x3(cbw_kws* h, const float* utt, int Tu, const float* kwd, int R, int D,
                               const int32_t* off_dev, const int32_t* off_host, int K, int Ho, int Wo, const int32_t* sel,
                               int n_sel, float* logits, void* ws, int64_t ws_bytes, cbw_stream_t stream);
/* the two tiers for a batch of segments (cb_whisper.py:87-129): utt f32 [B][L][Tu][D]; sel (device int32 [n_sel])
 * indexes the P = B * K pairs p = b * K + k, the rows of logits f32 [B * K][2] (cbw_kws_score_resized_batch's
 * layout).  logits[sel[i]] <- the tier's logits of pair sel[i]: bit-identical to the per-utterance call's for that
 * utterance and keyword; rows not selected are not written.  sel is clamped into [0, B * K) on the device before an
 * operand is read; the row written is sel[i] itself.  Checks as above, and CBW_ERR_INVALID for B < 1 and
 * n_sel > B * K; n_sel == 0 returns CBW_OK.  Workspace: cbw_kws_rescore_resized_workspace_bytes /
 * cbw_kws_rescore_resized_x3_workspace_bytes (a pass's size does not depend on B).  The host-blocking dispatch
 * throttle of cbw_kws_rescore applies unchanged: outside graph capture, a call over more than 256 selected pairs
 * waits on the host so that at most 16 passes are in flight.  The per-utterance calls are the B = 1 case.        */
int cbw_kws_rescore_resized_batch(cbw_kws* h, const float* utt, int B, int Tu, const float* kwd, int R, int D,
                                  const int32_t* off_dev, const int32_t* off_host, int K, int Ho, int Wo,
                                  const int32_t* sel, int n_sel, float* logits, void* ws, int64_t ws_bytes,
                                  cbw_stream_t stream);
int cbw_kws_rescore_resized_x3_batch(cbw_kws* h, const float* utt, int B, int Tu, const float* kwd, int R, int D,
                                     const int32_t* off_dev, const int32_t* off_host, int K, int Ho, int Wo,
                                     const int32_t* sel, int n_sel, float* logits, void* ws, int64_t ws_bytes,
                                     cbw_stream_t stream);
/* the two stages of a pass one by one (tests): rows f32 [n_sel][L][tk_max][ld] (ld >= Tu; row t < Tk_k and column
 * u < Tu of map i = keyword sel[i] written, cb_whisper.py:196), then maps f32 NHWC [n_sel][Ho][Wo][L]
 * (cb_whisper.py:206).  tk_max bounds the keyword lengths read; D % 16 == 0, L <= 16.                           */
int cbw_kws_sim_rows_f32(const float* utt, int Tu, const float* kwd, int R, int D, int L, const int32_t* off_dev, int K,
                         const int32_t* sel, int n_sel, int tk_max, int ld, float* rows, cbw_stream_t stream);
int cbw_kws_sim_resize_f32(const float* rows, int Tu, int R, int L, const int32_t* off_dev, int K, const int32_t* sel,
                           int n_sel, int tk_max, int ld, int Ho, int Wo, float* maps, cbw_stream_t stream);

/* bias correction of the bf16 scoring network (setup, no counterpart in the reference: it only narrows the
 * bf16 error the exact tiers must cover).  Runs the fp32 network (cbw_kws_rescore's arguments and
 * workspace) over the n_sel calibration pairs, takes each conv's mean input per channel E[x_c], and sets
 * the bf16 conv's bias to b + sum_{kh,kw,c} E[x_c] (w - bf16(w)) (the mean output shift of rounding the
 * weights; Nagel et al. 2019).  The fp32 and compensated tiers are unchanged.  Synchronises `stream`;
 * n_sel == 0 restores the folded biases.  n_layers <= 4 only.                                     */
int cbw_kws_calibrate_bias(cbw_kws* h, const float* utt, const float* utt_mask, const float* kwd, const float* kwd_mask,
                           int K, int Tk, int Tu, const int32_t* sel, int n_sel, void* ws, int64_t ws_bytes,
                           cbw_stream_t stream);
/* the bf16 scoring pass's logit offset: its classifier bias becomes classifier.1.bias + offset (host f32 [2]);
 * the compensated and fp32 tiers keep the reference bias.  KwsEngine.calibrate_bias sets it to the mean
 * fp32 - bf16 logit difference over the calibration pairs (the systematic error the weight correction
 * leaves); {0, 0} restores the reference bias.  Synchronous.                                            */
int cbw_kws_set_score_offset(cbw_kws* h, const float* offset);

/* measurement hooks (bench.py roofline): with max_launches > 0, every following
 * implicit-GEMM conv launch of this handle (up to max_launches) is bracketed by
 * hipEvents on its stream; _read (after the work completed) returns the summed
 * kernel time (ms), the summed algorithmic FLOPs 2*M*Cout*Cin*KH*KW and the
 * launch count, and rewinds.  max_launches = 0 disables.  Allocates events:
 * call outside graph capture.                                                   */
int cbw_kws_profile(cbw_kws* h, int max_launches);
int cbw_kws_profile_read(cbw_kws* h, double* ms, double* flop, int* n_launches);
/* the recorded launches themselves (call before _read, which rewinds): per launch its start / end (ms after
 * the first recorded launch started) and algorithmic FLOPs, up to max_records; returns the number recorded */
int cbw_kws_profile_records(cbw_kws* h, double* start_ms, double* end_ms, double* flop, int max_records);
/* The tier of each recorded launch (0 the bf16 scoring pass, 1 the compensated re-scoring tier, whose convs are
 * recorded too: their FLOPs are the split GEMMs' 2 M N K with K over the three segments).  Returns the count. */
int cbw_kws_profile_tiers(cbw_kws* h, int32_t* tier, int max_records);
/* The kernel each recorded launch ran (rocprofv3's short kernel name with its template arguments, e.g.
 * "conv_igemm_p8<1, 1, 256>"; the fused stage-1 blocks "bottleneck_kernel<64>" / "bottleneck_ring_kernel"): static
 * strings owned by the library.  Returns the count (round 6: bench.py's per-kernel in-bench roofline table). */
int cbw_kws_profile_kernels(cbw_kws* h, const char** kernel, int max_records);

/* decision (model.py:782-799, :804-813): prob = softmax(logits)[:,1] * ghost;
 * mode 0: idx = sorted {k : prob >= thr}; mode 1: argmax(logits) == 1
 * (cb_whisper.py:128).  prob (optional) f32 [K]; idx int32 [K]; n int32 [1].   */
int cbw_kws_spot(const float* logits, const float* ghost, int K, float thr, int mode, float* prob, int32_t* idx,
                 int32_t* n, cbw_stream_t stream);
/* 64-bit content checksum of a device byte range (16-byte aligned; position-dependent, not cryptographic): the
 * key of the keyword-database projection cache (efficient_kws.model.KWSModel re-projects the database when its
 * content changed, where the reference re-projects every group on every call, efficient_kws/model.py:767-780).
 * out: device uint64 [1]; ws >= cbw_checksum_workspace_bytes().                                             */
int64_t cbw_checksum_workspace_bytes(void);
int cbw_checksum(const void* data, int64_t bytes, uint64_t* out, void* ws, int64_t ws_bytes, cbw_stream_t stream);
/* the near-threshold band of the bf16 scores (the pairs cbw_kws_rescore re-runs in fp32 so the decision of
 * model.py:810-813 follows the reference's fp32 evaluation, eval-*-comp-*.yaml:8 `32-true`):
 * idx = sorted {k : |softmax(logits[k])[1] * ghost[k] - thr| <= band}, n = count (device int32).      */
int cbw_kws_band(const float* logits, const float* ghost, int K, float thr, float band, int32_t* idx, int32_t* n,
                 cbw_stream_t stream);
/* the same band with a half-width proportional to the pair's logit magnitude:
 * idx = sorted {k : |p[k] - thr| <= coef * max(|logits[k][0]|, |logits[k][1]|)} (the bf16 rounding error of a
 * pair's decision variable scales with its activations).                                  */
int cbw_kws_band_scaled(const float* logits, const float* ghost, int K, float thr, float coef, int32_t* idx,
                        int32_t* n, cbw_stream_t stream);

/* ---------------------------------------------------------------- resample + downmix
 * Replaces `torch.mean(waveform, dim=0)` + `torchaudio.functional.resample(waveform, sample_rate, 16000)` in front
 * of the feature extractor (utils.py:179-184, efficient_kws/dataset.py:472-483): torchaudio's sinc_interp_hann
 * defaults (lowpass_filter_width 6, rolloff 0.99) as a polyphase filter.  With g = gcd(orig, new_), o = orig / g,
 * n = new_ / g:  base = min(o, n) * 0.99, width = ceil(6 o / base), T = 2 width + o taps in each of n phases,
 *   t[j][k] = clamp((-j / n + (k - width) / o) * base, -6, 6),
 *   kernel[j][k] = sinc(pi t) * cos^2(pi t / 12) * base / o        (sinc(0) = 1),
 *   y[f n + j] = sum_k xpad[f o + k] * kernel[j][k],  xpad = x with `width` zeros in front and width + o behind,
 * y cut to cbw_resample_len = ceil(n * len / o) samples.  The table is evaluated in float64 on the host and rounded
 * to fp32 once (torchaudio evaluates it in fp32: bit parity with torchaudio is not the aim); the sum
 * is fp32 fmaf in ascending k, so a sample's bits do not depend on the launch shape or on where the input lies.
 * pcm f32 [channels][n] (device); each tap reads the mean over the channels (their sum in channel order, divided
 * once: the mean first, then the filter, the reference's order); out f32 [cbw_resample_len(n, orig, new_)].
 * orig == new_: a copy (channels == 1) or the mean alone; cbw_resample_ws_bytes is then 0 and ws is not read.
 * ws (4-byte aligned, >= cbw_resample_ws_bytes(orig, new_) = n T floats) receives the table by a stream-ordered copy.
 * The first call of a process for a rate pair evaluates that pair's table into pinned host memory, which is kept;
 * every later call neither allocates nor synchronises.
 * CBW_ERR_INVALID (checked in this order, nothing launched): pcm or out null; channels < 1; n < 0; a rate < 1;
 * a table of more than CBW_RESAMPLE_MAX_TABLE = 2^20 entries (4 MiB: 44100 -> 16000 needs 160 x 475 = 76 000,
 * 16001 -> 16000 would need 16000 x 16015 and is refused); n * new_ / o or its launch grid out of range
 * (more than 2^31 - 1 blocks of 256 outputs); ws null, misaligned or smaller than cbw_resample_ws_bytes.
 * The two helpers return CBW_ERR_INVALID (-1) for the arguments cbw_resample refuses.  n == 0 returns CBW_OK.   */
#define CBW_RESAMPLE_MAX_TABLE (1 << 20)
int64_t cbw_resample_len(int64_t n, int orig, int new_);
int64_t cbw_resample_ws_bytes(int orig, int new_);
int cbw_resample(const float* pcm, int channels, int64_t n, int orig, int new_, float* out, void* ws,
                 int64_t ws_bytes, cbw_stream_t stream);

/* ---------------------------------------------------------------- Whisper front end
 * Replaces WhisperFeatureExtractor(padding='max_length') (utils.py:186-187).
 * pcm f32 [n] (16 kHz) -> out f32 [n_mel][3000]; packed (optional) bf16 [3000][cpad]
 * time-major copy for cbw_encoder_hs (cpad >= n_mel, multiple of 64).
 * ws: >= 64 bytes.                                                              */
int cbw_mel(const float* pcm, int64_t n, int n_mel, float* out, uint16_t* packed, int cpad, void* ws,
            cbw_stream_t stream);
/* long-form features (the input of PBAWhisper.generate beyond 30 s, pba_whisper.py:343-475):
 * WhisperFeatureExtractor(padding='longest', truncation=False) of one waveform -- reflect padding at the
 * audio's ends, no zero padding, out f32 [n_mel][n / 160], the max - 8 floor over the whole audio.
 * ws >= 1 KB (partial maxima).                                                                        */
int cbw_mel_long(const float* pcm, int64_t n, int n_mel, float* out, void* ws, cbw_stream_t stream);

/* ---------------------------------------------------------------- Whisper encoder
 * Replaces WhisperModel.encoder(input_features, output_hidden_states=True)
 * (cb_whisper.py:100-104, utils.py:188-192).                                    */
typedef struct {
    int n_mel, d_model, n_layers, n_heads, ffn_dim;
} cbw_encoder_config;
int cbw_encoder_create(const cbw_encoder_config* cfg, cbw_encoder** out);
int cbw_encoder_destroy(cbw_encoder* h);
int cbw_encoder_set_param(cbw_encoder* h, const char* name, const float* host, int64_t numel);
int cbw_encoder_finalize(cbw_encoder* h);
int64_t cbw_encoder_workspace_bytes(cbw_encoder* h, int B);
/* mel bf16 [B][3000][cpad] (cpad = n_mel rounded up to 64) -> hs f32 [B][n_ids][1500][D]
 * = hidden_states[layer_ids[i]] (0 = embeddings, i = layer i output, n_layers = post-LN),
 * layer_ids is a HOST int32 array.  flags bit 0: divide by the per-frame L2 norm
 * (cb_whisper.py:106, utils.py:195); bit 1: stop after the last requested state
 * (same outputs, skips the layers no requested state depends on).               */
int cbw_encoder_hs(cbw_encoder* h, const uint16_t* mel, int B, const int32_t* layer_ids, int n_ids, int normalize,
                   float* hs, void* ws, int64_t ws_bytes, cbw_stream_t stream);

/* ---------------------------------------------------------------- Whisper decoder
 * Replaces the per-step WhisperDecoder forward that PBAWhisper.generate drives through
 * HF beam search (pba_whisper.py:323-331 short-form, :425-442 long-form).  B decoding
 * rows (= batch x beams) share Benc encoder items (row r reads item r / (B/Benc)).
 * `state` (size cbw_decoder_state_bytes) holds the self-attention KV cache
 * [L][B][max_len][D] and the cross-attention KV [L][Benc][1500][D] (bf16) plus scratch. */
typedef struct {
    int vocab, d_model, n_layers, n_heads, ffn_dim, max_len;   /* max_len <= 448 (max_target_positions) */
} cbw_decoder_config;
typedef struct cbw_decoder cbw_decoder;
int cbw_decoder_create(const cbw_decoder_config* cfg, cbw_decoder** out);
int cbw_decoder_destroy(cbw_decoder* h);
/* HF WhisperDecoder names without the `model.decoder.` prefix (embed_tokens is also proj_out) */
int cbw_decoder_set_param(cbw_decoder* h, const char* name, const float* host, int64_t numel);
int cbw_decoder_finalize(cbw_decoder* h);
int cbw_decoder_vocab_padded(cbw_decoder* h);   /* logits row pitch: vocab rounded up to 128 */
int64_t cbw_decoder_state_bytes(cbw_decoder* h, int B, int Benc);
/* cross-attention K/V from the post-LN encoder output f32 [Benc][1500][D] (once per window) */
int cbw_decoder_cross_kv(cbw_decoder* h, const float* enc_out, int Benc, void* state, int64_t state_bytes, int B,
                         cbw_stream_t stream);
/* one token per row at position pos (tokens int32 [B], device) -> logits f32 [B][vocab_padded] */
int cbw_decoder_step(cbw_decoder* h, const int32_t* tokens, int pos, int B, int Benc, void* state, int64_t state_bytes,
                     float* logits, cbw_stream_t stream);
/* the same step with the position read from device memory (pos_dev: one int32): every launch argument is then
 * independent of the position, so a caller can capture one step into a hipGraph and replay it for every
 * position (write *pos_dev, replay).  Needs the fused GEMV path (B <= 16, the defaults).                   */
int cbw_decoder_step_dev(cbw_decoder* h, const int32_t* tokens, const int32_t* pos_dev, int B, int Benc, void* state,
                         int64_t state_bytes, float* logits, cbw_stream_t stream);
/* beam reorder of the self-attention cache: row r <- row src_rows[r] for positions [0, len) */
/* Prefill of a forced prefix (replaces stepping the forced decoder_input_ids one token at a time): the T
 * prefix tokens (device int32 [T]) run as T rows at positions 0..T-1 with causal self-attention; their K/V
 * go to positions 0..T-1 of all B beam rows (identical through a forced prefix, HF beam search); logits
 * (f32 [vocab_padded]) receives the last token's logits.  Benc must be 1.  The next cbw_decoder_step is at
 * pos = T. */
int cbw_decoder_prefill(cbw_decoder* h, const int32_t* tokens, int T, int B, int Benc, void* state,
                        int64_t state_bytes, float* logits, cbw_stream_t stream);
/* Several windows in one decode step (rows = windows x beams, Benc = windows; no reference counterpart: the
 * reference decodes one audio per generate call, pba_whisper.py:343-475 -- this batches the long-form windows of
 * several audios so each step streams the decoder weights once for all of them).  Window w's beams are rows
 * [w nb, (w + 1) nb) and attend to encoder slot w.
 * cross_kv_slot: slot `slot`'s cross-attention K/V from enc_out f32 [1500][D] (the other slots untouched).
 * prefill_rows: cbw_decoder_prefill into rows [r0, r0 + nb) against slot `slot` (the other rows untouched);
 *   logits (f32 [vocab_padded]) receives the last token's logits.
 * step_rows: cbw_decoder_step_dev with one position per row (pos_rows: device int32 [B]); each row's logits
 *   equal those of a step over its window alone (bit for bit: the rows' arithmetic does not depend on B). */
int cbw_decoder_cross_kv_slot(cbw_decoder* h, const float* enc_out, int slot, int Benc, void* state,
                              int64_t state_bytes, int B, cbw_stream_t stream);
int cbw_decoder_prefill_rows(cbw_decoder* h, const int32_t* tokens, int T, int slot, int r0, int nb, int B, int Benc,
                             void* state, int64_t state_bytes, float* logits, cbw_stream_t stream);
int cbw_decoder_step_rows(cbw_decoder* h, const int32_t* tokens, const int32_t* pos_rows, int B, int Benc, void* state,
                          int64_t state_bytes, float* logits, cbw_stream_t stream);
/* cbw_decoder_step_rows for 1 <= B <= CBW_DEC_WIDE_ROWS rows (a batch of short clips: 16 windows x 5 beams in one
 * step): every Linear runs as ceil(B / 16) row groups in one launch, each group on the 16-row kernel of
 * cbw_decoder_step_rows, and the embedding and attention launches are those of the narrower step -- so each row's
 * logits equal, bit for bit, those of a step over its window alone on a state of <= 16 rows.  B % Benc == 0 and
 * B / Benc <= 8 (the split cross-attention reads a window's K/V once for its rows).  Each row group re-reads the
 * Linear's weights.  cbw_decoder_prefill_rows and cbw_decoder_reorder serve a state of up to 80 rows as they are. */
#define CBW_DEC_WIDE_ROWS 80
int cbw_decoder_step_wide(cbw_decoder* h, const int32_t* tokens, const int32_t* pos_rows, int B, int Benc, void* state,
                          int64_t state_bytes, float* logits, cbw_stream_t stream);
/* Cross-attention probabilities for token-level timestamps (transformers WhisperGenerationMixin.
 * _extract_token_timestamps, reached from pba_whisper.py:333-336 and the long-form return_token_timestamps path,
 * :425-442): the decoder runs teacher-forced over tokens[0..T) (device int32) against encoder slot 0 of `state`
 * (cbw_decoder_cross_kv first), writing its K/V into cache row 0, and for each (layer, head) pair i of `heads`
 * (host int32 [2 n]) probs[i][t][j] = softmax_j(q_t . k_j) over the 1500 encoder frames (device f32 [n][T][1500]):
 * the weights generate's cross_attentions carry for the alignment heads, one query row per decoder position. */
int cbw_decoder_cross_attn_probs(cbw_decoder* h, const int32_t* tokens, int T, const int32_t* heads, int n, int B,
                                 int Benc, void* state, int64_t state_bytes, float* probs, cbw_stream_t stream);
/* Dynamic time warping for token-level timestamps (host code, transformers' _dynamic_time_warping): matrix f64
 * [rows][cols] (host, row-major; the negated, normalised, median-filtered mean alignment weights); writes the
 * warping path as text_idx / time_idx (host int32, >= rows + cols entries) and its length to *len. */
int cbw_dtw(const double* matrix, int rows, int cols, int32_t* text_idx, int32_t* time_idx, int* len);
/* Token-level timestamps on the GPU: what transformers' _extract_token_timestamps (reached from pba_whisper.py:333-336,
 * 425-442) does with the weights, beside the host statement in cbw/token_timestamps.py, which stays the reference and
 * the fallback.  Every pointer is device memory; nothing allocates or synchronises.
 * cbw_align_matrix: probs f32 [n][T_all][1500] (cbw_decoder_cross_attn_probs' output), the positions [t0, t0 + T)
 *   (t0 > 0: the "5.x" variant, which drops the decoder input ids before normalising), the first F frames and an odd
 *   median width in {1, 3, 5, 7} -> matrix f32 [T][F], row-major: the negated head mean of the median-filtered
 *   normalised weights.  Per head and frame the mean over the T positions and the population variance (second pass,
 *   sum (w - mean)^2 / T) in float64, z = (float)((w - mean) / sqrt(var)), the median along the frames by exact
 *   selection with torch's reflect padding (none where F <= width / 2), the heads summed in fp32 in ascending order,
 *   divided by n, negated.  *degenerate (int32) is 0, or non-zero where a variance among the used frames is zero or
 *   not finite: the host path gives NaN there and the matrix is then not to be used.
 * cbw_dtw_dev: matrix f32 [T][F] -> first_frame int32 [T], the time index at which the warping path enters each text
 *   row (the jump frames of _extract_token_timestamps), by cbw_dtw's arithmetic bit for bit (fp32 tables, strict
 *   comparisons: diagonal, row above, else left).  text_idx / time_idx (int32, >= T + F entries) and len (int32) are
 *   all NULL, or all set and receive what cbw_dtw writes for the same matrix.  One workgroup, one thread per text row.
 * ws (4-byte aligned, >= cbw_token_ts_ws_bytes(T, F) = 4 T ceil((T + F - 1) / 16) bytes) holds the DTW's trace, 2 bits
 *   per cell in words of 16 anti-diagonals per text row; cbw_align_matrix keeps its statistics on chip and only checks
 *   ws, so that one buffer serves both calls.
 * CBW_ERR_INVALID before any GPU work for: a null pointer; n < 1; T < 2 (matrix) or T < 1 (DTW); T > 1024; t0 < 0 or
 *   t0 + T > T_all; F < 1 or F > 1500; an even width or one above 7; path pointers partly set; ws null, misaligned or
 *   too small.  cbw_token_ts_ws_bytes returns CBW_ERR_INVALID (-1) for a T or F that the two refuse.              */
int64_t cbw_token_ts_ws_bytes(int T, int F);
int cbw_align_matrix(const float* probs, int n, int T_all, int t0, int T, int F, int width, float* matrix,
                     int32_t* degenerate, void* ws, int64_t ws_bytes, cbw_stream_t stream);
int cbw_dtw_dev(const float* matrix, int T, int F, int32_t* first_frame, int32_t* text_idx, int32_t* time_idx,
                int32_t* len, void* ws, int64_t ws_bytes, cbw_stream_t stream);
/* Token-level timestamps for a batch of decoded rows (a batch of short clips, cbw_decoder_step_wide's callers: what
 * transformers' _extract_token_timestamps, reached from pba_whisper.py:333-336 and 425-442, gives each row; the
 * reference takes one clip per call, so the batching has no counterpart there).
 * cbw_decoder_cross_attn_probs_slot: cbw_decoder_cross_attn_probs against encoder slot `slot` of a lock-step state
 *   (cbw_decoder_cross_kv_slot first), the row's self-attention K/V written into cache row r0; the other slots'
 *   cross K/V and the other rows' self K/V are not touched.  The arithmetic follows T alone -- not B, Benc, slot or
 *   r0 -- so the probabilities equal, bit for bit, those of cbw_decoder_cross_attn_probs on a one-window state with
 *   the same encoder output.  One call per window: several windows' rows in one GEMM pass would change the tile
 *   and split-K choice, which follows the row count.  CBW_ERR_INVALID before any GPU work for what
 *   cbw_decoder_cross_attn_probs refuses and for slot outside [0, Benc) or r0 outside [0, B).
 * cbw_align_matrix_batch / cbw_dtw_dev_batch: cbw_align_matrix and cbw_dtw_dev (without the path) for N windows,
 *   1 <= N <= CBW_TOKEN_TS_MAX_WINDOWS, in one launch each: the windows' table `win` (host memory, read during the
 *   call) goes to the kernel by value, the window is a coordinate of the grid, and the alignment matrix, the DTW
 *   wavefront and the trace of a window are those of the single-window calls bit for bit.  Window i reads
 *   probs + probs_off (f32 [n][T_all][1500]), writes matrix + matrix_off (f32 [T][F]) and keeps its trace at
 *   (char*)ws + ws_off; probs_off and matrix_off count floats, ws_off counts bytes and is a multiple of 4; none is
 *   negative; the caller keeps the windows' ranges apart.  n heads and the median width are shared.
 *   degenerate int32 [N]: window i's flag (a flagged window's outputs are not to be used; the others' are not
 *   disturbed).  first_frame int32 [N][ld], ld >= the largest T: row i holds window i's T jump frames.
 *   cbw_token_ts_ws_bytes_batch: the bytes of ws for the table packed back to back, the sum of the windows'
 *   cbw_token_ts_ws_bytes(T, F) (each a multiple of 4, the alignment of ws_off); -1 as the calls refuse.
 *   Nothing allocates or synchronises.  CBW_ERR_INVALID before any GPU work, per window, for what the single-window
 *   entries refuse (T < 2 for the matrix, T < 1 for the DTW, T > 1024, F outside [1, 1500], t0 < 0 or t0 + T > T_all,
 *   n < 1, an even width or one above 7, a null pointer, ws misaligned or ws_off + the window's bytes > ws_bytes),
 *   and for N out of range, a negative offset, a ws_off that is no multiple of 4, ld below the largest T.        */
#define CBW_TOKEN_TS_MAX_WINDOWS 16
typedef struct {
    int32_t T_all, t0, T, F;
    int64_t probs_off, matrix_off;   /* floats */
    int64_t ws_off;                  /* bytes, a multiple of 4 */
} cbw_token_ts_window;
int cbw_decoder_cross_attn_probs_slot(cbw_decoder* h, const int32_t* tokens, int T, const int32_t* heads, int n,
                                      int slot, int r0, int B, int Benc, void* state, int64_t state_bytes,
                                      float* probs, cbw_stream_t stream);
int64_t cbw_token_ts_ws_bytes_batch(const cbw_token_ts_window* win, int N);
int cbw_align_matrix_batch(const float* probs, int n, const cbw_token_ts_window* win, int N, int width, float* matrix,
                           int32_t* degenerate, void* ws, int64_t ws_bytes, cbw_stream_t stream);
int cbw_dtw_dev_batch(const float* matrix, const cbw_token_ts_window* win, int N, int32_t* first_frame, int ld,
                      void* ws, int64_t ws_bytes, cbw_stream_t stream);
int cbw_decoder_reorder(cbw_decoder* h, const int32_t* src_rows, int B, int Benc, int len, void* state,
                        int64_t state_bytes, cbw_stream_t stream);
/* HF beam-search scores: log_softmax(logits) + bias, and their top-k (k <= 16, ties -> lower id) per
 * row.  bias = the logits processors as additive -inf masks, f32 [V] shared (bias_ld = 0) or per row
 * [B][bias_ld] (the timestamp rules), or NULL; the normaliser is the RAW logits' logsumexp
 * (next_token_scores = log_softmax(logits) before the processors).  lp f32 [B][k], idx int32 [B][k]. */
int cbw_logprob_topk(const float* logits, int B, int V, int ld, const float* bias, int64_t bias_ld, int k, float* lp,
                     int32_t* idx, cbw_stream_t stream);
/* WhisperTimeStampLogitsProcessor (long-form, return_timestamps; pba_whisper.py:425-442 runs it through
 * HF generate): per row r, bias_out[r][V] = bias (shared [V] suppression or NULL) + the timestamp masks
 * for that row's state[r] = {last_was_timestamp, penultimate_was_timestamp, lowest allowed timestamp
 * id, at_begin}; max_initial < 0 disables max_initial_timestamp_index.                             */
int cbw_timestamp_rules(const float* logits, int B, int V, int ld, const float* bias, const int32_t* state,
                        int timestamp_begin, int no_timestamps, int eos, int max_initial, float* bias_out,
                        cbw_stream_t stream);

/* One beam-search step's bookkeeping on the GPU (HF 4.37 BeamSearchScorer.process's next-beam choice,
 * generate/beam_search.py as pinned by cbw/generate.py), so a decode loop needs no host round trip per
 * token: candidates beam_scores[r] (f64 [B], in/out) + lp[r][j] (cbw_logprob_topk, [B][k]) sorted by
 * (score desc, row, token), top k logged to cand_score f64 [k], cand_row / cand_tok int32 [k] (the host
 * replays the EOS candidates into its finished hypotheses and detects the end); the first B non-EOS
 * candidates become the next beams: tokens / parents int32 [B] (parents feed cbw_decoder_reorder), *ok = 1
 * when B were found.  ts_state int32 [B][4] = {n, last, second last, last timestamp (-1)} of each row's
 * tokens at positions >= the rules' begin index, advanced by this step's token when count != 0 and gathered
 * from the parent rows; st_out int32 [B][4] = the cbw_timestamp_rules state for the next position. */
int cbw_beam_select(const float* lp, const int32_t* idx, int B, int k, int eos, double* beam_scores,
                    double* cand_score, int32_t* cand_row, int32_t* cand_tok, int32_t* tokens, int32_t* parents,
                    int32_t* ok, int32_t* ts_state, int32_t* st_out, int timestamp_begin, int count,
                    cbw_stream_t stream);

/* One greedy-search step's choice for up to 16 rows on the GPU, so a greedy decode loop needs no host round trip
 * per token (replaces the greedy branch of GenerationMixin.generate, num_beams = 1 and do_sample = False, reached
 * from pba_whisper.py:318-331 short-form and :425-442 long-form, temperature 0 of the fallback included): per active
 * row r, scores = logits[r] (f32, row pitch ld) + the shared bias (bias_begin [V] when the row has sampled nothing
 * yet, ts_state[r][0] == 0, else bias [V]; either may be NULL) + WhisperTimeStampLogitsProcessor's masks as
 * cbw_timestamp_rules applies them, the rule state derived from ts_state[r] (cbw_beam_select's {n, last, second last,
 * last timestamp (-1)}); timestamp_begin < 0 switches the rules off.  No [B][V] bias is written or read.
 * tokens[r] = argmax of the scores (ties -> lower id, as cbw_logprob_topk), logprob[r] = log_softmax(scores)[token]
 * (HF applies the processors to the raw logits, then normalises); a row with nothing finite left gets eos and -inf.
 * ts_state[r] advances by the token; active[r] = token != eos && pos_rows[r] + 1 < limit[r] (device int32 [B] each:
 * the position the token goes to, the row's max_length) -- also the increment the caller adds to pos_rows after the
 * decode step.  A row with active[r] == 0 on entry only gets tokens[r] = eos.  An active row therefore steps at
 * pos <= limit - 2 and an ended row stays at pos <= limit - 1: cbw_decoder_step_rows over all rows stays below
 * max_len for limit <= max_len.  Does not allocate or synchronise.  B in [1, 16], V >= 1, ld >= V. */
int cbw_greedy_select(const float* logits, int B, int V, int ld, const float* bias, const float* bias_begin,
                      int timestamp_begin, int no_timestamps, int eos, int max_initial, int32_t* ts_state,
                      const int32_t* pos_rows, const int32_t* limit, int32_t* active, int32_t* tokens, float* logprob,
                      cbw_stream_t stream);

/* One sampling step's choice for up to 16 rows on the GPU, so a temperature-sampling decode loop needs no host round
 * trip per token (replaces the sample branch of GenerationMixin.generate, num_beams = 1 and do_sample = True, reached
 * from pba_whisper.py:318-331 short-form and from every temperature > 0 rung of generate_with_fallback, :425-442).
 * cbw_greedy_select's arguments and bookkeeping (ts_state, active, the position invariant, a row inactive on entry
 * only gets tokens[r] = eos), with the choice replaced: s = the processed scores exactly as cbw_greedy_select forms
 * them; the kept set is {i : s_i finite and s_i >= the top_k-th largest s} (TopKLogitsWarper: ties at the threshold
 * all kept, exact; fewer than top_k finite scores: all of them); tokens[r] = argmax over the kept i of
 * softmax_kept(s / temperature)_i / noise[r][i] in fp32 (ties -> lower id), which is torch.multinomial's draw when
 * noise holds the Exp(1) numbers it would draw (noise f32 [B][noise_ld], noise_ld >= V; an entry that is not positive
 * and finite reads as FLT_MIN); logprob[r] = s[token] - logsumexp over the kept s (log_softmax of the top-k-filtered
 * scores at temperature 1, what HF's fallback checks read); nothing finite left: eos and -inf.  tokens[r] is always in
 * [0, V) or eos.  Does not allocate or synchronise and draws no random numbers itself.  B in [1, 16], V in [1, 52224]
 * (a workgroup holds its row's scores in registers), ld >= V, temperature > 0 and finite, top_k >= 1. */
int cbw_sample_select(const float* logits, int B, int V, int ld, const float* bias, const float* bias_begin,
                      int timestamp_begin, int no_timestamps, int eos, int max_initial, int32_t* ts_state,
                      const int32_t* pos_rows, const int32_t* limit, int32_t* active, int32_t* tokens, float* logprob,
                      float temperature, int top_k, const float* noise, int64_t noise_ld, cbw_stream_t stream);

/* The two logits processors that read a row's token history, for up to 16 rows on the GPU in front of
 * cbw_greedy_select / cbw_sample_select, so a lock-step decode with repetition_penalty or no_repeat_ngram_size needs no
 * host round trip per token (the kwargs pba_whisper.py:320-331 and :425-442 hand down to GenerationMixin.generate;
 * transformers 4.37.2 _get_logits_processor puts RepetitionPenaltyLogitsProcessor, then NoRepeatNGramLogitsProcessor,
 * in front of the suppression and timestamp processors, which are the select kernels' bias and rules).  Per row r with
 * active[r] != 0, logits[r] (f32, row pitch ld) is rewritten in place from the row's history hist[r][0 .. hist_len[r])
 * (int32 [B][hist_ld] and [B] on the device: the sequence so far, decoder prompt included; every token read from it is
 * clamped into [0, V) before it indexes the logits):
 *   upkeep -- the row's last token sits at position pos_rows[r].  hist_len[r] == pos_rows[r] + 1: the history is whole
 *   (a slot just admitted, its prefix written by the caller; a reused slot needs nothing else).  hist_len[r] ==
 *   pos_rows[r]: the row moved one position since the last call; last_tokens[r] is appended first and hist_len[r]
 *   incremented.  Any other relation, or an append that cannot be made (last_tokens NULL, hist_len[r] == hist_ld),
 *   leaves the row's logits and history untouched;
 *   repetition_penalty p != 1 -- x[t] = x[t] < 0 ? x[t] * p : x[t] / p in fp32 (round to nearest), once per distinct
 *   token t of the history however often it occurs (HF's gather, then scatter);
 *   no_repeat_ngram_size n > 0 and hist_len + 1 >= n -- x[hist[i + n - 1]] = -inf for every i in [0, hist_len - n]
 *   with hist[i .. i + n - 2] == the history's last n - 1 tokens (n == 1 bans every token of the history); after the
 *   penalty: -inf wins.
 * With p == 1 and n == 0 the call only keeps the history.  tokens, ts_state and active belong to the select kernels and
 * are not written.  One workgroup per row over the row's history, no pass over V.  Does not allocate or synchronise.
 * B in [1, 16], V >= 1, ld >= V, hist_ld in [1, 2048] (a workgroup stages its row's history in LDS),
 * repetition_penalty > 0 and finite, no_repeat_ngram_size >= 0; last_tokens may be NULL. */
int cbw_history_rules(float* logits, int B, int V, int ld, int32_t* hist, int hist_ld, int32_t* hist_len,
                      const int32_t* last_tokens, const int32_t* pos_rows, const int32_t* active,
                      float repetition_penalty, int no_repeat_ngram_size, cbw_stream_t stream);

/* ---------------------------------------------------------------- building blocks (tests, tools)
 * NHWC bf16 implicit-GEMM convolution, y = act(conv(x, w) + bias (+ res)).
 * x [N][H][W][Cin], w [Cout][KH][KW][Cin], res/y [N][Ho][Wo][Cout]; Cin % 64 == 0, Cout % 64 == 0.
 * flags: 1 ReLU, 2 GELU, 4 res is f32, 8 y is f32, 16 add res after the activation. */
int cbw_conv2d(const uint16_t* x, const uint16_t* w, const float* bias, const void* res, void* y, int N, int H, int W,
               int Cin, int Cout, int KH, int KW, int sh, int sw, int ph, int pw, int flags, cbw_stream_t stream);
/* One stage-2 identity junction of ResNet-50 as the scoring pass launches it (building block for the tests): block
 * b's expand y = relu(x . we^T + be + res) (x [N][H][W][128], we [512][128], res / y [N][H][W][512]) and, from the
 * same pass, block b + 1's reduce t1 = relu(y . wr^T + br) (wr [128][512], t1 [N][H][W][128]); both bit-identical to
 * two cbw_conv2d calls.  Packs wr per call and returns after the launch has finished. */
int cbw_conv1x1_chain(const uint16_t* x, const uint16_t* we, const float* be, const uint16_t* res, const uint16_t* wr,
                      const float* br, uint16_t* y, uint16_t* t1, int N, int H, int W, cbw_stream_t stream);
/* the fp8 tier's conv (building block, exposed for the parity tests): x e4m3 NHWC [N][H][W][Cin], w e4m3
 * [Cout][k][k][Cin], y[m][n] = act(alpha[n] * sum x.w + bias[n] (+ res[m][n] * res_scale)) stored as e4m3 of
 * y / y_scale (saturated at 448) or bf16 (out_bf16); res e4m3 [M][Cout] or NULL; pad k / 2; k 1 or 3;
 * Cin % 128 == 0, Cout % 128 == 0; relu 0/1. */
int cbw_conv2d_fp8(const uint8_t* x, const uint8_t* w, const float* alpha, const float* bias, const uint8_t* res,
                   float res_scale, void* y, float y_scale, int out_bf16, int relu, int N, int H, int W, int Cin,
                   int Cout, int k, int stride, cbw_stream_t stream);
/* test probes of the fp8 instructions: what 0..3 = one v_mfma_scale_f32_16x16x128_f8f6f4 with A [16][128] (a) and
 * B^T [16][128] (b) e4m3 loaded under operand lane map `what` -> out f32 C [16][16]; what 4 = the conversions,
 * a f32 [n] -> out e4m3 [n] (saturating) and out2 f32 [n] decoded back (n % 8 == 0). */
int cbw_fp8_probe(int what, const void* a, const void* b, void* out, void* out2, int n, cbw_stream_t stream);

/* 1x1 convolution over two K-sources (a ResNet expand conv with its shortcut conv folded in):
 * y = act([x | x2 sampled at (h*s2, w*s2)] . w + bias (+ res)); x [N][H][W][Cin], x2 [N][H2][W2][Cin2],
 * w [Cout][Cin + Cin2], res/y [N][H][W][Cout]; Cin, Cin2 % 64 == 0, Cout % 128 == 0; flags 1 ReLU. */
int cbw_conv1x1_dual(const uint16_t* x, const uint16_t* x2, const uint16_t* w, const float* bias, const void* res,
                     void* y, int N, int H, int W, int Cin, int H2, int W2, int Cin2, int s2, int Cout, int flags,
                     cbw_stream_t stream);
/* Plain bf16 GEMM on the implicit-GEMM tile kernel, y[M][N] = act(x[M][K] . w[N][K]^T + bias (+ res)), the
 * encoder's Linear layers (out-projection / fc2 run split-K: replaces the nn.Linear calls of HF
 * WhisperEncoderLayer under src/model/cb_whisper.py:100-104).  flags as cbw_conv2d.  ksplit: 0 = the factor
 * the encoder picks (cbw_gemm_splitk_factor), 1 = unsplit, S > 1 = S K-slices into fp32 partials
 * (partial: >= S * M * N floats) reduced in slice order by the split-K epilogue (deterministic). */
int cbw_gemm_splitk_factor(int M, int K, int N);
int cbw_gemm(const uint16_t* x, const uint16_t* w, const float* bias, const void* res, void* y, int M, int K, int N,
             int flags, int ksplit, float* partial, int64_t partial_floats, cbw_stream_t stream);
/* One Linear of a decode step as cbw_decoder_step* launches it (building block for the tests): the skinny GEMM over
 * 1 <= M <= 16 rows, y[m][n] = act(sum_k x[m][k] w[n][k] + bias[n] (+ res[m][n])), fp32 accumulation; asynchronous.
 *   rows: x bf16 [M] rows of pitch ldx, or (x NULL) xf f32 [M] rows of pitch ldx normalised over K in the kernel's
 *     prologue with ln_g / ln_b f32 [K] and ln_eps, exactly as cbw_layernorm_rows computes them (K <= 1280);
 *   w bf16 [N][K]; bias f32 [N] or NULL; res (or NULL) bf16, or f32 with flag 4, rows of pitch res_ld; y bf16, or f32
 *     with flag 8, rows of pitch ldy; flags as cbw_conv2d (1 ReLU, 2 GELU, 4, 8, 16 = residual after the activation);
 *   K/V append (kv_k NULL: none): N = 3 kv_D, bf16 output; columns [kv_D, 2 kv_D) of row m also go to
 *     kv_k + m * kv_ld + pos * kv_D and [2 kv_D, 3 kv_D) to kv_v likewise, pos = 0 (kv_pos NULL), kv_pos[0] (device
 *     int32, kv_pos_rows 0) or kv_pos[m] (kv_pos_rows 1).
 * K % 32 == 0, N % 4 == 0, ldx % 8 == 0, ldy, res_ld, kv_D, kv_ld % 4 == 0; x / xf, w, y 16-byte aligned.
 * Which kernel runs depends on (K, prologue or not) alone -- K 768, 1024, 1280, 3072, 4096, 5120 the VALU dot kernel,
 * every other K the MFMA kernel -- and never on M: row m of an M-row call carries the bits of a 1-row call on row m
 * alone (the guarantee cbw_decoder_step_rows gives).  cbw_linear_rows_kernel returns the name of the kernel a shape
 * runs, template arguments included (ln 0/1: with the prologue), "" for a shape cbw_linear_rows rejects. */
int cbw_linear_rows(const uint16_t* x, const float* xf, int ldx, const float* ln_g, const float* ln_b, float ln_eps,
                    const uint16_t* w, const float* bias, const void* res, int res_ld, void* y, int ldy, int M, int N,
                    int K, int flags, uint16_t* kv_k, uint16_t* kv_v, int64_t kv_ld, int kv_D, const int32_t* kv_pos,
                    int kv_pos_rows, cbw_stream_t stream);
const char* cbw_linear_rows_kernel(int M, int N, int K, int ln);
/* cbw_linear_rows over 1 <= M <= CBW_DEC_WIDE_ROWS rows, as cbw_decoder_step_wide launches it: ceil(M / 16) row groups
 * in one launch (a second grid coordinate), group g = the 16-row kernel of the shape's family on rows [16 g, 16 g + 16)
 * with x / xf, res, y, kv_k / kv_v and kv_pos moved by the group's rows.  Row m carries the bits cbw_linear_rows gives
 * it in a call over its 16-row slice.  CBW_GEMV_WIDE_ORDER=groups (read per call) makes the groups the fast grid
 * coordinate instead of the column blocks.  cbw_linear_rows_wide_kernel: the kernel's name, "" for a rejected shape. */
int cbw_linear_rows_wide(const uint16_t* x, const float* xf, int ldx, const float* ln_g, const float* ln_b, float ln_eps,
                         const uint16_t* w, const float* bias, const void* res, int res_ld, void* y, int ldy, int M,
                         int N, int K, int flags, uint16_t* kv_k, uint16_t* kv_v, int64_t kv_ld, int kv_D,
                         const int32_t* kv_pos, int kv_pos_rows, cbw_stream_t stream);
const char* cbw_linear_rows_wide_kernel(int M, int N, int K, int ln);
/* The decoder's (and encoder's) LayerNorm launch (building block for the tests): x f32 [rows][D] -> y bf16 [rows][D]
 * and / or y32 f32 [rows][D] (either may be NULL, not both) = (x - mean) * rsqrt(var + eps) * g + b, one wave per row,
 * fp32; D % 4 == 0, operands 16-byte aligned; asynchronous. */
int cbw_layernorm_rows(const float* x, const float* g, const float* b, uint16_t* y, float* y32, int rows, int D,
                       float eps, cbw_stream_t stream);
/* The encoder's self-attention (HF WhisperAttention under src/model/cb_whisper.py:100-104, non-causal, head dim
 * 64): qkv bf16 [B][T][3][H][64] with q pre-scaled by 1/8 -> out bf16 [B][T][H * 64], softmax in fp32. */
int cbw_encoder_attention(const uint16_t* qkv, uint16_t* out, int B, int T, int H, cbw_stream_t stream);
/* The decoder's attention kernels one by one (building blocks for the tests): out bf16 [B][D] (columns [0, 64 H)
 * written) = softmax_j(q_r . k_j) v_j per row r and head h, head dim 64, q pre-scaled, softmax in fp32; asynchronous.
 *   q bf16, row r at q + r * ldq (ldq = 3 D: the q slots of fused qkv rows); k, v bf16: key j, column c of K/V batch b
 *     at b * kv_bstride + j * D + c; row r reads batch r / rows_per_kv.
 *   keys: row r sees keys [0, n), n = n_keys; with n_keys_pos (device int32; paths 0, 1, 3, 4) n = min(n_keys,
 *     n_keys_pos[i] + 1), i = 0 (nk_rows 0) or the row's K/V batch (nk_rows 1), and every entry must be >= 0; with
 *     causal (path 2 only: the prefill) n = min(n_keys, r + 1).
 *   path: 0 what cbw_decoder_step* launches for self-attention and 1 for cross-attention (the step's own routing
 *     function, switches CBW_DEC_SPLIT, CBW_DEC_SELF_ONE, CBW_DEC_SELF_SPLIT read per call); 2 dec_attention_kernel, a
 *     workgroup per (row, head), n_keys <= 1536; 3 dec_attn_split_kernel + dec_attn_combine_kernel, 64-key chunks,
 *     rows_per_kv <= 8, n_keys <= 1536; 4 dec_self_attn_kernel, one launch, rows_per_kv == 1, n_keys <= 448.
 *   ws: cbw_decode_attention_ws_floats(B, H) floats (-1 on a bad shape), needed wherever the split kernel may run.
 * D, ldq, kv_bstride % 8 == 0, D >= 64 H, ldq >= 64 H, kv_bstride >= n_keys * D, B % rows_per_kv == 0; q, k, v 16-byte
 * aligned.  Every check comes before any GPU work. */
int64_t cbw_decode_attention_ws_floats(int B, int H);
int cbw_decode_attention(const uint16_t* q, int ldq, const uint16_t* k, const uint16_t* v, int64_t kv_bstride,
                         int n_keys, int rows_per_kv, const int32_t* n_keys_pos, int nk_rows, int causal, int path,
                         uint16_t* out, int B, int H, int D, float* ws, int64_t ws_floats, cbw_stream_t stream);
/* dec_cross_probs_kernel (the weights behind token-level timestamps): out f32 [T][n_keys] = softmax_j(q_r . k_j) of
 * head `head`; q rows of pitch ldq, k [n_keys][D]; 1 <= n_keys <= 1536, D % 8 == 0, 64 (head + 1) <= D and <= ldq. */
int cbw_decode_cross_probs(const uint16_t* q, int ldq, const uint16_t* k, int n_keys, int T, int D, int head,
                           float* out, cbw_stream_t stream);

/* The kernels of the exact-decision tiers (cbw_kws_rescore, cbw_kws_rescore_x3, cbw_kws_calibrate_bias) one by one
 * (building blocks for the tests): each entry checks its arguments and calls the launcher the tier itself calls, so a
 * test runs the tier's kernel at shapes the whole network never takes.  Asynchronous like the tiers; float4 operands
 * (noted per entry) must be 16-byte aligned.
 *
 * fp32 conv on the fp32-input MFMA (every conv of cbw_kws_rescore), y = act(conv(x, w) + bias (+ res)): x f32 NHWC
 * [N][H][W][Cin], w f32 [Cout][KH][KW][Cin], bias f32 [Cout] or NULL, res f32 [N][Ho][Wo][Cout] or NULL, y f32
 * [N][Ho][Wo][Cout]; any kernel size, strides and pads as cbw_conv2d; relu 0/1; Cout % 64 == 0.  Cin % 16 == 0
 * takes the float4 path (x, w aligned), any other Cin (the stem, Cin = n_layers) the element-wise one. */
int cbw_conv2d_f32(const float* x, const float* w, const float* bias, const float* res, float* y, int N, int H, int W,
                   int Cin, int Cout, int KH, int KW, int sh, int sw, int ph, int pw, int relu, cbw_stream_t stream);
/* fp32 masked similarity maps of the re-scoring tiers, out f32 NHWC [P][Tk][Tu][L]; kwd f32 [K][L][Tk][E] and
 * kwd_mask f32 [K][L][Tk] as cbw_kws_rescore; E % 4 == 0 (E == 64 with L * Tk * 260 <= 128 KB of LDS runs the
 * keyword-stationary kernel, everything else the generic one); utt, kwd aligned.
 *   B == 0, one utterance (cbw_kws_rescore): utt f32 [L][Tu][E], utt_mask f32 [L][Tu]; map p = keyword sel[p0 + p]
 *     (device int32, every index must lie in [0, K): not clamped); pair_utt, pair_kwd NULL, n_pairs ignored.
 *   B >= 1, a pair list (cbw_kws_rescore_pairs): utt f32 [B][L][Tu][E], utt_mask f32 [B][L][Tu]; map p = pair
 *     sel[p0 + p] of the n_pairs pairs (pair_utt[q], pair_kwd[q]) (device int32 [n_pairs]); both NULL = q = b * K + k
 *     and n_pairs must be B * K.  Indices are clamped into range on the device.
 * 1 <= P <= 65535. */
int cbw_sim_maps_f32(const float* utt, const float* utt_mask, int B, const float* kwd, const float* kwd_mask, int K,
                     int L, int Tk, int Tu, int E, const int32_t* pair_utt, const int32_t* pair_kwd, int n_pairs,
                     const int32_t* sel, int p0, int P, float* out, cbw_stream_t stream);
/* MaxPool2d(3, 2, 1) of the fp32 tiers: x f32 NHWC [N][H][W][C] -> y f32 [N][(H - 1) / 2 + 1][(W - 1) / 2 + 1][C]. */
int cbw_maxpool_f32(const float* x, float* y, int N, int H, int W, int C, cbw_stream_t stream);
/* AdaptiveAvgPool(1) + Linear(C -> 2) of the fp32 tiers: x f32 [P][HW][C], w f32 [2][C], b f32 [2];
 * logits[sel[p0 + p]] (f32 rows of 2) <- the logits of x[p]; rows sel does not name are not written. */
int cbw_pool_fc_f32(const float* x, const float* w, const float* b, const int32_t* sel, int p0, int P, float* logits,
                    int HW, int C, cbw_stream_t stream);
/* The compensated tier's activation split: x f32 [M][C] -> y bf16 [M][2C] = [hi | lo], hi = bf16(x) (round to nearest
 * even), lo = bf16(x - hi); C % 4 == 0, x and y aligned. */
int cbw_split3_f32(const float* x, uint16_t* y, int64_t M, int C, cbw_stream_t stream);
/* Per-channel sums of x f32 [M][C] (the statistics of cbw_kws_calibrate_bias): part f32 [G][C], part_bytes >=
 * cbw_channel_sum_workspace_bytes(C) = G * C * 4; workgroup g ADDS the sum of its rows to part[g][c], so the channel
 * sums are the column sums of a part the caller zeroed before the first call. */
int64_t cbw_channel_sum_workspace_bytes(int C);
int cbw_channel_sum_f32(const float* x, int64_t M, int C, float* part, int64_t part_bytes, cbw_stream_t stream);
/* One conv of the compensated tier (cbw_kws_rescore_x3) over caller-built split operands, on the bf16 MFMA kernels
 * with fp32 accumulation: x bf16 [N][H][W][2C] = [x_hi | x_lo], read as the K-segments [x_hi | x_hi | x_lo] against
 * w bf16 [Cout][k][k][3C] = [w_hi | w_lo | w_hi] per tap (w_hi = bf16(w), w_lo = bf16(w - w_hi)), so the sum is
 * x_hi.w_hi + x_hi.w_lo + x_lo.w_hi; v = act(sum + bias (+ res)), bias f32 [Cout].  res (or NULL): f32 [M][Cout]
 * (res_split 0) or bf16 [M][2 Cout] = [hi | lo], added as hi + lo (res_split 1).  out_split 0: y f32 [M][Cout] = v,
 * y32 NULL; out_split 1: y bf16 [M][2 Cout] = [bf16(v) | bf16(v - bf16(v))] and y32 (optional) f32 [M][Cout] = v.
 * k 1 or 3 with pad k / 2, stride 1 or 2, relu 0/1; C % 64 == 0, Cout % 64 == 0. */
int cbw_conv2d_x3(const uint16_t* x, const uint16_t* w, const float* bias, const void* res, int res_split, void* y,
                  float* y32, int out_split, int N, int H, int W, int C, int Cout, int k, int stride, int relu,
                  cbw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CBW_H */
