// Whisper front end and encoder kernels for gfx950: log-mel spectrogram,
// LayerNorm, and non-causal flash attention (hd = 64).
//
// Reference semantics: HF WhisperFeatureExtractor (called at src/utils.py:186-187,
// src/data/dataset.py:332-339) and HF WhisperEncoder (called at
// src/model/cb_whisper.py:100-104, src/utils.py:188-192); see oracle/mel.py and
// oracle/encoder.py for the restated algorithms these kernels are checked against.
#include <algorithm>
#include <cfloat>

#include "cbw_common.h"
#include "cbw_kernels.h"

namespace {

constexpr int N_FFT = 400, HOP = 160, N_SAMPLES = 480000, N_FRAMES = 3000, N_FREQ = 201;

// ---------------------------------------------------------------- log-mel
// one block per frame: windowed frame -> direct 400-point real DFT (exact twiddle
// table) -> |X|^2 -> mel projection -> log10(max(., 1e-10)).  Input is the raw
// clip; zero-pad/truncate to 30 s and the reflect padding of torch.stft(center=True)
// are applied on the fly.
// L_pad: the length the reflect padding of torch.stft(center=True) mirrors at (480000 for the 30 s window,
// the audio length for long-form features); frames: output frames = the row pitch of logmel
__global__ __launch_bounds__(256) void mel_frames_kernel(const float* __restrict__ pcm, int n_samples,
                                                         const float* __restrict__ filters,
                                                         const float* __restrict__ twiddle,
                                                         float* __restrict__ logmel, int n_mel, int L_pad, int frames) {
    __shared__ float xw[N_FFT];
    __shared__ float tw[2 * N_FFT];
    __shared__ float pw[N_FREQ + 7];
    const int t = blockIdx.x;
    for (int i = threadIdx.x; i < 2 * N_FFT; i += blockDim.x) tw[i] = twiddle[i];
    for (int n = threadIdx.x; n < N_FFT; n += blockDim.x) {
        int j = t * HOP + n - N_FFT / 2;
        if (j < 0) j = -j;
        if (j >= L_pad) j = 2 * (L_pad - 1) - j;
        const float v = j < n_samples ? pcm[j] : 0.f;
        const float win = 0.5f - 0.5f * tw[n];    // cos(2*pi*n/400) = twiddle[n]
        xw[n] = v * win;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < N_FREQ; f += blockDim.x) {
        float re = 0.f, im = 0.f;
        int idx = 0;
        for (int n = 0; n < N_FFT; ++n) {
            re = fmaf(xw[n], tw[idx], re);
            im = fmaf(xw[n], tw[N_FFT + idx], im);
            idx += f;
            if (idx >= N_FFT) idx -= N_FFT;
        }
        pw[f] = re * re + im * im;
    }
    __syncthreads();
    for (int m = threadIdx.x; m < n_mel; m += blockDim.x) {
        float s = 0.f;
        for (int f = 0; f < N_FREQ; ++f) s = fmaf(filters[f * n_mel + m], pw[f], s);
        logmel[(int64_t)m * frames + t] = log10f(fmaxf(s, 1e-10f));
    }
}

// block b writes the max of its grid-strided share to out[b] (mel_finish_kernel reduces the gridDim.x partials)
__global__ __launch_bounds__(1024) void max_reduce_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ out) {
    __shared__ float red[16];
    float m = -INFINITY;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        m = fmaxf(m, x[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = red[0];
        for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = fmaxf(r, red[i]);
        out[blockIdx.x] = r;
    }
}

// (max(x, gmax - 8) + 4) / 4, in place, + time-major bf16 copy [3000][cpad] for the encoder
__global__ void mel_finish_kernel(float* __restrict__ logmel, int n_mel, const float* __restrict__ gmax, int n_part,
                                  bf16* __restrict__ packed, int cpad, int frames) {
    float mx = gmax[0];
    for (int i = 1; i < n_part; ++i) mx = fmaxf(mx, gmax[i]);
    const float floor_v = mx - 8.0f;
    const int C = packed ? cpad : n_mel;
    const int64_t total = (int64_t)frames * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int64_t t = i / C;
        float v = 0.f;
        if (c < n_mel) {
            v = (fmaxf(logmel[(int64_t)c * frames + t], floor_v) + 4.0f) * 0.25f;
            logmel[(int64_t)c * frames + t] = v;
        }
        if (packed) packed[i] = f2bf(v);
    }
}

// ---------------------------------------------------------------- resample + downmix (in front of the log-mel)
// torchaudio.functional.resample(torch.mean(waveform, dim=0), orig, new) with the sinc_interp_hann defaults, as the
// reference calls it (src/utils.py:179-184, src/efficient_kws/dataset.py:472-483): a polyphase filter of n phases x T
// taps (o = orig / gcd, n = new / gcd, T = 2 width + o), y[f n + j] = sum_k xpad[f o + k] kernel[j][k] with xpad = x
// behind `width` zeros.  The coefficient table is the runtime's (float64 on the host, rounded once).
//
// sample i of the downmixed input: the mean over the C rows of pcm [C][len] (the channel sum in channel order, one
// division), 0 outside [0, len).  The index is clamped so that the load stays inside the buffer and the value is
// selected afterwards: no padded copy of the input exists.
__device__ __forceinline__ float downmix_at(const float* __restrict__ pcm, int C, int64_t len, int64_t i) {
    const int64_t ic = i < 0 ? 0 : (i >= len ? len - 1 : i);
    float s = pcm[ic];
    for (int c = 1; c < C; ++c) s += pcm[(int64_t)c * len + ic];
    if (C > 1) s /= (float)C;
    return (i >= 0 && i < len) ? s : 0.f;
}

// one thread per output sample; tab is phase-minor, tab[k * n + j] = kernel[j][k], so that the 256 consecutive
// outputs of a block (consecutive phases) read consecutive coefficients: coalesced from global memory, one bank each
// from LDS.  LDS: the whole table staged per block (the launcher picks it where n * T floats fit).  One fmaf per tap,
// k ascending from 0, in either variant: an output's bits depend on neither the variant nor the launch shape.
template <bool LDS>
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ pcm, int C, int64_t len,
                                                       const float* __restrict__ tab, int o, int n, int width, int T,
                                                       float* __restrict__ out, int64_t out_len) {
    extern __shared__ float coef[];
    if (LDS) {
        for (int i = threadIdx.x; i < n * T; i += blockDim.x) coef[i] = tab[i];
        __syncthreads();
    }
    const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (m >= out_len) return;
    const int64_t f = m / n;
    const int j = (int)(m - f * n);
    const int64_t i0 = f * o - width;
    const float* __restrict__ cf = (LDS ? coef : tab) + j;
    float acc = 0.f;
    for (int k = 0; k < T; ++k) acc = fmaf(downmix_at(pcm, C, len, i0 + k), cf[(int64_t)k * n], acc);
    out[m] = acc;
}

// orig == new with C > 1: the downmix alone
__global__ __launch_bounds__(256) void downmix_kernel(const float* __restrict__ pcm, int C, int64_t len,
                                                      float* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < len) out[i] = downmix_at(pcm, C, len, i);
}

// ---------------------------------------------------------------- LayerNorm (one wave per row)
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        const float* __restrict__ b, bf16* __restrict__ y,
                                                        float* __restrict__ y32, int rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (int64_t)row * D;
    float s = 0.f;
    for (int i = lane * 4; i < D; i += 256) {
        const f32x4 v = *(const f32x4*)(xr + i);
        s += v[0] + v[1] + v[2] + v[3];
    }
    const float mean = wave_sum(s) / D;
    float ss = 0.f;
    for (int i = lane * 4; i < D; i += 256) {
        const f32x4 v = *(const f32x4*)(xr + i);
#pragma unroll
        for (int q = 0; q < 4; ++q) ss += (v[q] - mean) * (v[q] - mean);
    }
    const float rstd = rsqrtf(wave_sum(ss) / D + eps);
    for (int i = lane * 4; i < D; i += 256) {
        const f32x4 v = *(const f32x4*)(xr + i);
        const f32x4 gg = *(const f32x4*)(g + i), bb = *(const f32x4*)(b + i);
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = (v[q] - mean) * rstd * gg[q] + bb[q];
        if (y) {
            bf16x4 ob;
#pragma unroll
            for (int q = 0; q < 4; ++q) ob[q] = f2bf(o[q]);
            *(bf16x4*)(y + (int64_t)row * D + i) = ob;
        }
        if (y32) *(f32x4*)(y32 + (int64_t)row * D + i) = o;
    }
}

// ---------------------------------------------------------------- attention
// Non-causal softmax(Q K^T) V with Q pre-scaled by hd^-1/2 (folded into q_proj).
// qkv: bf16 [B][T][3][H][64]; out: bf16 [B][T][H*64].
// Block = 4 waves x 16 queries of one (b, h); 64-key tiles staged in LDS.
// S^T = K Q^T puts the query on the MFMA lane (lane & 15) so the online-softmax
// state is lane-local; P^T feeds O^T = V^T P^T directly from the accumulator
// with a permuted key order that the V^T operand reads in the same order.
constexpr int AT_KT = 64;
__global__ __launch_bounds__(256) void attention_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ out, int T,
                                                        int H) {
    constexpr int HD = 64;
    constexpr int VT_PITCH = 136;    // bytes per d-row of V^T (64 keys * 2 B + 8 pad)
    __shared__ __attribute__((aligned(16))) char Ks[AT_KT * 128];
    __shared__ __attribute__((aligned(16))) char Vt[HD * VT_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int bh = blockIdx.y;
    const int b = bh / H, h = bh % H;
    const int D = H * HD;
    const int64_t row_stride = 3 * (int64_t)D;
    const bf16* base = qkv + (int64_t)b * T * row_stride;
    const int q = blockIdx.x * 64 + wid * 16 + fr;
    const int qld = min(q, T - 1);
    bf16x8 qf[2];
    qf[0] = *(const bf16x8*)(base + qld * row_stride + h * HD + fq * 8);
    qf[1] = *(const bf16x8*)(base + qld * row_stride + h * HD + 32 + fq * 8);

    f32x4 o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    for (int k0 = 0; k0 < T; k0 += AT_KT) {
        __syncthreads();
        // stage K (swizzled rows) and V^T
        for (int c = tid; c < AT_KT * 8; c += 256) {
            const int key = c >> 3, ch = c & 7;
            const int kg = k0 + key;
            bf16x8 kv, vv;
            if (kg < T) {
                kv = *(const bf16x8*)(base + kg * row_stride + D + h * HD + ch * 8);
                vv = *(const bf16x8*)(base + kg * row_stride + 2 * D + h * HD + ch * 8);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) { kv[j] = f2bf(0.f); vv[j] = f2bf(0.f); }
            }
            *(bf16x8*)(Ks + key * 128 + ((ch ^ ((key >> 1) & 7)) * 16)) = kv;
#pragma unroll
            for (int j = 0; j < 8; ++j) *(bf16*)(Vt + (ch * 8 + j) * VT_PITCH + key * 2) = vv[j];
        }
        __syncthreads();
        // S^T tile: 4 key-subtiles x 16 queries
        f32x4 s[4];
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            s[st] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int key = st * 16 + fr;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int ch = ks * 4 + fq;
                const bf16x8 kf = *(const bf16x8*)(Ks + key * 128 + ((ch ^ ((key >> 1) & 7)) * 16));
                s[st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s[st], 0, 0, 0);
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kg = k0 + st * 16 + fq * 4 + i;
                if (kg >= T) s[st][i] = -INFINITY;
                mx = fmaxf(mx, s[st][i]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __expf(m_run - m_new);
        float rs = 0.f;
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s[st][i] = __expf(s[st][i] - m_new);
                rs += s[st][i];
            }
        rs += __shfl_xor(rs, 16, 64);
        rs += __shfl_xor(rs, 32, 64);
        l_run = l_run * alpha + rs;
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int i = 0; i < 4; ++i) o[dt][i] *= alpha;
        // O^T += V^T P^T ; k-step ks covers keys 32ks + {4fq..4fq+3, 16+4fq..16+4fq+3}
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 pf;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pf[j] = f2bf(s[2 * ks][j]);
                pf[4 + j] = f2bf(s[2 * ks + 1][j]);
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int d = dt * 16 + fr;
                const char* vr = Vt + d * VT_PITCH + (ks * 32 + fq * 4) * 2;
                const bf16x4 v0 = *(const bf16x4*)vr;
                const bf16x4 v1 = *(const bf16x4*)(vr + 32);
                bf16x8 vf;
#pragma unroll
                for (int j = 0; j < 4; ++j) { vf[j] = v0[j]; vf[4 + j] = v1[j]; }
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
            }
        }
    }
    if (q >= T) return;
    const float inv = 1.0f / l_run;
    bf16* orow = out + ((int64_t)b * T + q) * D + h * HD;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        bf16x4 ov;
#pragma unroll
        for (int i = 0; i < 4; ++i) ov[i] = f2bf(o[dt][i] * inv);
        *(bf16x4*)(orow + dt * 16 + fq * 4) = ov;
    }
}

// ---------------------------------------------------------------- decoder step kernels
// h[r] = E[token[r]] + P[pos]  (fp32 residual stream)
__global__ void dec_embed_kernel(const int* __restrict__ tok, const bf16* __restrict__ E, const float* __restrict__ P,
                                 int pos, int pos_inc, float* __restrict__ h, int D, const int* __restrict__ pos_dev,
                                 int pos_rows) {
    const int r = blockIdx.x;
    const int t = tok[r];
    if (pos_dev) pos = pos_dev[pos_rows ? r : 0];   // pos_rows: one position per row (several windows in one step)
    const int pr = pos + pos_inc * r;   // decode step: every row at pos; prefill: row r is token r at pos + r
    for (int d = threadIdx.x; d < D; d += blockDim.x) h[(int64_t)r * D + d] = bf2f(E[(int64_t)t * D + d]) + P[(int64_t)pr * D + d];
}

// prefill: k, v of prefix token t (fused qkv row t) -> position t of every beam row's self-attention cache
__global__ void dec_kv_prefill_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ kc, bf16* __restrict__ vc, int D,
                                      int maxlen) {
    const int t = blockIdx.x, b = blockIdx.y;
    for (int d = threadIdx.x * 8; d < D; d += blockDim.x * 8) {
        *(bf16x8*)(kc + ((int64_t)b * maxlen + t) * D + d) = *(const bf16x8*)(qkv + (int64_t)t * 3 * D + D + d);
        *(bf16x8*)(vc + ((int64_t)b * maxlen + t) * D + d) = *(const bf16x8*)(qkv + (int64_t)t * 3 * D + 2 * D + d);
    }
}

// k, v of the fused qkv rows -> self-attention cache at position pos
__global__ void dec_kv_append_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ kc, bf16* __restrict__ vc, int D,
                                     int maxlen, int pos) {
    const int r = blockIdx.x;
    for (int d = threadIdx.x * 8; d < D; d += blockDim.x * 8) {
        *(bf16x8*)(kc + ((int64_t)r * maxlen + pos) * D + d) = *(const bf16x8*)(qkv + (int64_t)r * 3 * D + D + d);
        *(bf16x8*)(vc + ((int64_t)r * maxlen + pos) * D + d) = *(const bf16x8*)(qkv + (int64_t)r * 3 * D + 2 * D + d);
    }
}

// fma8: acc[e] += p * v[e] over the 8 dims of one 16-byte V load (the P.V accumulate of the decode-attention kernels)
CBW_DEV void fma8(float p, bf16x8 v, float (&acc)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = fmaf(p, bf2f(v[e]), acc[e]);
}

// dec_row_softmax: the softmax statistics of query row r, head h against n_keys keys (key j's 64 dims of the head at
// kc + j * D + h * 64), by a block of 256 threads.  The query is staged into qs[64], thread t scores keys t, t + 256, ... (one fmaf chain
// over the 64 dims), the block max meets in red[0..3] and the block sum in red[4..7].  Leaves the unnormalised
// exponentials in ps[0..n_keys) and returns 1 / sum; ps[] is visible to the whole block on return.
CBW_DEV float dec_row_softmax(const bf16* q, int ldq, int r, int h, const bf16* kc, int n_keys, int D, float* qs,
                              float* ps, float* red) {
    const int tid = threadIdx.x;
    if (tid < 64) qs[tid] = bf2f(q[(int64_t)r * ldq + h * 64 + tid]);
    __syncthreads();
    const bf16* kb = kc + h * 64;
    float mx = -INFINITY;
    for (int j = tid; j < n_keys; j += 256) {
        const bf16* kr = kb + (int64_t)j * D;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 64; c += 8) {
            const bf16x8 kv = *(const bf16x8*)(kr + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) s = fmaf(qs[c + e], bf2f(kv[e]), s);
        }
        ps[j] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int j = tid; j < n_keys; j += 256) {
        const float e = __expf(ps[j] - mx);
        ps[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red[4 + (tid >> 6)] = sum;
    __syncthreads();
    return 1.0f / (red[4] + red[5] + red[6] + red[7]);
}

// one query row per (row, head) against n_keys cached keys (decode step); q pre-scaled.
// K/V element (key j, dim c) of kv batch b at kv + b*kv_bstride + j*D + c; row r reads kv batch r / rows_per_kv.
constexpr int DA_MAXK = 1536;
__global__ __launch_bounds__(256) void dec_attention_kernel(const bf16* __restrict__ q, int ldq,
                                                            const bf16* __restrict__ kc, const bf16* __restrict__ vc,
                                                            int64_t kv_bstride, int n_keys_all, int rows_per_kv,
                                                            bf16* __restrict__ out, int D, int causal) {
    __shared__ float qs[64];
    __shared__ float ps[DA_MAXK];
    __shared__ float red[8];
    __shared__ float pv[32][65];
    const int r = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    const int b = r / rows_per_kv;
    // causal (prefill): query row r is prefix token r and sees keys 0..r
    const int n_keys = causal ? min(n_keys_all, r + 1) : n_keys_all;
    const float inv = dec_row_softmax(q, ldq, r, h, kc + b * kv_bstride, n_keys, D, qs, ps, red);
    const bf16* vb = vc + b * kv_bstride + h * 64;
    // P.V: thread = 8 dims (one 16-byte load per key) x every 32nd key, four keys in flight per step;
    // the 32 key groups meet in LDS (fixed order)
    const int dg = tid & 7, kg = tid >> 3;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bf16* vd = vb + dg * 8;
    int j = kg;
    for (; j + 96 < n_keys; j += 128) {
        bf16x8 v4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v4[u] = *(const bf16x8*)(vd + (int64_t)(j + 32 * u) * D);
#pragma unroll
        for (int u = 0; u < 4; ++u) fma8(ps[j + 32 * u], v4[u], acc);
    }
    for (; j < n_keys; j += 32) {
        const bf16x8 vv = *(const bf16x8*)(vd + (int64_t)j * D);
        fma8(ps[j], vv, acc);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) pv[kg][dg * 8 + e] = acc[e];
    __syncthreads();
    if (tid < 64) {
        float o = 0.f;
        for (int k = 0; k < 32; ++k) o += pv[k][tid];
        out[(int64_t)r * D + h * 64 + tid] = f2bf(o * inv);
    }
}

// Cross-attention probabilities of one head (token-level timestamps: the alignment heads' weights that
// transformers' _extract_token_timestamps reads from generate's cross_attentions): row r = softmax_j(q_r . k_j)
// over the n_keys encoder frames, dec_attention_kernel's scores, max and exponentials (dec_row_softmax); out f32
// [T][n_keys].
__global__ __launch_bounds__(256) void dec_cross_probs_kernel(const bf16* __restrict__ q, int ldq,
                                                              const bf16* __restrict__ kc, int n_keys, int D, int h,
                                                              float* __restrict__ out) {
    __shared__ float qs[64];
    __shared__ float ps[DA_MAXK];
    __shared__ float red[8];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float inv = dec_row_softmax(q, ldq, r, h, kc, n_keys, D, qs, ps, red);
    for (int j = tid; j < n_keys; j += 256) out[(int64_t)r * n_keys + j] = ps[j] * inv;
}

// ---------------------------------------------------------------- token-level timestamps behind the probabilities
// transformers' _extract_token_timestamps after the weights (pba_whisper.py:333-336, 425-442; the host statement is
// cbw/token_timestamps.py): the alignment matrix and its dynamic time warping.
//
// Alignment matrix: matrix[t][f] = -(1/n) sum_h median_k z_h[t][reflect(f + k - W/2)], z_h[t][f] = (w - mean) / std
// over the T positions [t0, t0 + T) of head h at frame f (population std).  One block per tile of 32 - 2 (W / 2) frames;
// thread = (row group g of 32, column lane of 32): lane l holds frame reflect(f0 - W/2 + l), so that a half wave owns
// a tile with its halo and the W neighbours of a median come by lane shuffles.  Per head: the mean in float64 (32
// partial sums over the rows g, g + 32, ..., added in g order), the variance in float64 in a second pass, z with one
// rounding to fp32, the median by exact selection, and the head sum in fp32 kept in the output itself: element (t, f)
// is read and written by the same thread for h = 0, 1, ..., n - 1, the last one dividing by n and negating.
// *degenerate |= 1 where a variance of a used frame is zero or not finite (the host path gives NaN there).
constexpr int AM_G = 32;   // row groups of a block (1024 threads)

template <int W>
__device__ __forceinline__ float median_of(float (&v)[W]) {
    // bubble network, unrolled: after pass p the p + 1 largest stand at the end; W / 2 + 1 passes fix v[W / 2]
#pragma unroll
    for (int p = 0; p <= W / 2; ++p)
#pragma unroll
        for (int q = 0; q + 1 < W - p; ++q) {
            const float lo = fminf(v[q], v[q + 1]), hi = fmaxf(v[q], v[q + 1]);
            v[q] = lo;
            v[q + 1] = hi;
        }
    return v[W / 2];
}

// the block of frame tile `tile` of one window (the kernels below: one window, or a batch with the window as grid.y)
template <int W>
__device__ __forceinline__ void align_matrix_tile(const float* __restrict__ probs, int n, int T_all, int t0, int T,
                                                  int F, float* __restrict__ matrix, int* __restrict__ degenerate,
                                                  int tile, double (&part)[AM_G][33]) {
    constexpr int P = W / 2, FT = 32 - 2 * P;
    const int lane = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int c = tile * FT - P + lane;   // the lane's column before the reflection
    int fr = c < 0 ? -c : c;
    if (fr >= F) fr = 2 * (F - 1) - fr;
    fr = min(max(fr, 0), F - 1);                // lanes behind the last halo: some frame, never stored
    const bool inner = lane >= P && lane < 32 - P && c < F;
    for (int h = 0; h < n; ++h) {
        const float* __restrict__ w = probs + ((int64_t)h * T_all + t0) * 1500 + fr;
        double s = 0.0;
        for (int t = g; t < T; t += AM_G) s += (double)w[(int64_t)t * 1500];
        part[g][lane] = s;
        __syncthreads();
        double mean = 0.0;
        for (int q = 0; q < AM_G; ++q) mean += part[q][lane];
        mean /= (double)T;
        __syncthreads();
        s = 0.0;
        for (int t = g; t < T; t += AM_G) {
            const double d = (double)w[(int64_t)t * 1500] - mean;
            s += d * d;
        }
        part[g][lane] = s;
        __syncthreads();
        double var = 0.0;
        for (int q = 0; q < AM_G; ++q) var += part[q][lane];
        var /= (double)T;
        __syncthreads();
        if (g == 0 && !(var > 0.0 && var <= DBL_MAX)) atomicOr(degenerate, 1);
        const double sd = sqrt(var);
        for (int tb = 0; tb < T; tb += AM_G) {   // uniform trip count: every lane takes part in the shuffles
            const int t = tb + g, tc = min(t, T - 1);
            const float z = (float)(((double)w[(int64_t)tc * 1500] - mean) / sd);
            float v[W];
#pragma unroll
            for (int k = 0; k < W; ++k) v[k] = W == 1 ? z : __shfl(z, (lane + k - P) & 31, 32);
            const float med = median_of<W>(v);
            if (inner && t < T) {
                float* o = matrix + (int64_t)t * F + c;
                float acc = h ? *o + med : med;
                if (h == n - 1) acc = -(acc / (float)n);
                *o = acc;
            }
        }
    }
}

template <int W>
__global__ __launch_bounds__(32 * AM_G) void align_matrix_kernel(const float* __restrict__ probs, int n, int T_all,
                                                                 int t0, int T, int F, float* __restrict__ matrix,
                                                                 int* __restrict__ degenerate) {
    __shared__ double part[AM_G][33];
    align_matrix_tile<W>(probs, n, T_all, t0, T, F, matrix, degenerate, blockIdx.x, part);
}

// N windows in one launch: grid = (the frame tiles of the window with the most, N), the table by value in the kernel
// arguments.  A block beyond its window's tiles leaves before any barrier; a window too short to filter (F <= W / 2)
// takes the W = 1 tile, as cbw_align_matrix_launch chooses for it.  degenerate: one flag per window.
template <int W>
__global__ __launch_bounds__(32 * AM_G) void align_matrix_batch_kernel(const cbw_ts_batch b, int n,
                                                                       int* __restrict__ degenerate) {
    __shared__ double part[AM_G][33];
    const cbw_ts_win& w = b.w[blockIdx.y];
    const int tile = blockIdx.x;
    if (W > 1 && w.F <= W / 2) {
        if (tile * 32 >= w.F) return;
        align_matrix_tile<1>(w.probs, n, w.T_all, w.t0, w.T, w.F, w.matrix, degenerate + blockIdx.y, tile, part);
    } else {
        if (tile * (32 - 2 * (W / 2)) >= w.F) return;
        align_matrix_tile<W>(w.probs, n, w.T_all, w.t0, w.T, w.F, w.matrix, degenerate + blockIdx.y, tile, part);
    }
}

// Dynamic time warping of matrix f32 [T][F] with cbw_dtw's arithmetic (fp32 tables, +inf borders around cost 0,
// strict comparisons: the diagonal, then the row above, else the column to the left; cost = min + matrix as one fp32
// add): an anti-diagonal wavefront.  One workgroup, thread i = text row i; at step d it computes cell (i, d - i) from
// its own previous cost (a register), the cost thread i - 1 posted at step d - 1 (LDS, double-buffered: one barrier per
// step) and the one it read from there a step earlier.  The steps go in blocks of 16: a thread loads the 16 matrix
// entries of the next block (contiguous in its row) while it works on the current one, and packs the 16 trace entries
// (2 bits each) of a block into one word, trace[block][i].  Then thread 0 walks the trace back from (T, F), holding
// the current word in a register, and writes first_frame[i] = the time index at which the path enters row i and, if
// asked, the path (backwards; the block reverses it in place afterwards).
constexpr int DTW_MAX_T = 1024;
__device__ __forceinline__ void dtw_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// the 16 entries m[i][jb .. jb + 15] of a block of steps: one clamped load each and no branch, so that the loads of
// the next block stay counted in flight behind those of the current one (entries outside [0, F) are never used)
__device__ __forceinline__ void dtw_load16(const float* __restrict__ mr, int jb, int F, float (&buf)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) buf[k] = mr[min(max(jb + k, 0), F - 1)];
}

// the 16 steps of block b for text row i: returns the packed trace word
__device__ __forceinline__ uint32_t dtw_block16(const float (&mv)[16], int b, int i, bool row, int F,
                                                float (&sh)[2][DTW_MAX_T], float& left, float& diag) {
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {   // step d = 16 b + k: d & 1 == k & 1
        const int j = 16 * b + k - i;
        if (row && j >= 0 && j < F) {
            const float up = i ? sh[(k & 1) ^ 1][i - 1] : INFINITY;
            float c;
            uint32_t t;
            if (diag < up && diag < left) c = diag, t = 0;
            else if (up < diag && up < left) c = up, t = 1;
            else c = left, t = 2;
            c += mv[k];
            sh[k & 1][i] = c;
            left = c;
            diag = up;
            word |= t << (2 * k);
        }
        dtw_lds_barrier();
    }
    return word;
}

// the kernel: once for one window, once with the window as the grid's coordinate
#define DTW_BATCH 0
#include "dtw_kernel.inc"
#undef DTW_BATCH
#define DTW_BATCH 1
#include "dtw_kernel.inc"
#undef DTW_BATCH

// Split-key decode attention (flash-decoding): workgroup = (key chunk of DS_CHUNK keys, head, kv batch)
// serving ALL the R query rows that share the kv batch (the beams of a window against its cross K/V: K/V
// read once, not once per beam).  With one chunk the workgroup writes the output; otherwise each writes
// its chunk's unnormalised P.V and (max, sum) per query row and dec_attn_combine_kernel merges the S
// partials in chunk order (deterministic).  (A last-arriver combine inside this kernel needs an
// agent-scope release per workgroup -- an L2 writeback on gfx950 -- and measured 1.7x slower than the
// second launch.)
// R <= RMAX rows per kv batch (1 for self-attention, beams for cross-attention); q pre-scaled.
constexpr int DS_CHUNK = 64;
constexpr int DS_MAXS = 24;   // 1536 keys

// dot16_quad: q . k over the 64 dims of a head by the four lanes of a key, 16 dims each: the lane's two 8-dim halves
// in one fmaf chain (a[0], b[0], a[1], b[1], ...), then the four lanes' sums by two lane exchanges; every lane of the
// four returns the dot product.  The query halves are floats in LDS (split kernel) or bf16 in registers (self kernel).
CBW_DEV float dot16_elem(float v) { return v; }
CBW_DEV float dot16_elem(bf16 v) { return bf2f(v); }
template <class Q>
CBW_DEV float dot16_quad(const Q& qa, const Q& qb, bf16x8 ka, bf16x8 kb) {
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        d = fmaf(dot16_elem(qa[e]), bf2f(ka[e]), d);
        d = fmaf(dot16_elem(qb[e]), bf2f(kb[e]), d);
    }
    d += xor_lane<1>(d);
    d += xor_lane<2>(d);
    return d;
}

template <int RMAX>
__global__ __launch_bounds__(256) void dec_attn_split_kernel(const bf16* __restrict__ q, int ldq,
                                                             const bf16* __restrict__ kc, const bf16* __restrict__ vc,
                                                             int64_t kv_bstride, int n_keys, int R,
                                                             bf16* __restrict__ out, int D, float* __restrict__ part,
                                                             const int* __restrict__ n_keys_pos, int nk_rows) {
    __shared__ float qs[RMAX][64];
    __shared__ float ps[RMAX][DS_CHUNK];
    __shared__ float st[2][RMAX];
    constexpr int NQ = 8;   // partial P.V sums per (row, dim): 4 waves x 2 half-waves
    __shared__ float red[NQ][RMAX][64];
    const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z, S = gridDim.x, H = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = b * R;
    const int j0 = s * DS_CHUNK;
    const bf16* kb = kc + b * kv_bstride + (int64_t)j0 * D + h * 64;
    const bf16* vb = vc + b * kv_bstride + (int64_t)j0 * D + h * 64;
    if (n_keys_pos) n_keys = min(n_keys, n_keys_pos[nk_rows ? b : 0] + 1);   // nk_rows: a key count per kv batch
    const int nk = min(DS_CHUNK, n_keys - j0);
    if (nk <= 0) {   // a chunk past the live keys (device-side count): a neutral partial (m = -inf, l = 0, o = 0)
        float* pp = part + ((int64_t)(b * H + h) * S + s) * (RMAX * 66);
        for (int i = tid; i < R * 64; i += 256) pp[i] = 0.f;
        if (tid < R) { pp[RMAX * 64 + tid] = -INFINITY; pp[RMAX * 65 + tid] = 0.f; }
        return;
    }
    // every global load of the chunk in flight before the first wait: the R query rows first (their LDS
    // staging then waits only for them), then K for the scores and V for P.V
    const int j = tid >> 2, p = tid & 3;          // scores: 4 threads per key, 16 dims each
    const int dg = tid & 7, kg = tid >> 3;        // P.V: 8 dims x keys kg, kg + 32
    static_assert(RMAX * 64 <= 2 * 256, "query staging: two elements per thread");
    // unconditional loads of clamped elements (a conditionally loaded value made the compiler wait for it at the
    // branch join: the two query loads and then K / V went out one round trip after another); rows past nk are
    // read as row nk - 1 and carry score -inf / weight p = 0 below (0 x a finite value adds nothing)
    const int qi0 = min(tid, R * 64 - 1), qi1 = min(tid + 256, R * 64 - 1);
    const unsigned short qv0 = ((const unsigned short*)q)[(int64_t)(r0 + (qi0 >> 6)) * ldq + h * 64 + (qi0 & 63)];
    const unsigned short qv1 = ((const unsigned short*)q)[(int64_t)(r0 + (qi1 >> 6)) * ldq + h * 64 + (qi1 & 63)];
    const int jc = min(j, nk - 1), kg0 = min(kg, nk - 1), kg1 = min(kg + 32, nk - 1);
    const bf16x8 k0 = *(const bf16x8*)(kb + (int64_t)jc * D + p * 16);
    const bf16x8 k1 = *(const bf16x8*)(kb + (int64_t)jc * D + p * 16 + 8);
    const bf16x8 v0 = *(const bf16x8*)(vb + (int64_t)kg0 * D + dg * 8);
    const bf16x8 v1 = *(const bf16x8*)(vb + (int64_t)kg1 * D + dg * 8);
    if (tid < R * 64) qs[tid >> 6][tid & 63] = bf2f(__builtin_bit_cast(bf16, qv0));
    if (tid + 256 < R * 64) qs[(tid + 256) >> 6][tid & 63] = bf2f(__builtin_bit_cast(bf16, qv1));
    __syncthreads();
    {
#pragma unroll
        for (int i = 0; i < RMAX; ++i) {
            if (i < R) {
                const float d = dot16_quad(qs[i] + p * 16, qs[i] + p * 16 + 8, k0, k1);
                if (p == 0) ps[i][j] = j < nk ? d : -INFINITY;
            }
        }
    }
    __syncthreads();
    // chunk softmax statistics: wave w takes rows w, w + 4, ...
    for (int i = w; i < R; i += 4) {
        const float v = ps[i][lane];
        const float m = wave_max_x(v);
        const float e = lane < nk ? __expf(v - m) : 0.f;
        ps[i][lane] = e;
        const float l = wave_sum_x(e);
        if (lane == 0) { st[0][i] = m; st[1][i] = l; }
    }
    __syncthreads();
    // P.V: key groups reduced by shuffles within the wave, LDS across waves (keys past nk carry p = 0, v = 0)
    float acc[RMAX][8];
#pragma unroll
    for (int i = 0; i < RMAX; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const bf16x8 v = u ? v1 : v0;
        const int jj = kg + 32 * u;
#pragma unroll
        for (int i = 0; i < RMAX; ++i)
            if (i < R) {
                // not fma8: through the helper the RMAX = 8 kernel's conversions are vectorised and its registers and
                // occupancy change (84 -> 79 VGPRs, 5 -> 6 waves per SIMD)
                const float pr = ps[i][jj];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[i][e] = fmaf(pr, bf2f(v[e]), acc[i][e]);
            }
    }
#pragma unroll
    for (int i = 0; i < RMAX; ++i)
        if (i < R)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // the two half-waves' key groups stay separate (no xor-32 round trip): 8 partials per output
                float a = acc[i][e];
                a += xor_lane<8>(a);
                a += xor_lane<16>(a);
                if ((lane & 31) < 8) red[2 * w + (lane >> 5)][i][dg * 8 + e] = a;
            }
    __syncthreads();
    auto osum = [&](int r, int d) {   // the NQ partial sums of output (r, d), in a fixed order
        float o = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) o += red[q][r][d];
        return o;
    };
    if (S == 1 && !n_keys_pos) {
        for (int i = tid; i < R * 64; i += 256) {
            const int r = i >> 6, d = i & 63;
            out[(int64_t)(r0 + r) * D + h * 64 + d] = f2bf(osum(r, d) / st[1][r]);
        }
        return;
    }
    // partial of this chunk: o[R][64], m[R], l[R]
    float* pp = part + ((int64_t)(b * H + h) * S + s) * (RMAX * 66);
    for (int i = tid; i < R * 64; i += 256) {
        const int r = i >> 6, d = i & 63;
        pp[i] = osum(r, d);
    }
    if (tid < R) { pp[RMAX * 64 + tid] = st[0][tid]; pp[RMAX * 65 + tid] = st[1][tid]; }
}

// the S chunk partials of a (kv batch, head) combined in chunk order: thread = (row, dim)
template <int RMAX>
__global__ __launch_bounds__(512) void dec_attn_combine_kernel(const float* __restrict__ part, int S, int R,
                                                               bf16* __restrict__ out, int D) {
    const int h = blockIdx.x, b = blockIdx.y, H = gridDim.x, i = threadIdx.x;
    if (i >= R * 64) return;
    const int r = i >> 6, d = i & 63;
    const float* base = part + (int64_t)(b * H + h) * S * (RMAX * 66);
    float mv[DS_MAXS], lv[DS_MAXS], ov[DS_MAXS];   // every partial load in flight at once (clamped chunk index:
    // unconditional loads, the chunks past S are never used)
#pragma unroll
    for (int c = 0; c < DS_MAXS; ++c) {
        const float* pc = base + min(c, S - 1) * (RMAX * 66);
        mv[c] = pc[RMAX * 64 + r];
        lv[c] = pc[RMAX * 65 + r];
        ov[c] = pc[i];
    }
    float M = -INFINITY;
#pragma unroll
    for (int c = 0; c < DS_MAXS; ++c)
        if (c < S) M = fmaxf(M, mv[c]);
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int c = 0; c < DS_MAXS; ++c)
        if (c < S && lv[c] > 0.f) {
            const float f = __expf(mv[c] - M);
            o = fmaf(f, ov[c], o);
            L = fmaf(f, lv[c], L);
        }
    out[(int64_t)(b * R + r) * D + h * 64 + d] = f2bf(o / L);
}

// Decode-step self-attention in one launch (round 6): workgroup = (row, head) over the row's <= DSA_MAXK cached keys,
// every load of the row issued before the first wait -- the query's 16 dims per lane straight from global (no LDS
// staging), K as NP passes of 64 keys (4 lanes per key, 16 dims each), V as 2 NP groups of 32 keys (8 dims per lane)
// -- so the softmax, P.V and the normalisation need no second launch (the split kernel's combine).  NP = ceil(n_keys
// / 64) is uniform per workgroup and selects a fully unrolled body (unconditional, clamped loads: keys past n_keys
// read key n_keys - 1 and carry weight 0).  Reductions in a fixed order (deterministic).
constexpr int DSA_MAXP = 7;
constexpr int DSA_MAXK = DSA_MAXP * 64;   // 448 = Whisper's max_target_positions
template <int NP>
__device__ __forceinline__ void dec_self_attn_body(const bf16* __restrict__ qr, const bf16* __restrict__ kb,
                                                   const bf16* __restrict__ vb, int nk, int D, bf16* __restrict__ out,
                                                   float* ps, float* red, float (*pv)[64]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j = tid >> 2, p = tid & 3;     // scores: key j + 64 u, dims 16 p .. 16 p + 15
    const int dg = tid & 7, kg = tid >> 3;   // P.V: dims 8 dg .. 8 dg + 7, keys kg + 32 u
    const bf16x8 qa = *(const bf16x8*)(qr + p * 16);
    const bf16x8 qb = *(const bf16x8*)(qr + p * 16 + 8);
    bf16x8 ka[NP], kb2[NP], vv[2 * NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const int jj = min(j + 64 * u, nk - 1);
        ka[u] = *(const bf16x8*)(kb + (int64_t)jj * D + p * 16);
        kb2[u] = *(const bf16x8*)(kb + (int64_t)jj * D + p * 16 + 8);
    }
#pragma unroll
    for (int u = 0; u < 2 * NP; ++u) vv[u] = *(const bf16x8*)(vb + (int64_t)min(kg + 32 * u, nk - 1) * D + dg * 8);
    float sc[NP];
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const float d = dot16_quad(qa, qb, ka[u], kb2[u]);
        sc[u] = j + 64 * u < nk ? d : -INFINITY;
        mx = fmaxf(mx, sc[u]);
    }
    mx = wave_max_x(mx);
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float l = 0.f;
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const float e = j + 64 * u < nk ? __expf(sc[u] - mx) : 0.f;
        if (p == 0) { ps[j + 64 * u] = e; l += e; }
    }
    l = wave_sum_x(l);
    if (lane == 0) red[4 + w] = l;
    __syncthreads();
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2 * NP; ++u) fma8(ps[kg + 32 * u], vv[u], acc);
#pragma unroll
    for (int e = 0; e < 8; ++e) {   // the wave's 8 key groups (lane bits 3-5), then the 4 waves in LDS
        float a = acc[e];
        a += xor_lane<8>(a);
        a += xor_lane<16>(a);
        a += __shfl_xor(a, 32, 64);
        if (lane < 8) pv[w][dg * 8 + e] = a;
    }
    __syncthreads();
    if (tid < 64) {
        const float L = (red[4] + red[5]) + (red[6] + red[7]);
        out[tid] = f2bf(((pv[0][tid] + pv[1][tid]) + (pv[2][tid] + pv[3][tid])) / L);
    }
}
__global__ __launch_bounds__(256) void dec_self_attn_kernel(const bf16* __restrict__ q, int ldq,
                                                            const bf16* __restrict__ kc, const bf16* __restrict__ vc,
                                                            int64_t kv_bstride, int n_keys, bf16* __restrict__ out,
                                                            int D, const int* __restrict__ n_keys_pos, int nk_rows) {
    __shared__ float ps[DSA_MAXK];
    __shared__ float red[8];
    __shared__ float pv[4][64];
    const int r = blockIdx.x, h = blockIdx.y;
    if (n_keys_pos) n_keys = min(n_keys, n_keys_pos[nk_rows ? r : 0] + 1);
    const int nk = max(1, min(n_keys, DSA_MAXK));
    const bf16* qr = q + (int64_t)r * ldq + h * 64;
    const bf16* kb = kc + r * kv_bstride + h * 64;
    const bf16* vb = vc + r * kv_bstride + h * 64;
    bf16* o = out + (int64_t)r * D + h * 64;
    switch ((nk + 63) >> 6) {
        case 1: dec_self_attn_body<1>(qr, kb, vb, nk, D, o, ps, red, pv); break;
        case 2: dec_self_attn_body<2>(qr, kb, vb, nk, D, o, ps, red, pv); break;
        case 3: dec_self_attn_body<3>(qr, kb, vb, nk, D, o, ps, red, pv); break;
        case 4: dec_self_attn_body<4>(qr, kb, vb, nk, D, o, ps, red, pv); break;
        case 5: dec_self_attn_body<5>(qr, kb, vb, nk, D, o, ps, red, pv); break;
        case 6: dec_self_attn_body<6>(qr, kb, vb, nk, D, o, ps, red, pv); break;
        default: dec_self_attn_body<7>(qr, kb, vb, nk, D, o, ps, red, pv); break;
    }
}

// beam reorder: dst[r] = src[src_rows[r]] for the first len positions of every cache row
__global__ void dec_gather_rows_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst, const int* __restrict__ rows,
                                       int64_t row_elems, int64_t copy_elems) {
    const int r = blockIdx.y;
    const bf16* s = src + (int64_t)min(max(rows[r], 0), (int)gridDim.y - 1) * row_elems;   // clamped, as dec_reorder_kv_kernel
    bf16* d = dst + (int64_t)r * row_elems;
    for (int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * 8; i < copy_elems; i += (int64_t)gridDim.x * blockDim.x * 8)
        *(bf16x8*)(d + i) = *(const bf16x8*)(s + i);
}

// beam reorder of the whole self-attention K/V cache in place, every layer in one launch: a thread owns
// one 16-byte column (layer, K or V, position chunk) of all B <= 16 rows, loads the B source rows of it,
// then writes the rows whose source differs -- no other thread touches those bytes, so no staging copy
__global__ __launch_bounds__(256) void dec_reorder_kv_kernel(bf16* __restrict__ ks, bf16* __restrict__ vs,
                                                             const int* __restrict__ rows, int B, int64_t layer_elems,
                                                             int64_t row_elems, int64_t chunks) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= chunks) return;
    bf16* base = (blockIdx.z ? vs : ks) + blockIdx.y * layer_elems + i * 8;
    bf16x8 v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r)   // rows that keep their own history are neither read nor written
        if (r < B && rows[r] != r) v[r] = *(const bf16x8*)(base + min(max(rows[r], 0), B - 1) * row_elems);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (r < B && rows[r] != r) *(bf16x8*)(base + r * row_elems) = v[r];
}
}  // namespace

hipError_t cbw_dec_embed(const int* tok, const uint16_t* E, const float* P, int pos, float* h, int B, int D,
                         hipStream_t st, int pos_inc, const int* pos_dev, int pos_rows) {
    hipLaunchKernelGGL(dec_embed_kernel, dim3(B), dim3(256), 0, st, tok, (const bf16*)E, P, pos, pos_inc, h, D, pos_dev,
                       pos_rows);
    return hipGetLastError();
}

hipError_t cbw_dec_kv_prefill(const uint16_t* qkv, uint16_t* kc, uint16_t* vc, int T, int B, int D, int maxlen,
                              hipStream_t st) {
    hipLaunchKernelGGL(dec_kv_prefill_kernel, dim3(T, B), dim3(64), 0, st, (const bf16*)qkv, (bf16*)kc, (bf16*)vc, D,
                       maxlen);
    return hipGetLastError();
}

hipError_t cbw_dec_kv_append(const uint16_t* qkv, uint16_t* kc, uint16_t* vc, int B, int D, int maxlen, int pos,
                             hipStream_t st) {
    hipLaunchKernelGGL(dec_kv_append_kernel, dim3(B), dim3(64), 0, st, (const bf16*)qkv, (bf16*)kc, (bf16*)vc, D, maxlen,
                       pos);
    return hipGetLastError();
}

hipError_t cbw_dec_attention(const uint16_t* q, int ldq, const uint16_t* kc, const uint16_t* vc, int64_t kv_bstride,
                             int n_keys, int rows_per_kv, uint16_t* out, int B, int H, int D, hipStream_t st,
                             int causal) {
    if (n_keys > DA_MAXK || n_keys <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_attention_kernel, dim3(B, H), dim3(256), 0, st, (const bf16*)q, ldq, (const bf16*)kc,
                       (const bf16*)vc, kv_bstride, n_keys, rows_per_kv, (bf16*)out, D, causal);
    return hipGetLastError();
}

hipError_t cbw_dec_self_attn(const uint16_t* q, int ldq, const uint16_t* kc, const uint16_t* vc, int64_t kv_bstride,
                             int n_keys, uint16_t* out, int B, int H, int D, hipStream_t st, const int* n_keys_pos,
                             int nk_rows) {
    if (n_keys <= 0 || n_keys > DSA_MAXK || B <= 0 || H * 64 > D) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_self_attn_kernel, dim3(B, H), dim3(256), 0, st, (const bf16*)q, ldq, (const bf16*)kc,
                       (const bf16*)vc, kv_bstride, n_keys, (bf16*)out, D, n_keys_pos, nk_rows);
    return hipGetLastError();
}

hipError_t cbw_dec_cross_probs(const uint16_t* q, int ldq, const uint16_t* kc, int n_keys, int T, int D, int head,
                               float* out, hipStream_t st) {
    if (n_keys > DA_MAXK || n_keys <= 0 || T <= 0 || head < 0 || (head + 1) * 64 > D) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_cross_probs_kernel, dim3(T), dim3(256), 0, st, (const bf16*)q, ldq, (const bf16*)kc, n_keys,
                       D, head, out);
    return hipGetLastError();
}

int64_t cbw_dtw_trace_words(int T, int F) { return (int64_t)T * ((T + F - 1 + 15) >> 4); }

hipError_t cbw_align_matrix_launch(const float* probs, int n, int T_all, int t0, int T, int F, int width,
                                   float* matrix, int* degenerate, hipStream_t st) {
    if (n < 1 || T < 1 || t0 < 0 || t0 + T > T_all || F < 1 || F > 1500 || width < 1 || width > 7 || !(width & 1))
        return hipErrorInvalidValue;
    if (F <= width / 2) width = 1;   // median_filter leaves such a short row as it is
    const int tile = 32 - 2 * (width / 2);
    const dim3 grid((F + tile - 1) / tile), block(32 * AM_G);
    switch (width) {
    case 1: hipLaunchKernelGGL(align_matrix_kernel<1>, grid, block, 0, st, probs, n, T_all, t0, T, F, matrix, degenerate); break;
    case 3: hipLaunchKernelGGL(align_matrix_kernel<3>, grid, block, 0, st, probs, n, T_all, t0, T, F, matrix, degenerate); break;
    case 5: hipLaunchKernelGGL(align_matrix_kernel<5>, grid, block, 0, st, probs, n, T_all, t0, T, F, matrix, degenerate); break;
    default: hipLaunchKernelGGL(align_matrix_kernel<7>, grid, block, 0, st, probs, n, T_all, t0, T, F, matrix, degenerate);
    }
    return hipGetLastError();
}

hipError_t cbw_dtw_launch(const float* matrix, int T, int F, int* first_frame, int* text_idx, int* time_idx, int* len,
                          uint32_t* trace, hipStream_t st) {
    if (T < 1 || T > DTW_MAX_T || F < 1 || F > CBW_DTW_MAX_F) return hipErrorInvalidValue;
    // the x dimension of the grid stays free for a batch of matrices
    hipLaunchKernelGGL(dtw_kernel, dim3(1), dim3((T + 63) / 64 * 64), 0, st, matrix, T, F, first_frame, text_idx,
                       time_idx, len, trace);
    return hipGetLastError();
}

hipError_t cbw_align_matrix_batch_launch(const cbw_ts_batch& b, int N, int n, int width, int* degenerate,
                                         hipStream_t st) {
    if (N < 1 || N > CBW_TS_MAX_WINDOWS || n < 1 || width < 1 || width > 7 || !(width & 1)) return hipErrorInvalidValue;
    int tiles = 0;
    for (int i = 0; i < N; ++i) {
        const cbw_ts_win& w = b.w[i];
        if (w.T < 1 || w.t0 < 0 || w.t0 + w.T > w.T_all || w.F < 1 || w.F > 1500) return hipErrorInvalidValue;
        const int tile = 32 - 2 * (w.F <= width / 2 ? 0 : width / 2);
        tiles = std::max(tiles, (w.F + tile - 1) / tile);
    }
    const dim3 grid(tiles, N), block(32 * AM_G);
    switch (width) {
    case 1: hipLaunchKernelGGL(align_matrix_batch_kernel<1>, grid, block, 0, st, b, n, degenerate); break;
    case 3: hipLaunchKernelGGL(align_matrix_batch_kernel<3>, grid, block, 0, st, b, n, degenerate); break;
    case 5: hipLaunchKernelGGL(align_matrix_batch_kernel<5>, grid, block, 0, st, b, n, degenerate); break;
    default: hipLaunchKernelGGL(align_matrix_batch_kernel<7>, grid, block, 0, st, b, n, degenerate);
    }
    return hipGetLastError();
}

hipError_t cbw_dtw_batch_launch(const cbw_ts_batch& b, int N, int* first_frame, int ld, hipStream_t st) {
    if (N < 1 || N > CBW_TS_MAX_WINDOWS) return hipErrorInvalidValue;
    int Tmax = 0;
    for (int i = 0; i < N; ++i) {
        const cbw_ts_win& w = b.w[i];
        if (w.T < 1 || w.T > DTW_MAX_T || w.F < 1 || w.F > CBW_DTW_MAX_F) return hipErrorInvalidValue;
        Tmax = std::max(Tmax, w.T);
    }
    if (ld < Tmax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dtw_batch_kernel, dim3(N), dim3((Tmax + 63) / 64 * 64), 0, st, b, first_frame, ld);
    return hipGetLastError();
}

int cbw_dec_attn_split_floats(int B, int H) { return B * H * DS_MAXS * 8 * 66; }

hipError_t cbw_dec_attn_split(const uint16_t* q, int ldq, const uint16_t* kc, const uint16_t* vc, int64_t kv_bstride,
                              int n_keys, int rows_per_kv, uint16_t* out, int B, int H, int D, float* part,
                              hipStream_t st, const int* n_keys_pos, int nk_rows) {
    const int S = (n_keys + DS_CHUNK - 1) / DS_CHUNK;
    if (n_keys <= 0 || S > DS_MAXS || rows_per_kv < 1 || rows_per_kv > 8 || B % rows_per_kv) return hipErrorInvalidValue;
    const dim3 grid(S, H, B / rows_per_kv);
#define DS_LAUNCH(RM)                                                                                                 \
    hipLaunchKernelGGL((dec_attn_split_kernel<RM>), grid, dim3(256), 0, st, (const bf16*)q, ldq, (const bf16*)kc,      \
                       (const bf16*)vc, kv_bstride, n_keys, rows_per_kv, (bf16*)out, D, part, n_keys_pos, nk_rows)
    if (rows_per_kv == 1) DS_LAUNCH(1);
    else DS_LAUNCH(8);
#undef DS_LAUNCH
    if (S > 1 || n_keys_pos) {
        const dim3 cgrid(H, B / rows_per_kv);
        if (rows_per_kv == 1)
            hipLaunchKernelGGL(dec_attn_combine_kernel<1>, cgrid, dim3(64), 0, st, part, S, 1, (bf16*)out, D);
        else
            hipLaunchKernelGGL(dec_attn_combine_kernel<8>, cgrid, dim3(64 * rows_per_kv), 0, st, part, S, rows_per_kv,
                               (bf16*)out, D);
    }
    return hipGetLastError();
}

hipError_t cbw_dec_gather_rows(const uint16_t* src, uint16_t* dst, const int* rows, int B, int64_t row_elems,
                               int64_t copy_elems, hipStream_t st) {
    hipLaunchKernelGGL(dec_gather_rows_kernel, dim3(64, B), dim3(256), 0, st, (const bf16*)src, (bf16*)dst, rows,
                       row_elems, copy_elems);
    return hipGetLastError();
}

hipError_t cbw_dec_reorder_kv(uint16_t* ks, uint16_t* vs, const int* rows, int B, int n_layers, int64_t layer_elems,
                              int64_t row_elems, int64_t copy_elems, hipStream_t st) {
    if (B < 1 || B > 16 || copy_elems % 8 || row_elems % 8) return hipErrorInvalidValue;
    const int64_t chunks = copy_elems / 8;
    if (chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(dec_reorder_kv_kernel, dim3((unsigned)((chunks + 255) / 256), n_layers, 2), dim3(256), 0, st,
                       (bf16*)ks, (bf16*)vs, rows, B, layer_elems, row_elems, chunks);
    return hipGetLastError();
}

hipError_t cbw_mel_frames(const float* pcm, int n_samples, const float* filters, const float* twiddle, float* logmel,
                          int n_mel, hipStream_t st, int L_pad, int frames) {
    if (L_pad <= 0) L_pad = N_SAMPLES;
    if (frames <= 0) frames = N_FRAMES;
    hipLaunchKernelGGL(mel_frames_kernel, dim3(frames), dim3(256), 0, st, pcm, n_samples, filters, twiddle, logmel,
                       n_mel, L_pad, frames);
    return hipGetLastError();
}

hipError_t cbw_mel_finish(float* logmel, int n_mel, float* scratch, uint16_t* packed, int cpad, hipStream_t st,
                          int frames) {
    const int parts = frames > 0 ? CBW_MEL_LONG_PARTS : 1;   // the 30 s window keeps its single-block max
    if (frames <= 0) frames = N_FRAMES;
    hipLaunchKernelGGL(max_reduce_kernel, dim3(parts), dim3(1024), 0, st, logmel, (int64_t)n_mel * frames, scratch);
    hipLaunchKernelGGL(mel_finish_kernel, dim3(1024), dim3(256), 0, st, logmel, n_mel, scratch, parts, (bf16*)packed,
                       cpad, frames);
    return hipGetLastError();
}

hipError_t cbw_resample_taps(const float* pcm, int C, int64_t len, const float* tab, int o, int n, int width, int T,
                             float* out, int64_t out_len, hipStream_t st) {
    const int64_t blocks = (out_len + 255) / 256;
    if (C < 1 || len < 1 || out_len < 1 || blocks > 0x7fffffffLL || T != 2 * width + o) return hipErrorInvalidValue;
    if ((int64_t)n * T <= CBW_RESAMPLE_LDS_FLOATS)
        hipLaunchKernelGGL(resample_kernel<true>, dim3((unsigned)blocks), dim3(256), (size_t)n * T * sizeof(float), st,
                           pcm, C, len, tab, o, n, width, T, out, out_len);
    else
        hipLaunchKernelGGL(resample_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, pcm, C, len, tab, o, n,
                           width, T, out, out_len);
    return hipGetLastError();
}

hipError_t cbw_downmix(const float* pcm, int C, int64_t len, float* out, hipStream_t st) {
    const int64_t blocks = (len + 255) / 256;
    if (C < 1 || len < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(downmix_kernel, dim3((unsigned)blocks), dim3(256), 0, st, pcm, C, len, out);
    return hipGetLastError();
}

hipError_t cbw_layernorm(const float* x, const float* g, const float* b, uint16_t* y, float* y32, int rows, int D,
                         float eps, hipStream_t st) {
    if (D % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(layernorm_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x, g, b, (bf16*)y, y32, rows, D, eps);
    return hipGetLastError();
}

hipError_t cbw_attention(const uint16_t* qkv, uint16_t* out, int B, int T, int H, int hd, hipStream_t st) {
    if (hd != 64 || T <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attention_kernel, dim3((T + 63) / 64, B * H), dim3(256), 0, st, (const bf16*)qkv, (bf16*)out,
                       T, H);
    return hipGetLastError();
}
