// Token choice for gfx950: from a row of decoder logits to the next token.  The beam path's log-softmax + top-k
// (one-pass and two-stage), WhisperTimeStampLogitsProcessor as an additive mask, the greedy and the sampling choice of a
// lock-step decode, and the beam-search bookkeeping.  Each shared piece is stated once: the 16-wave block reductions,
// the sorted register top-k list (tk_*), the timestamp rule state and its positional mask (ts_rule_state, ts_masked).
//
// Reference semantics: transformers 4.37.2 generation (logits_process.py, beam_search.py, utils.py); see
// oracle/decoder.py and cbw/timestamps.py for the restated algorithms these kernels are checked against.
#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <map>

#include "cbw_common.h"
#include "cbw_kernels.h"

namespace {

// ---------------------------------------------------------------- reductions over a 1024-thread block's 16 waves
// every thread receives the result; red[0..15] are combined in ascending order
CBW_DEV float block_max16(float v, float* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    v = wave_max(v);
    if (lane == 0) red[wid] = v;
    __syncthreads();
    float m = red[0];
    for (int w = 1; w < 16; ++w) m = fmaxf(m, red[w]);
    __syncthreads();
    return m;
}
CBW_DEV float block_sum16(float v, float* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    v = wave_sum(v);
    if (lane == 0) red[wid] = v;
    __syncthreads();
    float tot = 0.f;
    for (int w = 0; w < 16; ++w) tot += red[w];
    __syncthreads();
    return tot;
}
// (max, lowest index of it); nothing above -inf: index 0x7fffffff
CBW_DEV void block_argmax16(float v, int i, float* red, int* redi, float& M, int& I) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float wm = wave_max(v);
    int ci = v == wm ? i : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ci = min(ci, __shfl_xor(ci, o, 64));
    if (lane == 0) { red[wid] = wm; redi[wid] = ci; }
    __syncthreads();
    M = red[0];
    I = redi[0];
    for (int w = 1; w < 16; ++w)
        if (red[w] > M || (red[w] == M && redi[w] < I)) { M = red[w]; I = redi[w]; }
    __syncthreads();
}

// ---------------------------------------------------------------- log-softmax + top-k (the beam path)
// A lane's top-k (k <= 16) as a sorted register list of (value, token id), best first; ties keep the lower id.
// Empty slots hold (-inf, 0x7fffffff).
constexpr int TK_MAX = 16;

CBW_DEV bool tk_better(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }

CBW_DEV void tk_clear(float (&tv)[TK_MAX], int (&ti)[TK_MAX]) {
#pragma unroll
    for (int j = 0; j < TK_MAX; ++j) { tv[j] = -INFINITY; ti[j] = 0x7fffffff; }
}

// insert (v, i) into the list's k entries (compare-and-swap down the list: static indices only, so the list stays in
// VGPRs -- a data-dependent insertion index put it in scratch memory)
CBW_DEV void tk_insert(float (&tv)[TK_MAX], int (&ti)[TK_MAX], int k, float v, int i) {
#pragma unroll
    for (int q = 0; q < TK_MAX; ++q) {
        if (q < k) {
            const bool b = tk_better(v, i, tv[q], ti[q]);
            const float ov = tv[q];
            const int oi = ti[q];
            tv[q] = b ? v : ov;
            ti[q] = b ? i : oi;
            v = b ? ov : v;
            i = b ? oi : i;
        }
    }
}

// insert (v, i) if it beats the list's k-th entry
CBW_DEV void tk_offer(float (&tv)[TK_MAX], int (&ti)[TK_MAX], int k, float v, int i) {
    float kv = -INFINITY;
    int ki = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < TK_MAX; ++q)
        if (q == k - 1) { kv = tv[q]; ki = ti[q]; }
    if (tk_better(v, i, kv, ki)) tk_insert(tv, ti, k, v, i);
}

// k rounds of (max value, min index) over the 64 lanes' list heads; lane 0 receives the merged list
CBW_DEV void tk_wave_merge(float (&tv)[TK_MAX], int (&ti)[TK_MAX], int k, float* mv, int* mi) {
    const int lane = threadIdx.x & 63;
    for (int j = 0; j < k; ++j) {
        float bv = tv[0];
        int bi = ti[0];
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (tk_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { mv[j] = bv; mi[j] = bi; }
        if (ti[0] == bi && tv[0] == bv) {   // the owner pops its head (ids are unique across lanes)
#pragma unroll
            for (int q = 0; q < TK_MAX - 1; ++q) { tv[q] = tv[q + 1]; ti[q] = ti[q + 1]; }
            tv[TK_MAX - 1] = -INFINITY;
            ti[TK_MAX - 1] = 0x7fffffff;
        }
    }
}

// a block's n sorted lists in LDS (one per wave; n a power of two <= 64) merged by one wave: lane l < n owns list l,
// lane 0 receives the merged list
CBW_DEV void tk_merge_lists(const float (*cv)[TK_MAX], const int (*ci)[TK_MAX], int n, int k, float* mv, int* mi) {
    const int lane = threadIdx.x & 63;
    float lv[TK_MAX];
    int li[TK_MAX];
#pragma unroll
    for (int q = 0; q < TK_MAX; ++q) {
        lv[q] = (lane < n && q < k) ? cv[lane & (n - 1)][q] : -INFINITY;
        li[q] = (lane < n && q < k) ? ci[lane & (n - 1)][q] : 0x7fffffff;
    }
    tk_wave_merge(lv, li, k, mv, mi);
}

// One pass per row, one workgroup (CBW_TOPK_SPLIT=0; the two-stage kernels below are the default):
// log_softmax(logits) + bias and its top-k.
__global__ __launch_bounds__(1024) void logprob_topk_kernel(const float* __restrict__ logits, int V, int ld,
                                                            const float* __restrict__ bias, int64_t bias_ld, int k,
                                                            float* __restrict__ out_lp, int* __restrict__ out_idx) {
    __shared__ float red[16];
    __shared__ float cand_v[16][TK_MAX], outv[TK_MAX];
    __shared__ int cand_i[16][TK_MAX], outi[TK_MAX];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* x = logits + (int64_t)r * ld;
    if (bias) bias += (int64_t)r * bias_ld;
    // log_softmax over the RAW logits, the logits processors' additive masks after it: HF beam search
    // normalises first (next_token_scores = log_softmax(logits); processed = processors(scores)), so a
    // suppressed token's mass stays in the normaliser
    // two passes over the row, eight loads in flight per thread in each
    constexpr int TK_U = 8;
    float mx = -INFINITY;
    for (int i0 = tid; i0 < V; i0 += 1024 * TK_U) {
        float v[TK_U];
#pragma unroll
        for (int u = 0; u < TK_U; ++u) v[u] = i0 + u * 1024 < V ? x[i0 + u * 1024] : -INFINITY;
#pragma unroll
        for (int u = 0; u < TK_U; ++u) mx = fmaxf(mx, v[u]);
    }
    mx = block_max16(mx, red);
    // second pass: the normaliser and, per thread, the top-k of its strided slice of logits + bias
    float tv[TK_MAX];
    int ti[TK_MAX];
    tk_clear(tv, ti);
    float s = 0.f;
    for (int i0 = tid; i0 < V; i0 += 1024 * TK_U) {
        float v[TK_U], bv[TK_U];
#pragma unroll
        for (int u = 0; u < TK_U; ++u) {
            const int i = i0 + u * 1024;
            v[u] = i < V ? x[i] : -INFINITY;
            bv[u] = (bias && i < V) ? bias[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < TK_U; ++u) {
            const int i = i0 + u * 1024;
            if (i >= V) continue;
            s += __expf(v[u] - mx);
            tk_offer(tv, ti, k, v[u] + bv[u], i);
        }
    }
    const float lse = mx + logf(block_sum16(s, red));
    tk_wave_merge(tv, ti, k, cand_v[wid], cand_i[wid]);
    __syncthreads();
    if (wid != 0) return;
    tk_merge_lists(cand_v, cand_i, 16, k, outv, outi);
    if (lane < k) {
        out_lp[(int64_t)r * k + lane] = outv[lane] - lse;
        out_idx[(int64_t)r * k + lane] = outi[lane];
    }
}

// ---- two-stage top-k: the row split into TK_CHUNKS chunks so ~B x 32 workgroups share the pass
constexpr int TK_CHUNKS = 32;

// stage 1: chunk c of row r -> its max m_c, sum exp(x - m_c), and top-k of x + bias.
// part layout per (r, c): [k values | k ids (int bits) | m_c | s_c], stride 2 * TK_MAX + 2 floats
__global__ __launch_bounds__(256) void topk_chunk_kernel(const float* __restrict__ logits, int V, int ld,
                                                         const float* __restrict__ bias, int64_t bias_ld, int k,
                                                         int chunk, float* __restrict__ part) {
    __shared__ float red[4];
    __shared__ float cv[4][TK_MAX];
    __shared__ int ci[4][TK_MAX];
    const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* x = logits + (int64_t)r * ld;
    if (bias) bias += (int64_t)r * bias_ld;
    const int lo = c * chunk, hi = min(V, lo + chunk);
    constexpr int U = 8;
    float tv[TK_MAX];
    int ti[TK_MAX];
    tk_clear(tv, ti);
    float mx = -INFINITY, sm = 0.f;
    for (int i0 = lo + tid; i0 < hi; i0 += 256 * U) {
        float v[U], bv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 256;
            v[u] = i < hi ? x[i] : -INFINITY;
            bv[u] = (bias && i < hi) ? bias[i] : 0.f;
        }
        float m2 = mx;
#pragma unroll
        for (int u = 0; u < U; ++u) m2 = fmaxf(m2, v[u]);
        if (m2 > -INFINITY) {
            sm *= __expf(mx - m2);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (i0 + u * 256 < hi) sm += __expf(v[u] - m2);
            mx = m2;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i0 + u * 256 < hi) tk_offer(tv, ti, k, v[u] + bv[u], i0 + u * 256);
    }
    // (max, sum) of the chunk: wave then block, rescaled to the chunk max
    float wm = wave_max(mx);
    float ws = wave_sum(mx > -INFINITY ? sm * __expf(mx - wm) : 0.f);
    __shared__ float red_s[4];
    if (lane == 0) { red[wid] = wm; red_s[wid] = ws; }
    tk_wave_merge(tv, ti, k, cv[wid], ci[wid]);
    __syncthreads();
    if (wid != 0) return;
    float* pp = part + ((int64_t)r * gridDim.x + c) * (2 * TK_MAX + 2);
    __shared__ float outv[TK_MAX];
    __shared__ int outi[TK_MAX];
    tk_merge_lists(cv, ci, 4, k, outv, outi);
    if (lane < k) {
        pp[lane] = outv[lane];
        pp[TK_MAX + lane] = __int_as_float(outi[lane]);
    }
    if (lane == 0) {
        float M = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        float S = 0.f;
        for (int w = 0; w < 4; ++w) S += red[w] > -INFINITY ? red_s[w] * __expf(red[w] - M) : 0.f;
        pp[2 * TK_MAX] = M;
        pp[2 * TK_MAX + 1] = S;
    }
}

// stage 2: one wave per row merges the chunks (lane c owns chunk c's sorted list) and the normaliser
__global__ __launch_bounds__(64) void topk_merge_kernel(const float* __restrict__ part, int C, int k,
                                                        float* __restrict__ out_lp, int* __restrict__ out_idx) {
    __shared__ float mv[TK_MAX];
    __shared__ int mi[TK_MAX];
    const int r = blockIdx.x, lane = threadIdx.x;
    const float* pp = part + ((int64_t)r * C + min(lane, C - 1)) * (2 * TK_MAX + 2);
    const bool own = lane < C;
    float tv[TK_MAX];
    int ti[TK_MAX];
#pragma unroll
    for (int q = 0; q < TK_MAX; ++q) {
        tv[q] = (own && q < k) ? pp[q] : -INFINITY;
        ti[q] = (own && q < k) ? __float_as_int(pp[TK_MAX + q]) : 0x7fffffff;
    }
    const float m = own ? pp[2 * TK_MAX] : -INFINITY;
    const float sc = own ? pp[2 * TK_MAX + 1] : 0.f;
    const float M = wave_max(m);
    const float S = wave_sum(m > -INFINITY ? sc * __expf(m - M) : 0.f);
    const float lse = M + logf(S);
    tk_wave_merge(tv, ti, k, mv, mi);
    __syncthreads();
    if (lane < k) {
        out_lp[(int64_t)r * k + lane] = mv[lane] - lse;
        out_idx[(int64_t)r * k + lane] = mi[lane];
    }
}

// ---------------------------------------------------------------- WhisperTimeStampLogitsProcessor
// (transformers 4.37.2, generation/logits_process.py; installed 5.15 copy is identical)
// A row's rule state: {last_was_timestamp, penultimate_was_timestamp, first allowed timestamp id (timestamps below it
// are masked; = timestamp_begin when none was sampled), at_begin (no token sampled yet)}.
struct TsRuleState {
    bool last_ts, penult_ts;
    int ts_floor;
    bool at_begin;
};

// ... from the row's history state {n tokens sampled, the last, the second last, the last timestamp (-1: none)}; tb =
// the first timestamp id (cbw/timestamps.py TimestampRules.state is the host's statement of it)
CBW_DEV TsRuleState ts_rule_state(int n, int t1, int t2, int lts, int tb) {
    const bool last = n >= 1 && t1 >= tb, penult = n < 2 || t2 >= tb;
    return {last, penult, lts < 0 ? tb : ((last && !penult) ? lts : lts + 1), n == 0};
}

// The processor's positional mask of token i (everything but the mass rule): no_timestamps, the pair rules, the
// non-decreasing floor and the max_initial window at the start.  Text ids below tb, timestamps from tb on.  The only
// statement of the mask, and a function over scalars on purpose: behind a struct holding the same values
// timestamp_rules_kernel ran 31.5 us instead of 24.6 (docs/MEASUREMENT_LOG.md, "token_select.hip").
CBW_DEV bool ts_masked(int i, bool last_ts, bool penult_ts, int ts_floor, bool at_begin, int tb, int no_ts, int eos,
                       int max_initial) {
    bool m = i == no_ts;
    if (last_ts) m = m || (penult_ts ? i >= tb : i < eos);
    m = m || (i >= tb && i < ts_floor);
    if (at_begin) m = m || i < tb || (max_initial >= 0 && i > tb + max_initial);
    return m;
}
// the rule state and the three token ids of a row whose mask is asked for many times (SelectRow)
struct TsMask {
    TsRuleState s;
    int tb, no_ts, eos, max_initial;
    CBW_DEV bool masked(int i) const {
        return ts_masked(i, s.last_ts, s.penult_ts, s.ts_floor, s.at_begin, tb, no_ts, eos, max_initial);
    }
};

// The processor for one decoding row per block, as an additive mask on top of the shared suppression bias:
// bias_out[r][i] = bias[i] + (masked ? -inf : 0); st[r] = the row's rule state.
// The "timestamp mass beats every text token" test compares logsumexp over the timestamp tokens with
// the max over text tokens of the masked logits (log_softmax is a common shift of both).
__global__ __launch_bounds__(1024) void timestamp_rules_kernel(const float* __restrict__ logits, int V, int ld,
                                                               const float* __restrict__ bias,
                                                               const int* __restrict__ st, int ts_begin, int no_ts,
                                                               int eos, int max_initial,
                                                               float* __restrict__ bias_out) {
    __shared__ float red[16];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (int64_t)r * ld;
    float* o = bias_out + (int64_t)r * V;
    const int last_ts = st[4 * r], penult_ts = st[4 * r + 1], ts_floor = st[4 * r + 2], at_begin = st[4 * r + 3];
#define TS_MASKED(i) ts_masked(i, last_ts, penult_ts, ts_floor, at_begin, ts_begin, no_ts, eos, max_initial)
    float mt = -INFINITY, mts = -INFINITY;
    // eight logits and biases in flight per thread: unconditional loads of clamped indices (a load inside the bound
    // check made the compiler wait for each before the next); max is order-independent
    const float* bsrc = bias ? bias : x;
    for (int i0 = tid; i0 < V; i0 += 8 * 1024) {
        float xv[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int ii = min(i0 + u * 1024, V - 1);
            xv[u] = x[ii];
            bv[u] = bsrc[ii];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 1024;
            if (i >= V) break;
            const float v = xv[u] + (TS_MASKED(i) ? -INFINITY : (bias ? bv[u] : 0.f));
            if (i < ts_begin) mt = fmaxf(mt, v);
            else mts = fmaxf(mts, v);
        }
    }
    const float m_ts = block_max16(mts, red), m_text = block_max16(mt, red);
    float s = 0.f;
    if (m_ts > -INFINITY)
        for (int i = ts_begin + tid; i < V; i += 1024) {
            const float b = bias ? bias[i] : 0.f;
            s += __expf(x[i] + (TS_MASKED(i) ? -INFINITY : b) - m_ts);
        }
    const float tot = block_sum16(s, red);
    const float lse_ts = m_ts > -INFINITY ? m_ts + logf(tot) : -INFINITY;
    const bool force_ts = lse_ts > m_text;
    for (int i0 = tid; i0 < V; i0 += 8 * 1024) {   // the biases again, eight in flight (as above)
        float bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) bv[u] = bsrc[min(i0 + u * 1024, V - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 1024;
            if (i >= V) break;
            const bool m = TS_MASKED(i);   // not behind the `||`: the compiler then sank a bias load into the branch
            o[i] = ((force_ts && i < ts_begin) || m) ? -INFINITY : (bias ? bv[u] : 0.f);
        }
    }
#undef TS_MASKED
}

// What greedy_select_kernel and sample_select_kernel share (1024-thread blocks, one row each).
// SelectRow: a row's history state ts_state[r] = {n, last, second last, last timestamp}, the rule state derived from it
// and the positional mask (ts_begin < 0: no timestamp rules, every token is text).
struct SelectRow {
    int sn, t1, tb, ts_begin, eos;
    bool rules;
    TsMask mask;
    __device__ __forceinline__ SelectRow(const int* st, int V, int ts_begin_, int no_ts, int eos_, int max_initial)
        : sn(st[0]), t1(st[1]), ts_begin(ts_begin_), eos(eos_) {
        rules = ts_begin >= 0;
        tb = rules ? ts_begin : V;   // text below, timestamps from tb on
        mask = {ts_rule_state(sn, t1, st[2], st[3], tb), tb, no_ts, eos, max_initial};
    }
    __device__ __forceinline__ bool masked(int i) const {
        const bool m = mask.masked(i);   // evaluated first, not behind `rules &&`: sample_select_kernel's register
        return rules && m;               // allocation follows this form (66 spilled VGPRs; 102 with the short circuit)
    }
};

// f(i, score_i) for the thread's indices tid, tid + 1024, ... in ascending order; score = -inf where the row's mask
// applies, else x[i] + bs[i] (bs may be NULL).  Unconditional loads of clamped indices, eight in flight, as
// timestamp_rules_kernel.
template <class F>
__device__ __forceinline__ void select_for_each(const SelectRow& row, const float* __restrict__ x,
                                                const float* __restrict__ bs, int V, F&& f) {
    const float* bsrc = bs ? bs : x;
    for (int i0 = threadIdx.x; i0 < V; i0 += 8 * 1024) {
        float xv[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int ii = min(i0 + u * 1024, V - 1);
            xv[u] = x[ii];
            bv[u] = bsrc[ii];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 1024;
            if (i >= V) break;
            f(i, row.masked(i) ? -INFINITY : xv[u] + (bs ? bv[u] : 0.f));
        }
    }
}

// Two passes over a row's masked scores (each(f) calls f(i, score_i) over the thread's indices in ascending order;
// tb = the row's first timestamp id), the same result in every thread: the max and its lowest index over the
// text and over the timestamp tokens, their sums of exponentials, and the mass rule (logsumexp of the timestamp
// scores > max text score: every text token is to be masked).
struct SelectStats {
    float m_text, m_ts, s_text, s_ts, lse_ts;
    int i_text, i_ts;
    bool force_ts;
};
template <class E>
__device__ __forceinline__ SelectStats select_class_stats(int tb, E&& each, float* red, int* redi) {
    SelectStats c;
    float mt = -INFINITY, mts = -INFINITY;
    int it = 0x7fffffff, its = 0x7fffffff;
    each([&](int i, float v) {   // ascending indices: `>` keeps the lowest of a maximum; selects of values, so that
                                 // the four stay in registers
        const bool text = i < tb;
        const bool ut = text && v > mt, us = !text && v > mts;
        mt = ut ? v : mt;
        it = ut ? i : it;
        mts = us ? v : mts;
        its = us ? i : its;
    });
    block_argmax16(mt, it, red, redi, c.m_text, c.i_text);
    block_argmax16(mts, its, red, redi, c.m_ts, c.i_ts);
    const float m_text = c.m_text, m_ts = c.m_ts;
    float st = 0.f, sts = 0.f;
    each([&](int i, float v) {
        const bool text = i < tb;
        const float e = text ? (m_text > -INFINITY ? __expf(v - m_text) : 0.f)
                             : (m_ts > -INFINITY ? __expf(v - m_ts) : 0.f);
        st += text ? e : 0.f;
        sts += text ? 0.f : e;
    });
    c.s_text = block_sum16(st, red);
    c.s_ts = block_sum16(sts, red);
    c.lse_ts = m_ts > -INFINITY ? m_ts + logf(c.s_ts) : -INFINITY;
    c.force_ts = c.lse_ts > m_text;
    return c;
}

// The bookkeeping after row r's choice (one thread): ts_state advances by the token and
// active[r] = token != eos && pos_rows[r] + 1 < limit[r].
__device__ __forceinline__ void select_finish(const SelectRow& row, int r, int tok, float lp, int* ts_state,
                                              const int* __restrict__ pos_rows, const int* __restrict__ limit,
                                              int* active, int* __restrict__ tokens, float* __restrict__ logprob) {
    ts_state[4 * r] = row.sn + 1;
    ts_state[4 * r + 1] = tok;
    ts_state[4 * r + 2] = row.t1;
    if (row.rules && tok >= row.ts_begin) ts_state[4 * r + 3] = tok;
    active[r] = (tok != row.eos && pos_rows[r] + 1 < limit[r]) ? 1 : 0;
    tokens[r] = tok;
    logprob[r] = lp;
}

// One greedy step's choice for every row of a lock-step decode, no host in the loop (HF 4.37.2 greedy search: the
// processors on the raw logits, argmax, log_softmax of the processed scores for the fallback checks).  One block per
// row, two passes over the row's V logits, eight loads in flight per thread in each:
//   scores = logits + (n == 0 ? bias_begin : bias) + the masks timestamp_rules_kernel applies, its rule state derived
//   here from ts_state[r] = {n, last, second last, last timestamp} (SelectRow)
//   (ts_begin < 0: no timestamp rules); pass 1 the max and lowest argmax of the text and of the timestamp scores,
//   pass 2 their sums of exponentials -> the mass rule (logsumexp of the timestamp scores > max text score: every
//   text token masked), token = argmax of what is left (ties -> lower id), logprob = score - logsumexp(left).
// Nothing finite left: token eos, logprob -inf.  Then ts_state[r] advances by the token and
// active[r] = token != eos && pos_rows[r] + 1 < limit[r]; the driver adds active to pos_rows after the decode step.
// A row inactive on entry only gets tokens[r] = eos.
// Invariant the driver relies on: an active row steps at pos <= limit - 2 (its token was kept only if
// pos + 1 < limit) and a row that ends stays at pos <= limit - 1 (it was selected at pos <= limit - 1 and its position
// no longer moves), so every K/V write of the steps enqueued past a row's end stays below limit <= max_len.
__global__ __launch_bounds__(1024) void greedy_select_kernel(const float* __restrict__ logits, int V, int ld,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ bias_begin, int ts_begin,
                                                             int no_ts, int eos, int max_initial, int* ts_state,
                                                             const int* __restrict__ pos_rows,
                                                             const int* __restrict__ limit, int* active,
                                                             int* __restrict__ tokens, float* __restrict__ logprob) {
    __shared__ float red[16];
    __shared__ int redi[16];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (!active[r]) {   // the whole block: uniform, before any barrier
        if (tid == 0) tokens[r] = eos;
        return;
    }
    const float* x = logits + (int64_t)r * ld;
    const SelectRow row(ts_state + 4 * r, V, ts_begin, no_ts, eos, max_initial);
    const float* bs = row.sn == 0 ? bias_begin : bias;
    const SelectStats c = select_class_stats(row.tb, [&](auto&& f) { select_for_each(row, x, bs, V, f); }, red, redi);
    if (tid != 0) return;
    const bool pick_ts = c.force_ts || c.m_ts > c.m_text;   // a tie across the boundary goes to the text token, the lower id
    const float best = pick_ts ? c.m_ts : c.m_text;
    int tok = pick_ts ? c.i_ts : c.i_text;
    float lp = -INFINITY;
    if (best > -INFINITY) {
        const float M = fmaxf(c.m_text, c.m_ts);
        const float lse = c.force_ts ? c.lse_ts
                                     : M + logf((c.m_text > -INFINITY ? c.s_text * __expf(c.m_text - M) : 0.f) +
                                                (c.m_ts > -INFINITY ? c.s_ts * __expf(c.m_ts - M) : 0.f));
        lp = best - lse;
    } else {
        tok = eos;
    }
    select_finish(row, r, tok, lp, ts_state, pos_rows, limit, active, tokens, logprob);
}

// The order-preserving integer image of a float (a < b as floats <=> okey(a) < okey(b) as unsigned; -inf the lowest
// of the ordered values) and its inverse: the radix select below works on it.
__device__ __forceinline__ unsigned okey(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float okey_value(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// scores a thread of sample_select_kernel holds in registers: V <= 1024 * 51 = 52224 (Whisper's vocabularies: 51864 to
// 51866)
constexpr int SAMPLE_PER_THREAD = CBW_SAMPLE_MAX_V / 1024;

// One sampling step's choice for every row of a lock-step decode, no host in the loop (HF 4.37.2 sample loop: the
// processors on the raw logits, then TemperatureLogitsWarper and TopKLogitsWarper, torch.multinomial of the softmax,
// log_softmax of the top-k-filtered processed scores for the fallback checks).  One block per row:
//   s = the processed scores exactly as greedy_select_kernel forms them (SelectRow's masks, select_class_stats' two
//   passes, then the mass rule's mask on the text tokens), read once into 51 registers per thread;
//   kth = the top_k-th largest s, found exactly by a radix select on okey(s): four passes, each a 256-bin LDS
//   histogram of one byte of the keys that match the bytes chosen so far (a thread adds a run of equal bins with one
//   atomic: the high bytes of logits fall into a handful of bins), wave 0 scans the bins from the top;
//   kept = {i : s_i > -inf and s_i >= kth} (ties at kth all kept; fewer than top_k finite: every finite one), tested
//   on the keys;
//   token = argmax over the kept i of (exp(s_i / T - max / T) / sum) / q_i in fp32, the form torch.multinomial's
//   exponential race evaluates with q = noise[r][i] ~ Exp(1) (ties -> lower id; a q that is not positive and finite
//   reads as FLT_MIN); logprob = s_token - logsumexp over the kept s.
// Nothing finite left, or no kept index won (NaN scores): token eos, logprob -inf -- the token written is always in
// [0, V) or eos.  The bookkeeping is greedy_select_kernel's (select_finish), so its position invariant holds here too.
__global__ __launch_bounds__(1024) void sample_select_kernel(const float* __restrict__ logits, int V, int ld,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ bias_begin, int ts_begin,
                                                             int no_ts, int eos, int max_initial, int* ts_state,
                                                             const int* __restrict__ pos_rows,
                                                             const int* __restrict__ limit, int* active,
                                                             int* __restrict__ tokens, float* __restrict__ logprob,
                                                             float inv_t, int top_k, const float* __restrict__ noise,
                                                             int64_t noise_ld) {
    __shared__ float red[16];
    __shared__ int redi[16];
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[2];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (!active[r]) {   // the whole block: uniform, before any barrier
        if (tid == 0) tokens[r] = eos;
        return;
    }
    const float* x = logits + (int64_t)r * ld;
    const float* q = noise + (int64_t)r * noise_ld;
    const SelectRow row(ts_state + 4 * r, V, ts_begin, no_ts, eos, max_initial);
    const float* bs = row.sn == 0 ? bias_begin : bias;
    // the thread's scores, indices tid, tid + 1024, ...: loaded once, every later pass runs on registers (the masks
    // applied here; beyond V: -inf, which no pass below counts as a score)
    float s[SAMPLE_PER_THREAD];
    const float* bsrc = bs ? bs : x;
#pragma unroll
    for (int u0 = 0; u0 < SAMPLE_PER_THREAD; u0 += 8) {   // eight logits and biases in flight, as select_for_each
        float xv[8], bv[8];
#pragma unroll
        for (int u = u0; u < min(u0 + 8, SAMPLE_PER_THREAD); ++u) {
            const int ii = min(tid + u * 1024, V - 1);
            xv[u - u0] = x[ii];
            bv[u - u0] = bsrc[ii];
        }
#pragma unroll
        for (int u = u0; u < min(u0 + 8, SAMPLE_PER_THREAD); ++u) {
            const int i = tid + u * 1024;
            // + 0.f: a score of -0.0 becomes +0.0 (equal as floats, one key)
            s[u] = (i < V && !row.masked(i)) ? xv[u - u0] + (bs ? bv[u - u0] : 0.f) + 0.f : -INFINITY;
        }
        __builtin_amdgcn_sched_barrier(0);   // or all 102 loads are issued at once and the scores spill
    }
    // f(i, s_i) over the thread's indices in ascending order
    auto scores = [&](auto&& f) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < SAMPLE_PER_THREAD; ++u) f(tid + u * 1024, s[u]);
    };
    const SelectStats c = select_class_stats(row.tb, scores, red, redi);
    const float best = (c.force_ts || c.m_ts > c.m_text) ? c.m_ts : c.m_text;   // the maximum of the processed scores
    if (!(best > -INFINITY)) {   // block-uniform: the stats are the same in every thread
        if (tid == 0) select_finish(row, r, eos, -INFINITY, ts_state, pos_rows, limit, active, tokens, logprob);
        return;
    }
    if (c.force_ts) {   // the mass rule: every text token masked
#pragma unroll
        for (int u = 0; u < SAMPLE_PER_THREAD; ++u)
            if (tid + u * 1024 < row.tb) s[u] = -INFINITY;
    }
    // from here on the scores as their keys (okey_value gives a score back): the radix select's view, and no second
    // set of 51 registers
    unsigned key[SAMPLE_PER_THREAD];
#pragma unroll
    for (int u = 0; u < SAMPLE_PER_THREAD; ++u) key[u] = okey(s[u]);
    auto keys = [&](auto&& f) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < SAMPLE_PER_THREAD; ++u) f(tid + u * 1024, key[u]);
    };
    unsigned prefix = 0, known = 0, remaining = (unsigned)min(top_k, V);
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        unsigned run_bin = 0, run = 0;
        keys([&](int, unsigned k) {
            if ((k & known) != prefix) return;
            const unsigned b = (k >> shift) & 255u;
            if (run && b != run_bin) { atomicAdd(&hist[run_bin], run); run = 0; }
            run_bin = b;
            ++run;
        });
        if (run) atomicAdd(&hist[run_bin], run);
        __syncthreads();
        if (wid == 0) {   // lane l owns bins 255 - 4 l ... 252 - 4 l; the bin where the count from the top reaches `remaining`
            unsigned cnt[4], tot = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { cnt[j] = hist[255 - (4 * lane + j)]; tot += cnt[j]; }
            unsigned inc = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_up(inc, o, 64);
                if (lane >= o) inc += up;
            }
            unsigned above = inc - tot;
            if (above < remaining && remaining <= inc) {   // one lane: the keys that match number >= remaining
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (remaining <= above + cnt[j]) {
                        sel[0] = 255u - (4 * lane + j);
                        sel[1] = remaining - above;
                        break;
                    }
                    above += cnt[j];
                }
            }
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        known |= 255u << shift;
        remaining = sel[1];
    }
    // prefix = okey(kth); kept: finite and >= kth (no score is -0.0, so the keys order equal scores equally)
    const unsigned floor_key = max(prefix, okey(-INFINITY) + 1u);
    const float max_w = best * inv_t;
    float sw = 0.f, ss = 0.f;   // the kept set's sums: of the warped softmax, and of exp(s - max) for the log-prob
    keys([&](int, unsigned k) {
        if (k >= floor_key) {
            const float v = okey_value(k);
            sw += expf(v * inv_t - max_w);
            ss += __expf(v - best);
        }
    });
    const float sum_w = block_sum16(sw, red), sum_s = block_sum16(ss, red);
    float win = -1.f;   // p / q >= 0 for every kept index; a thread's indices ascend, so `>` keeps its lowest
    int iw = 0x7fffffff;
    keys([&](int i, unsigned k) {
        if (k >= floor_key) {
            float qi = q[i];
            if (!(qi > 0.f && qi < INFINITY)) qi = FLT_MIN;
            const float p = expf(okey_value(k) * inv_t - max_w) / sum_w / qi;
            if (p > win) { win = p; iw = i; }
        }
    });
    float pw;
    int tok;
    block_argmax16(win, iw, red, redi, pw, tok);
    if (tid != 0) return;
    float lp = -INFINITY;
    if (pw >= 0.f && tok >= 0 && tok < V)
        lp = x[tok] + (bs ? bs[tok] : 0.f) - (best + logf(sum_s));
    else
        tok = eos;
    select_finish(row, r, tok, lp, ts_state, pos_rows, limit, active, tokens, logprob);
}

// ---------------------------------------------------------------- the processors that read a row's token history
// RepetitionPenaltyLogitsProcessor then NoRepeatNGramLogitsProcessor (transformers 4.37.2 _get_logits_processor's first
// two, on the raw logits of a greedy or sample step), in place, in front of greedy_select_kernel / sample_select_kernel,
// whose bias and rules are the processors after them.  One block per row; the work is the row's history (at most
// hist_ld <= CBW_HISTORY_MAX_LD tokens, staged in LDS clamped into [0, V)), not a pass over V.
//   upkeep: len = hist_len[r], the row's last token at position pos_rows[r].  len == pos + 1: the history is whole (a
//   slot just admitted, its prefix written by the caller).  len == pos: the row moved one position since the last call,
//   last_tokens[r] is appended.  Anything else, or an append that cannot be made (no last_tokens, len == hist_ld): the
//   row is left as it is -- no address is formed from a bad state.
//   penalty (p != 1): x[t] = x[t] < 0 ? x[t] * p : x[t] / p once per distinct token t: every entry's value is gathered
//   into LDS before any is scattered, so the entries of one token write equal values.
//   bans (n > 0, len + 1 >= n): x[hist[i + n - 1]] = -inf for every i in [0, len - n] whose n - 1 tokens equal the last
//   n - 1 (cbw.decoder.banned_ngram_tokens), behind a barrier: -inf wins over a penalised value.
constexpr int HR_THREADS = 256;

__global__ __launch_bounds__(HR_THREADS) void history_rules_kernel(float* __restrict__ logits, int V, int ld, int* hist,
                                                                   int hist_ld, int* hist_len,
                                                                   const int* __restrict__ last_tokens,
                                                                   const int* __restrict__ pos_rows,
                                                                   const int* __restrict__ active, float p, int n) {
    __shared__ int h[CBW_HISTORY_MAX_LD];
    __shared__ float hv[CBW_HISTORY_MAX_LD];
    const int r = blockIdx.x, tid = threadIdx.x;
    // block-uniform exits, all before the first barrier and before hist_len[r] is written
    if (!active[r] || hist_ld < 1 || hist_ld > CBW_HISTORY_MAX_LD) return;
    const int len = hist_len[r], pos = pos_rows[r];
    if (len < 0 || len > hist_ld) return;
    const bool append = len == pos;
    if (append ? (!last_tokens || len >= hist_ld) : len - 1 != pos) return;
    int* hr = hist + (int64_t)r * hist_ld;
    float* x = logits + (int64_t)r * ld;
    const int last = append ? last_tokens[r] : 0;
    const int L = len + (append ? 1 : 0);   // <= hist_ld
    for (int i = tid; i < L; i += HR_THREADS) h[i] = min(max(i < len ? hr[i] : last, 0), V - 1);
    __syncthreads();   // every thread has read hist_len[r]
    if (append && tid == 0) {
        hr[len] = last;
        hist_len[r] = L;
    }
    if (p != 1.f) {
        for (int i = tid; i < L; i += HR_THREADS) hv[i] = x[h[i]];
        __syncthreads();
        for (int i = tid; i < L; i += HR_THREADS) {
            const float v = hv[i];
            x[h[i]] = v < 0.f ? v * p : __fdiv_rn(v, p);   // round to nearest, as torch and numpy divide
        }
        __syncthreads();   // the penalised values are written before a ban overwrites one
    }
    if (n > 0 && L + 1 >= n) {
        const int* tail = h + (L - n + 1);   // the last n - 1 tokens
        for (int i = tid; i <= L - n; i += HR_THREADS) {
            bool same = true;
            for (int j = 0; j < n - 1; ++j) same = same && h[i + j] == tail[j];
            if (same) x[h[i + n - 1]] = -INFINITY;
        }
    }
}

// ---------------------------------------------------------------- beam bookkeeping on the GPU
// One HF 4.37 beam-search step's next-beam choice (cbw/generate.py BeamProcess.process; transformers
// BeamSearchScorer.process): the B*k candidates beam_scores[r] + lp[r][j] (f64, the host's Python floats),
// sorted by (score desc, row, token), truncated to k; EOS candidates are left to the host's hypotheses (it
// replays this step from the logged candidates); the first B non-EOS candidates become the next beams.  One
// thread: at most 16 x 16 candidates.  Timestamp-rule state per row {n, t1, t2, last_ts} of the tokens at
// positions >= begin (count != 0), gathered from the parent rows, and the cbw_timestamp_rules state derived
// from it.
// One workgroup of 256 threads: candidate c = (row c / k, slot c % k) is ranked by comparing it with every other
// candidate under the total order (score desc, row asc, token asc) -- the ranks < k are exactly the top k the
// bounded insertion sort of the previous single-thread version produced (the order is total: a row's top-k tokens
// are distinct) -- then thread 0 walks those <= 16 entries from LDS.  (The single-thread version indexed private
// arrays dynamically, i.e. through scratch: 43 us per decode step at 5 beams.)
__global__ __launch_bounds__(256) void beam_select_kernel(const float* __restrict__ lp, const int* __restrict__ idx,
                                                          int B, int k, int eos, double* __restrict__ beam_scores,
                                                          double* __restrict__ cand_score, int* __restrict__ cand_row,
                                                          int* __restrict__ cand_tok, int* __restrict__ tokens,
                                                          int* __restrict__ parents, int* __restrict__ ok,
                                                          int* __restrict__ ts_state, int* __restrict__ st_out,
                                                          int ts_begin, int count) {
    __shared__ double c_sc[256];
    __shared__ int c_r[256], c_t[256];
    __shared__ double s_cs[16];
    __shared__ int s_cr[16], s_ct[16], s_st[16][4];
    const int tid = threadIdx.x, nall = B * k;
    if (tid < nall) {
        const int r = tid / k;
        c_sc[tid] = beam_scores[r] + (double)lp[tid];
        c_r[tid] = r;
        c_t[tid] = idx[tid];
    }
    if (tid < 4 * B) s_st[tid >> 2][tid & 3] = ts_state[tid];
    __syncthreads();
    if (tid < nall) {
        const double sc = c_sc[tid];
        const int r = c_r[tid], tok = c_t[tid];
        int rank = 0;
        for (int j = 0; j < nall; ++j) {
            const double sj = c_sc[j];
            const int rj = c_r[j], tj = c_t[j];
            rank += (sj > sc || (sj == sc && (rj < r || (rj == r && tj < tok)))) ? 1 : 0;
        }
        if (rank < k) {
            s_cs[rank] = sc;
            s_cr[rank] = r;
            s_ct[rank] = tok;
        }
    }
    __syncthreads();
    if (tid != 0) return;
    const int n = nall < k ? nall : k;
    int nb = 0;
    double nscore[16];
    int ntok[16], nrow[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {   // fixed trip count: the arrays stay in registers
        if (i < n && nb < B && s_ct[i] != eos) {
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (b == nb) { nscore[b] = s_cs[i]; ntok[b] = s_ct[i]; nrow[b] = s_cr[i]; }
            ++nb;
        }
    }
    for (int i = 0; i < n; ++i) { cand_score[i] = s_cs[i]; cand_row[i] = s_cr[i]; cand_tok[i] = s_ct[i]; }
    *ok = nb == B ? 1 : 0;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        if (b >= B) break;
        const int pr = b < nb ? nrow[b] : 0, t = b < nb ? ntok[b] : eos;
        beam_scores[b] = b < nb ? nscore[b] : -1e9;
        tokens[b] = t;
        parents[b] = pr;
        int sn = s_st[pr][0], t1 = s_st[pr][1], t2 = s_st[pr][2], lts = s_st[pr][3];
        if (count) {
            ++sn;
            t2 = t1;
            t1 = t;
            if (t >= ts_begin) lts = t;
        }
        ts_state[4 * b] = sn; ts_state[4 * b + 1] = t1; ts_state[4 * b + 2] = t2; ts_state[4 * b + 3] = lts;
        const TsRuleState rs = ts_rule_state(sn, t1, t2, lts, ts_begin);
        st_out[4 * b] = rs.last_ts;
        st_out[4 * b + 1] = rs.penult_ts;
        st_out[4 * b + 2] = rs.ts_floor;
        st_out[4 * b + 3] = rs.at_begin;
    }
}
}  // namespace

hipError_t cbw_beam_select_launch(const float* lp, const int* idx, int B, int k, int eos, double* beam_scores,
                                  double* cand_score, int* cand_row, int* cand_tok, int* tokens, int* parents, int* ok,
                                  int* ts_state, int* st_out, int ts_begin, int count, hipStream_t st) {
    if (B < 1 || B > 16 || k < 1 || k > 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_select_kernel, dim3(1), dim3(256), 0, st, lp, idx, B, k, eos, beam_scores, cand_score,
                       cand_row, cand_tok, tokens, parents, ok, ts_state, st_out, ts_begin, count);
    return hipGetLastError();
}

static bool topk_split_enabled() {   // CBW_TOPK_SPLIT=0 runs the one-pass, one-workgroup-per-row kernel (A/B)
    const char* e = getenv("CBW_TOPK_SPLIT");
    return !(e && atoi(e) == 0);
}

hipError_t cbw_logprob_topk_launch(const float* logits, int B, int V, int ld, const float* bias, int64_t bias_ld,
                                   int k, float* lp, int* idx, hipStream_t st) {
    if (k < 1 || k > TK_MAX || B < 1 || V < 1) return hipErrorInvalidValue;
    if (!topk_split_enabled()) {
        hipLaunchKernelGGL(logprob_topk_kernel, dim3(B), dim3(1024), 0, st, logits, V, ld, bias, bias_ld, k, lp, idx);
        return hipGetLastError();
    }
    // chunk partials in a per-device scratch owned by the library (grow-only, stream-ordered reuse)
    static thread_local std::map<int, std::pair<float*, size_t>> scratch;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const int C = std::min(TK_CHUNKS, V);
    const int chunk = (V + C - 1) / C;
    const size_t need = (size_t)B * C * (2 * TK_MAX + 2) * sizeof(float);
    auto& sc = scratch[dev];
    if (sc.second < need) {
        if (sc.first) {
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
            (void)hipFree(sc.first);
            sc = {nullptr, 0};
        }
        if ((e = hipMalloc((void**)&sc.first, need)) != hipSuccess) return e;
        sc.second = need;
    }
    hipLaunchKernelGGL(topk_chunk_kernel, dim3(C, B), dim3(256), 0, st, logits, V, ld, bias, bias_ld, k, chunk,
                       sc.first);
    hipLaunchKernelGGL(topk_merge_kernel, dim3(B), dim3(64), 0, st, sc.first, C, k, lp, idx);
    return hipGetLastError();
}

hipError_t cbw_timestamp_rules_launch(const float* logits, int B, int V, int ld, const float* bias, const int* state,
                                      int ts_begin, int no_ts, int eos, int max_initial, float* bias_out,
                                      hipStream_t st) {
    hipLaunchKernelGGL(timestamp_rules_kernel, dim3(B), dim3(1024), 0, st, logits, V, ld, bias, state, ts_begin, no_ts,
                       eos, max_initial, bias_out);
    return hipGetLastError();
}

hipError_t cbw_greedy_select_launch(const float* logits, int B, int V, int ld, const float* bias,
                                    const float* bias_begin, int ts_begin, int no_ts, int eos, int max_initial,
                                    int* ts_state, const int* pos_rows, const int* limit, int* active, int* tokens,
                                    float* logprob, hipStream_t st) {
    if (B < 1 || B > 16 || V < 1 || ld < V) return hipErrorInvalidValue;
    hipLaunchKernelGGL(greedy_select_kernel, dim3(B), dim3(1024), 0, st, logits, V, ld, bias, bias_begin, ts_begin,
                       no_ts, eos, max_initial, ts_state, pos_rows, limit, active, tokens, logprob);
    return hipGetLastError();
}

hipError_t cbw_history_rules_launch(float* logits, int B, int V, int ld, int* hist, int hist_ld, int* hist_len,
                                    const int* last_tokens, const int* pos_rows, const int* active,
                                    float repetition_penalty, int no_repeat_ngram_size, hipStream_t st) {
    if (B < 1 || B > 16 || V < 1 || ld < V || hist_ld < 1 || hist_ld > CBW_HISTORY_MAX_LD ||
        !(repetition_penalty > 0.f) || !(repetition_penalty < INFINITY) || no_repeat_ngram_size < 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(history_rules_kernel, dim3(B), dim3(HR_THREADS), 0, st, logits, V, ld, hist, hist_ld, hist_len,
                       last_tokens, pos_rows, active, repetition_penalty, no_repeat_ngram_size);
    return hipGetLastError();
}

hipError_t cbw_sample_select_launch(const float* logits, int B, int V, int ld, const float* bias,
                                    const float* bias_begin, int ts_begin, int no_ts, int eos, int max_initial,
                                    int* ts_state, const int* pos_rows, const int* limit, int* active, int* tokens,
                                    float* logprob, float temperature, int top_k, const float* noise,
                                    int64_t noise_ld, hipStream_t st) {
    if (B < 1 || B > 16 || V < 1 || V > CBW_SAMPLE_MAX_V || ld < V || noise_ld < V || top_k < 1 || !(temperature > 0.f) ||
        !(temperature < INFINITY))
        return hipErrorInvalidValue;
    // scores * (1 / T) in fp32, as torch divides a device tensor by a host scalar
    hipLaunchKernelGGL(sample_select_kernel, dim3(B), dim3(1024), 0, st, logits, V, ld, bias, bias_begin, ts_begin,
                       no_ts, eos, max_initial, ts_state, pos_rows, limit, active, tokens, logprob,
                       1.0f / temperature, top_k, noise, noise_ld);
    return hipGetLastError();
}
