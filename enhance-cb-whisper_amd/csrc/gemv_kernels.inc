// The two decode-step GEMV kernels of gemv.hip, which includes this text twice: with GEMV_WIDE 0 as gemv_kernel /
// gemv_dot_kernel (one launch = all M <= 16 rows; the text is then what the compiler saw before the wide launch
// existed, so those kernels keep their code), and with GEMV_WIDE 1 as gemv_wide_kernel / gemv_dot_wide_kernel (a
// workgroup = one row group of a launch over up to 80 rows: gemv_wide_group moves the row-indexed operands first).
#if GEMV_WIDE
#define GEMV_KERNEL gemv_wide_kernel
#define GEMV_DOT_KERNEL gemv_dot_wide_kernel
#define GEMV_COLUMN_BLOCK(a) gemv_wide_group(a)
#else
#define GEMV_KERNEL gemv_kernel
#define GEMV_DOT_KERNEL gemv_dot_kernel
#define GEMV_COLUMN_BLOCK(a) blockIdx.x
#endif

// LN: the LayerNorm-prologue instance (K <= 1280 -> at most 8 waves, so a wider register budget)
template <bool LN>
__global__ __launch_bounds__(LN ? 512 : 1024) void GEMV_KERNEL(GemvArgs a) {
    const int cb = GEMV_COLUMN_BLOCK(a);
    __shared__ f32x4 red[16][64];
    extern __shared__ __attribute__((aligned(16))) char gv_dyn[];   // LN prologue: bf16 [M][K + 8]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int W = blockDim.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int KS = a.K / 32;
    const int k_lo = w * KS / W, k_hi = (w + 1) * KS / W;
    const int c0 = cb * 16;
    const int n_ld = min(c0 + fr, a.N - 1);
    const bf16* wr = a.w + (int64_t)n_ld * a.K + fq * 8;
    const bool row_ok = fr < a.M;
    constexpr bool ln = LN;
    const int pitch = a.K + 8;
    const bf16* xr = ln ? (const bf16*)gv_dyn + (row_ok ? fr : 0) * pitch + fq * 8
                        : a.x + (int64_t)(row_ok ? fr : 0) * a.ldx + fq * 8;

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    bf16x8 wv[GV_BATCH], xv[GV_BATCH];
    int k0 = k_lo;
#pragma unroll
    for (int j = 0; j < GV_BATCH; ++j)
        if (k0 + j < k_hi) wv[j] = __builtin_nontemporal_load((const bf16x8*)(wr + (k0 + j) * 32));   // wave-uniform
    if (ln) {
        // LayerNorm of the M rows into LDS while the first weight burst is in flight: wave w takes rows
        // w, w + W, ..., with layernorm_kernel's arithmetic (same per-lane order, same wave reduction)
        bf16* xs = (bf16*)gv_dyn;
        for (int r = w; r < a.M; r += W) {
            const float* xrow = a.xf + (int64_t)r * a.ldx;
            f32x4 v[GV_LN_MAXK / 256], gg[GV_LN_MAXK / 256], bb[GV_LN_MAXK / 256];
#pragma unroll
            for (int c = 0; c < GV_LN_MAXK / 256; ++c) {   // row, gamma and beta in one round trip
                const int i = lane * 4 + c * 256;
                if (i < a.K) {
                    v[c] = *(const f32x4*)(xrow + i);
                    gg[c] = *(const f32x4*)(a.ln_g + i);
                    bb[c] = *(const f32x4*)(a.ln_b + i);
                }
            }
            float sm = 0.f;
#pragma unroll
            for (int c = 0; c < GV_LN_MAXK / 256; ++c)
                if (lane * 4 + c * 256 < a.K) sm += v[c][0] + v[c][1] + v[c][2] + v[c][3];
            const float mean = wave_sum(sm) / a.K;
            float ss = 0.f;
#pragma unroll
            for (int c = 0; c < GV_LN_MAXK / 256; ++c)
                if (lane * 4 + c * 256 < a.K)
#pragma unroll
                    for (int q = 0; q < 4; ++q) ss += (v[c][q] - mean) * (v[c][q] - mean);
            const float rstd = rsqrtf(wave_sum(ss) / a.K + a.ln_eps);
#pragma unroll
            for (int c = 0; c < GV_LN_MAXK / 256; ++c) {
                const int i = lane * 4 + c * 256;
                if (i < a.K) {
                    bf16x4 ob;
#pragma unroll
                    for (int q = 0; q < 4; ++q) ob[q] = f2bf((v[c][q] - mean) * rstd * gg[c][q] + bb[c][q]);
                    *(bf16x4*)(xs + r * pitch + i) = ob;
                }
            }
        }
        __syncthreads();
    }
    for (;;) {
#pragma unroll
        for (int j = 0; j < GV_BATCH; ++j)
            if (k0 + j < k_hi) xv[j] = row_ok ? *(const bf16x8*)(xr + (k0 + j) * 32) : bf16x8{};
#pragma unroll
        for (int j = 0; j < GV_BATCH; ++j)
            if (k0 + j < k_hi) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[j], xv[j], acc, 0, 0, 0);
        k0 += GV_BATCH;
        if (k0 >= k_hi) break;
#pragma unroll
        for (int j = 0; j < GV_BATCH; ++j)
            if (k0 + j < k_hi) wv[j] = __builtin_nontemporal_load((const bf16x8*)(wr + (k0 + j) * 32));
    }
    if (W > 1) {
        red[w][lane] = acc;
        __syncthreads();
        if (w != 0) return;
        for (int ww = 1; ww < W; ++ww) acc += red[ww][lane];
    }
    // lane holds C^T[n = c0 + 4 fq + q][m = fr]
    const int m = fr, n = c0 + fq * 4;
    if (!row_ok || n >= a.N) return;
    f32x4 v = acc;
    if (a.bias) v += *(const f32x4*)(a.bias + n);
    float rv[4] = {0.f, 0.f, 0.f, 0.f};
    const bool has_res = a.res != nullptr;
    if (has_res) {
        if (a.flags & CBW_EPI_RES_F32) {
            const f32x4 r = *(const f32x4*)((const float*)a.res + (int64_t)m * a.res_ld + n);
#pragma unroll
            for (int q = 0; q < 4; ++q) rv[q] = r[q];
        } else {
            const bf16x4 r = *(const bf16x4*)((const bf16*)a.res + (int64_t)m * a.res_ld + n);
#pragma unroll
            for (int q = 0; q < 4; ++q) rv[q] = bf2f(r[q]);
        }
        if (!(a.flags & CBW_EPI_RES_AFTER_ACT))
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] += rv[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (a.flags & CBW_EPI_RELU) v[q] = fmaxf(v[q], 0.f);
        else if (a.flags & CBW_EPI_GELU) v[q] = gelu_erf(v[q]);
        if (has_res && (a.flags & CBW_EPI_RES_AFTER_ACT)) v[q] += rv[q];
    }
    if (a.flags & CBW_EPI_OUT_F32) {
        *(f32x4*)((float*)a.y + (int64_t)m * a.ldy + n) = v;
    } else {
        bf16x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = f2bf(v[q]);
        *(bf16x4*)((bf16*)a.y + (int64_t)m * a.ldy + n) = o;
        if (a.kv_k && n >= a.kv_D) {   // 4 columns never straddle the q/k/v boundaries (kv_D % 4 == 0)
            const int64_t po = a.kv_pos ? (int64_t)a.kv_pos[a.kv_pos_rows ? m : 0] * a.kv_D : 0;
            bf16* dst = (n < 2 * a.kv_D ? a.kv_k + (n - a.kv_D) : a.kv_v + (n - 2 * a.kv_D)) + po;
            *(bf16x4*)(dst + (int64_t)m * a.kv_ld) = o;
        }
    }
}

// CPW = output columns per wave: 2 (a column's K over 32 lanes) or 1 (over all 64 lanes: half the weight bytes per
// workgroup, twice the workgroups -- the K 5120 fc2, whose 160 workgroups each staged 51 KB of rows and streamed 80 KB)
// KS = K stages of the DMA'd rows (no LayerNorm): the rows are staged KS times, K / KS columns at a time, so the 16-row
// K 5120 fc2 needs 80 instead of 154 KB of LDS (two workgroups per CU: its 320 workgroups in one round instead of
// two); the sums run over j in the same order, so the results are those of KS = 1 (15-row step 3.44 -> 3.13 ms, r03aj)
// WV = computing waves per workgroup (4, or 8 for the 9..16-row instantiation: each wave's LayerNorm prologue then
// normalises 2 rows instead of 4, and every column is computed by the same lanes in the same order as with 4; 15-row
// step 3.13 -> 2.89 ms, r03al)
template <bool LN, int NJ, int CPW = 2, int MAXM = GD_MAXM, int KS = 1, int WV = 4>
__global__ __launch_bounds__(WV * 64) void GEMV_DOT_KERNEL(GemvArgs a) {   // NJ = K / 256; M <= MAXM
    const int cb = GEMV_COLUMN_BLOCK(a);
    extern __shared__ __attribute__((aligned(16))) char gv_dyn[];   // bf16 [M][K + 8]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int LANES = 64 / CPW, STEP = LANES * 8;   // lanes per column, elements per load step
    constexpr int K = NJ * 256, NL = K / STEP;          // loads per lane
    const int half = CPW == 2 ? lane >> 5 : 0, hl = lane & (LANES - 1);
    static_assert(KS == 1 || (!LN && NL % KS == 0), "K stages: DMA'd rows");
    constexpr int KP = K / KS, NLS = NL / KS;           // columns of K per stage, loads per lane per stage
    const int M = a.M, pitch = LN ? K + 8 : KP;   // the LayerNorm prologue writes padded rows, the DMA packed ones
    const int col = cb * (WV * CPW) + w * CPW + half;
    const bf16* wr = a.w + (int64_t)min(col, a.N - 1) * K + hl * 8;
    // the epilogue's operands (bias, residual) do not depend on the sums: requested before anything else, as raw
    // words (no conversion at a branch join, which would wait for the load there), so the epilogue does not start
    // with a dependent round trip
    const int m_e = min(hl, M - 1);
    const bool has_res = a.res != nullptr, res32 = (a.flags & CBW_EPI_RES_F32) != 0;
    const int n_e = min(col, a.N - 1);
    const float bias_raw = *(a.bias ? a.bias + n_e : (const float*)a.w);
    unsigned res_raw = 0;
    if (has_res) {
        const char* rp = (const char*)a.res + ((int64_t)m_e * a.res_ld + n_e) * (res32 ? 4 : 2);
        res_raw = res32 ? *(const unsigned*)rp : (unsigned)*(const unsigned short*)rp;
    }
    // the activations are requested next (L2 round trip), then every weight load of the lane's slice: the
    // counted waits of the activation staging then do not wait behind the weight stream
    bf16x8 wv[NL];
    bf16* xs = (bf16*)gv_dyn;
    if constexpr (LN) {   // LayerNorm of the M rows (layernorm_kernel's arithmetic): wave w takes rows w, w + WV, ...
        constexpr int NC = K / 256;
        static_assert(K <= GV_LN_MAXK, "LayerNorm prologue width");
        constexpr int HS = MAXM / WV;   // row slots per wave: rows w, w + WV, ...
        static_assert(HS >= 1, "row slots");
        f32x4 v[HS][NC], gg[NC], bb[NC];
#pragma unroll
        for (int h = 0; h < HS; ++h) {
            const int r = min(w + WV * h, M - 1);
            const float* xrow = a.xf + (int64_t)r * a.ldx;
#pragma unroll
            for (int c = 0; c < NC; ++c) v[h][c] = *(const f32x4*)(xrow + lane * 4 + c * 256);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            gg[c] = *(const f32x4*)(a.ln_g + lane * 4 + c * 256);
            bb[c] = *(const f32x4*)(a.ln_b + lane * 4 + c * 256);
        }
#pragma unroll
        for (int j = 0; j < NL; ++j) wv[j] = __builtin_nontemporal_load((const bf16x8*)(wr + j * STEP));
        // both row slots normalised unconditionally (a slot past M repeats row M - 1, its result is not stored): with
        // a conditional second row the compiler sank that row's loads (and gamma / beta) behind the first row's
        // reductions -- three round trips instead of one
#pragma unroll
        for (int h = 0; h < HS; ++h) {
            const int r = w + WV * h;
            float sm = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) sm += v[h][c][0] + v[h][c][1] + v[h][c][2] + v[h][c][3];
            const float mean = wave_sum_x(sm) / K;
            float ss = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int q = 0; q < 4; ++q) ss += (v[h][c][q] - mean) * (v[h][c][q] - mean);
            const float rstd = rsqrtf(wave_sum_x(ss) / K + a.ln_eps);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                bf16x4 ob;
#pragma unroll
                for (int q = 0; q < 4; ++q) ob[q] = f2bf((v[h][c][q] - mean) * rstd * gg[c][q] + bb[c][q]);
                if (r < M) *(bf16x4*)(xs + r * pitch + lane * 4 + c * 256) = ob;
            }
        }
    } else {   // the M rows DMA'd straight into LDS (global_load_lds: no registers), every piece in flight at once,
        // then the weight stream; one counted wait for the DMAs leaves the weight loads in flight.  (Staged through
        // registers, the compiler sank each row load next to its LDS store and waited for it before issuing the
        // next: the rows arrived one round trip at a time.)
        const int total = M * KP * 2;                // bytes, rows packed [M][KP] (pitch KP): the first K stage
        const int pieces = (total + 1023) >> 10;     // 1 KB per wave instruction; LDS holds whole pieces
        const int e = lane * 8;                      // this lane's first element within a piece
        for (int pc = w; pc < pieces; pc += WV) {
            const int el = min(pc * 512 + e, M * KP - 8), r = el / KP, c = el - r * KP;
            __builtin_amdgcn_global_load_lds((const void*)(a.x + (int64_t)r * a.ldx + c), (void*)(gv_dyn + pc * 1024),
                                             16, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NL; ++j) wv[j] = __builtin_nontemporal_load((const bf16x8*)(wr + j * STEP));
        // the DMAs were issued before the NL weight loads: vmcnt(NL) retires them (in-order completion)
        wait_vm<NL>();
    }
    __syncthreads();
    float acc[MAXM];
#pragma unroll
    for (int r = 0; r < MAXM; ++r) acc[r] = 0.f;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        if constexpr (KS > 1) {
            if (j > 0 && j % NLS == 0) {   // the next K stage's rows into the same LDS, once every wave has read these
                __syncthreads();
                const int pieces = (M * KP * 2 + 1023) >> 10, e = lane * 8, k0 = (j / NLS) * KP;
                for (int pc = w; pc < pieces; pc += WV) {
                    const int el = min(pc * 512 + e, M * KP - 8), r = el / KP, c = el - r * KP;
                    __builtin_amdgcn_global_load_lds((const void*)(a.x + (int64_t)r * a.ldx + k0 + c),
                                                     (void*)(gv_dyn + pc * 1024), 16, 0, 0);
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
        }
        const bf16x8 wj = wv[j];
#pragma unroll
        for (int r = 0; r < MAXM; ++r) {
            if (r >= M) continue;
            const bf16x8 xv = *(const bf16x8*)(xs + r * pitch + (j % NLS) * STEP + hl * 8);
#pragma unroll
            for (int p = 0; p < 4; ++p)
                acc[r] = __builtin_amdgcn_fdot2_f32_bf16(bf16x2v{wj[2 * p], wj[2 * p + 1]}, bf16x2v{xv[2 * p], xv[2 * p + 1]},
                                                         acc[r], false);
        }
    }
#pragma unroll
    for (int r = 0; r < MAXM; ++r)   // the lanes of each column: a half-wave, or the whole wave
        acc[r] = CPW == 2 ? half_wave_sum(acc[r]) : wave_sum_x(acc[r]);
    // lane hl = r of each column's lanes finishes row r of its column
    float v = 0.f;
#pragma unroll
    for (int r = 0; r < MAXM; ++r)
        if (hl == r) v = acc[r];
    const int m = hl, n = col;
    if (m >= M || n >= a.N) return;
    if (a.bias) v += bias_raw;
    float rv = 0.f;
    if (has_res) {
        rv = res32 ? __uint_as_float(res_raw) : bf2f(__builtin_bit_cast(bf16, (unsigned short)res_raw));
        if (!(a.flags & CBW_EPI_RES_AFTER_ACT)) v += rv;
    }
    if (a.flags & CBW_EPI_RELU) v = fmaxf(v, 0.f);
    else if (a.flags & CBW_EPI_GELU) v = gelu_erf(v);
    if (has_res && (a.flags & CBW_EPI_RES_AFTER_ACT)) v += rv;
    if (a.flags & CBW_EPI_OUT_F32) {
        ((float*)a.y)[(int64_t)m * a.ldy + n] = v;
    } else {
        const bf16 o = f2bf(v);
        ((bf16*)a.y)[(int64_t)m * a.ldy + n] = o;
        if (a.kv_k && n >= a.kv_D) {
            const int64_t po = a.kv_pos ? (int64_t)a.kv_pos[a.kv_pos_rows ? m : 0] * a.kv_D : 0;
            bf16* dst = (n < 2 * a.kv_D ? a.kv_k + (n - a.kv_D) : a.kv_v + (n - 2 * a.kv_D)) + po;
            dst[(int64_t)m * a.kv_ld] = o;
        }
    }
}

#undef GEMV_KERNEL
#undef GEMV_DOT_KERNEL
#undef GEMV_COLUMN_BLOCK
