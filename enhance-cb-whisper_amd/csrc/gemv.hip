// Skinny GEMM ("GEMV") for the Whisper decoder step on gfx950: y[m][n] = act(sum_k x[m][k] W[n][k] + b[n]
// (+ res[m][n])) for M <= 16 rows (the beams of one decode step), every decoder Linear (self q/k/v + out,
// cross q + out, fc1, fc2) and the vocabulary projection (HF WhisperDecoderLayer / proj_out as run by
// PBAWhisper.generate's beam search, src/model/pba_whisper.py:283-338 via HF 4.37 _beam_search).
//
// A decode step reads every decoder weight once (large-v3: 1.6 GB) for 5 rows, so it is HBM- and
// latency-bound; the 128-row implicit-GEMM tiles the step used before put 10-40 workgroups on a
// 1280-wide Linear and reached 0.15 TB/s.  Here:
//   * workgroup = 16 output columns x the whole K, split over its W waves (W = 1..16, so that a wave
//     owns <= 10 k-steps of 32): every weight byte of the workgroup's 16 rows is requested in one burst,
//     16 bytes per lane, before the first MFMA;
//   * each wave runs C^T = W . x^T on mfma_f32_16x16x32_bf16 over its K-slice: the weight fragment
//     (16 columns x 32 k) is the A operand, the rows (zero-padded to 16) the B operand;
//   * the W partial accumulators meet in LDS and wave 0 sums them in wave order (deterministic), then
//     applies bias, residual, activation and the output type.  One launch per Linear, no global
//     partials, no atomics.
// More than 16 rows (cbw_gemv_wide, up to 80: the windows of a batch of short clips): row groups of 16 in one launch,
// each group the same kernel text on its rows (gemv_kernels.inc holds the two kernels, compiled here twice).
#include "cbw_common.h"
#include "cbw_kernels.h"
#include "gemv_route.h"

namespace {

// GV_BATCH, GV_LN_MAXK, GV_LN_LDS, GD_MAXM, GD_LDS16: gemv_route.h (the dispatch sizes its launches by them)
static_assert(sizeof(f32x4) * 16 * 64 + GV_LN_LDS <= GV_LDS_DEFAULT, "gemv_kernel<true>: red[16][64] + the padded rows");
static_assert(GV_LN_MAXK % 256 == 0 && gemv_waves(GV_LN_MAXK) * 64 <= 512, "gemv_kernel<true>: launch bounds");
static_assert(gemv_waves(16 * GV_BATCH * 32) == 16 && gemv_waves(GV_BATCH * 32) == 1, "a wave owns <= GV_BATCH k-steps");

// The wide launch (cbw_gemv_wide): 17..80 rows as ceil(M / 16) row groups in one launch, the groups a second grid
// coordinate.  Group g is the kernel body below applied to rows [16 g, min(16 g + 16, M)): the row-indexed operands
// move by the group's rows, the group's row count replaces M, and nothing else in the arithmetic changes -- a row
// carries the bits cbw_gemv gives it in a launch over its 16-row slice.  Returns the workgroup's column block.
// a.wide_gx: the groups are grid x (neighbouring workgroups share a column block's weights), else grid y.
CBW_DEV int gemv_wide_group(GemvArgs& a) {
    const int g = a.wide_gx ? blockIdx.x : blockIdx.y, r0 = g * 16;
    if (a.x) a.x += (int64_t)r0 * a.ldx;
    if (a.xf) a.xf += (int64_t)r0 * a.ldx;
    if (a.res) a.res = (const char*)a.res + (int64_t)r0 * a.res_ld * ((a.flags & CBW_EPI_RES_F32) ? 4 : 2);
    a.y = (char*)a.y + (int64_t)r0 * a.ldy * ((a.flags & CBW_EPI_OUT_F32) ? 4 : 2);
    if (a.kv_k) {
        a.kv_k += (int64_t)r0 * a.kv_ld;
        a.kv_v += (int64_t)r0 * a.kv_ld;
        if (a.kv_pos && a.kv_pos_rows) a.kv_pos += r0;
    }
    a.M = min(16, a.M - r0);
    return a.wide_gx ? blockIdx.y : blockIdx.x;
}

// VALU variant for the beam rows of a decode step (M <= 16, K % 256 == 0): 2 * WV output columns per workgroup (one
// per wave for the K 5120 fc2), each column's K split over 32 (64) lanes in interleaved 16-byte chunks (a half-wave
// reads 512 contiguous bytes of the weight row per load), every load of the lane's slice issued at once; the M rows
// staged in LDS (LayerNorm prologue or a DMA copy), dot products on v_dot2_f32_bf16, the partial sums reduced by lane
// exchanges in a fixed order (deterministic).  Versus the MFMA kernel above (16 columns per workgroup, 16 - M of its
// 16 B-operand rows padding): 2x the workgroups at the decode step's N (160 at D 1280 instead of 80), so twice the
// CUs stream the weights; the step is latency-bound on the chain of its ~300 launches.
// GD_MAXM = 8 rows (K <= 5120); 9..16 rows: the 16-row instantiation, its rows staged in up to GD_LDS16 = 158 KB of LDS
// (gfx950: 160 KB per workgroup)
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));

constexpr bool wait_vm_has(int n) {
    for (int c : GD_WAIT_COUNTS)
        if (c == n) return true;
    return false;
}

template <int N>
CBW_DEV void wait_vm() {   // s_waitcnt vmcnt(N) for the counts the kernel below uses
    static_assert(wait_vm_has(N), "count");   // GD_WAIT_COUNTS (gemv_route.h): the route check walks the same list
    if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if constexpr (N == 20) asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
    else if constexpr (N == 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else if constexpr (N == 32) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(40)" ::: "memory");
}

// the kernels: once for a launch over <= 16 rows, once as a row group of the wide launch
#define GEMV_WIDE 0
#include "gemv_kernels.inc"
#undef GEMV_WIDE
#define GEMV_WIDE 1
#include "gemv_kernels.inc"
#undef GEMV_WIDE

}  // namespace

int cbw_gemv_waves(int K) { return gemv_waves(K); }
bool cbw_gemv_ln_ok(int M, int K) { return gemv_ln_ok(M, K); }

namespace {
// One instantiation of the dot kernel, launched as the route says.  The route's template arguments for this
// instantiation's (rows, K, LN) must be this instantiation's: checked here at compile time, so the header cannot
// drift from the kernels.  raise_lds: above the 64 KB default the limit is raised once per kernel.
template <bool LN, int NJ, int CPW, int MAXM, int KS, int WV>
hipError_t dot_launch(const GemvRoute& r, const GemvArgs& a, hipStream_t st) {
    constexpr GemvRoute R = gemv_route(MAXM, 4, NJ * 256, LN);
    static_assert(R.kernel == GemvKernel::Dot && R.ln == LN && R.nj == NJ && R.cpw == CPW && R.maxm == MAXM &&
                      R.ks == KS && R.wv == WV && R.block == WV * 64 && R.cols == WV * CPW, "gemv_route.h");
    static_assert(LN || wait_vm_has(NJ * 256 / (512 / CPW)), "NL is one of wait_vm's counts");
    if (r.raise_lds) {
        static const bool once = hipFuncSetAttribute((const void*)gemv_dot_kernel<LN, NJ, CPW, MAXM, KS, WV>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, GD_LDS16) == hipSuccess;
        (void)once;
    }
    hipLaunchKernelGGL((gemv_dot_kernel<LN, NJ, CPW, MAXM, KS, WV>), dim3(r.grid), dim3(r.block), r.lds, st, a);
    return hipGetLastError();
}
}  // namespace

// Launches what gemv_route (gemv_route.h) says and nothing else.  The kernel family -- MFMA or dot -- depends on (K,
// LayerNorm prologue) alone, never on the row count, and within the dot family rows 0..7 run the same arithmetic in
// the 8-row and the 16-row instantiation (each row's sums are independent of M, of the wave count and of the K
// stages), so a step over several windows' beams gives each window's rows the values a step over that window alone
// gives, bit for bit (tests/test_gpu_gemv.py: every row count 1..16 at every width).  One column per wave for the K
// 5120 Linear (fc2, no LayerNorm); its 9..16-row rows staged in two K halves, its 7 and 8 rows (70 / 80 KB) under the
// raised LDS limit on the instantiation rows 1..6 run.
hipError_t cbw_gemv(const GemvArgs& a, hipStream_t st) {
    if (a.M < 1 || a.M > 16 || a.K % 32 || a.N % 4 || a.ldx % 8 || a.ldy % 4 || (a.res && a.res_ld % 4))
        return hipErrorInvalidValue;
    if (a.xf && (!a.ln_g || !a.ln_b || a.ldx % 4 || !cbw_gemv_ln_ok(a.M, a.K))) return hipErrorInvalidValue;
    if (a.kv_k && (!a.kv_v || a.kv_D % 4 || a.N != 3 * a.kv_D || a.kv_ld % 4 || (a.flags & CBW_EPI_OUT_F32)))
        return hipErrorInvalidValue;
    const GemvRoute r = gemv_route(a.M, a.N, a.K, a.xf != nullptr);
    if (r.kernel == GemvKernel::Mfma) {
        if (r.ln) hipLaunchKernelGGL(gemv_kernel<true>, dim3(r.grid), dim3(r.block), r.lds, st, a);
        else hipLaunchKernelGGL(gemv_kernel<false>, dim3(r.grid), dim3(r.block), r.lds, st, a);
        return hipGetLastError();
    }
    if (r.kernel != GemvKernel::Dot) return hipErrorInvalidValue;
#define GD_TRY(LN, NJ, CPW, MAXM, KS, WV)                                                         \
    if (r.ln == LN && r.nj == NJ && r.cpw == CPW && r.maxm == MAXM && r.ks == KS && r.wv == WV) \
        return dot_launch<LN, NJ, CPW, MAXM, KS, WV>(r, a, st);
#define GD_TRY_M(LN, NJ) GD_TRY(LN, NJ, 2, GD_MAXM, 1, 4) GD_TRY(LN, NJ, 2, 16, 1, 8)
    GD_TRY_M(true, 3) GD_TRY_M(true, 4) GD_TRY_M(true, 5)
    GD_TRY_M(false, 3) GD_TRY_M(false, 4) GD_TRY_M(false, 5) GD_TRY_M(false, 12) GD_TRY_M(false, 16)
    GD_TRY(false, 20, 1, GD_MAXM, 1, 4) GD_TRY(false, 20, 1, 16, 2, 8)
#undef GD_TRY_M
#undef GD_TRY
    return hipErrorInvalidValue;   // a route no instantiation matches: a missing kernel is an error
}

namespace {
template <bool LN, int NJ, int CPW, int KS>
hipError_t dot_wide_launch(const GemvWideRoute& w, const GemvArgs& a, hipStream_t st) {
    constexpr GemvRoute R = gemv_route(16, 4, NJ * 256, LN);   // the 16-slot instantiation dot_launch checks too
    static_assert(R.kernel == GemvKernel::Dot && R.cpw == CPW && R.ks == KS && R.maxm == 16 && R.wv == 8 && R.raise_lds,
                  "gemv_route.h");
    static const bool once = hipFuncSetAttribute((const void*)gemv_dot_wide_kernel<LN, NJ, CPW, 16, KS, 8>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, GD_LDS16) == hipSuccess;
    (void)once;
    hipLaunchKernelGGL((gemv_dot_wide_kernel<LN, NJ, CPW, 16, KS, 8>), dim3(w.grid_x, w.grid_y), dim3(w.group.block),
                       w.group.lds, st, a);
    return hipGetLastError();
}
}  // namespace

// Launches what gemv_wide_route says and nothing else: cbw_gemv's checks with 1 <= M <= GV_WIDE_ROWS, every group on
// the 16-slot kernel of its (K, LayerNorm) family.  Each group re-reads the Linear's weights.
hipError_t cbw_gemv_wide(const GemvArgs& a0, hipStream_t st, bool groups_fast) {
    GemvArgs a = a0;
    if (a.M < 1 || a.M > GV_WIDE_ROWS || a.K % 32 || a.N % 4 || a.ldx % 8 || a.ldy % 4 || (a.res && a.res_ld % 4))
        return hipErrorInvalidValue;
    if (a.xf && (!a.ln_g || !a.ln_b || a.ldx % 4 || !cbw_gemv_ln_ok(16, a.K))) return hipErrorInvalidValue;
    if (a.kv_k && (!a.kv_v || a.kv_D % 4 || a.N != 3 * a.kv_D || a.kv_ld % 4 || (a.flags & CBW_EPI_OUT_F32)))
        return hipErrorInvalidValue;
    const GemvWideRoute w = gemv_wide_route(a.M, a.N, a.K, a.xf != nullptr, groups_fast);
    if (w.groups < 1) return hipErrorInvalidValue;
    a.wide_gx = groups_fast ? 1 : 0;
    const GemvRoute& r = w.group;
    if (r.kernel == GemvKernel::Mfma) {
        const dim3 grid(w.grid_x, w.grid_y);
        if (r.ln) hipLaunchKernelGGL(gemv_wide_kernel<true>, grid, dim3(r.block), r.lds, st, a);
        else hipLaunchKernelGGL(gemv_wide_kernel<false>, grid, dim3(r.block), r.lds, st, a);
        return hipGetLastError();
    }
#define GDW_TRY(LN, NJ, CPW, KS) \
    if (r.ln == LN && r.nj == NJ && r.cpw == CPW && r.ks == KS) return dot_wide_launch<LN, NJ, CPW, KS>(w, a, st);
    GDW_TRY(true, 3, 2, 1) GDW_TRY(true, 4, 2, 1) GDW_TRY(true, 5, 2, 1)
    GDW_TRY(false, 3, 2, 1) GDW_TRY(false, 4, 2, 1) GDW_TRY(false, 5, 2, 1) GDW_TRY(false, 12, 2, 1)
    GDW_TRY(false, 16, 2, 1) GDW_TRY(false, 20, 1, 2)
#undef GDW_TRY
    return hipErrorInvalidValue;   // a missing kernel is an error
}
