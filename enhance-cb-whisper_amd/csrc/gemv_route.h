// Which kernel a decode-step Linear (cbw_gemv, gemv.hip) runs on, with which template arguments, grid, block and
// dynamic LDS: the whole dispatch as a pure host function of (M, N, K, LayerNorm prologue or not).  Plain C++17, no
// HIP include: tests/host/gemv_route_check.cpp checks on the CPU that every route is launchable, that the kernel
// family of a (K, LN) does not depend on the row count, and pins the routes of the shapes the decoders run.  cbw_gemv
// launches what gemv_route says and nothing else; gemv.hip ties the constants below to its own with static_asserts.
#pragma once
#include <stddef.h>

enum class GemvKernel { Invalid, Mfma, Dot };

struct GemvRoute {
    GemvKernel kernel = GemvKernel::Invalid;
    bool ln = false;   // the LayerNorm-prologue instantiation
    // gemv_dot_kernel<LN, NJ, CPW, MAXM, KS, WV>: K / 256, columns per wave, row slots, K stages of the DMA'd rows,
    // computing waves (all 0 for the MFMA kernel)
    int nj = 0, cpw = 0, maxm = 0, ks = 0, wv = 0;
    int waves = 0;     // gemv_kernel<LN>: the waves K is split over (0 for the dot kernel)
    int cols = 0;      // output columns per workgroup
    int grid = 0, block = 0;
    size_t lds = 0;    // dynamic LDS bytes of the launch
    // the launch must first raise the kernel's dynamic-LDS limit (to GD_LDS16): lds may then exceed GV_LDS_DEFAULT
    bool raise_lds = false;
    // the kernel as rocprofv3 names it, template arguments included: a string literal
    const char* name = "";
};

// ---- constants shared with gemv.hip (which asserts its own against these)
constexpr int GV_BATCH = 10;              // gemv_kernel: k-steps (of 32) in flight per wave
constexpr int GV_LN_MAXK = 1280;          // LayerNorm prologue: a row is <= 5 f32x4 per lane (Whisper d_model <= 1280)
constexpr int GV_LN_LDS = 48 * 1024;      // gemv_kernel<true>: + its 16 KB reduction buffer = the 64 KB default
constexpr int GV_LDS_DEFAULT = 64 * 1024; // dynamic LDS a launch may ask for without raising the limit
constexpr int GD_MAXM = 8;                // gemv_dot_kernel: rows of the 4-wave instantiation (9..16: MAXM 16, 8 waves)
constexpr int GD_LDS16 = 158 * 1024;      // the raised limit (gfx950: 160 KB per workgroup)
// the counts gemv_dot_kernel's wait_vm<NL> has an instruction for (NL = loads per lane = K / (512 / CPW))
constexpr int GD_WAIT_COUNTS[] = {3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40};

constexpr int gemv_waves(int K) {   // enough waves that each owns <= GV_BATCH k-steps (one burst of loads), at most 16
    const int ks = K / 32;
    int W = 1;
    while (W < 16 && (ks + W - 1) / W > GV_BATCH) W *= 2;
    return W;
}

// whether the LayerNorm prologue applies to this shape (either kernel: padded bf16 rows [M][K + 8] in LDS)
constexpr bool gemv_ln_ok(int M, int K) {
    return M >= 1 && M <= 16 && K % 32 == 0 && K <= GV_LN_MAXK && (size_t)M * (K + 8) * 2 <= (size_t)GV_LN_LDS;
}

// the widths gemv_dot_kernel is instantiated for: the d_model and ffn_dim of Whisper small, medium and large
constexpr bool gemv_dot_width(int K) {
    return K == 768 || K == 1024 || K == 1280 || K == 3072 || K == 4096 || K == 5120;
}

// "gemv_dot_kernel<LN, NJ, CPW, MAXM, KS, WV>" for the instantiated widths
#define CBW_GD_NAME_NJ(nj, pre, post)                                                                     \
    ((nj) == 3 ? pre "3" post : (nj) == 4 ? pre "4" post : (nj) == 5 ? pre "5" post : (nj) == 12 ? pre "12" post \
     : (nj) == 16 ? pre "16" post : pre "20" post)

// The route of y[M][N] = act(x[M][K] . W[N][K]^T ...), ln = with the LayerNorm prologue.  The kernel family depends on
// (K, ln) alone, never on M: a row's sums are then those of a step over that row alone, whatever the other rows of
// the step (cbw_decoder_step_rows' guarantee).  Within the dot family M picks the instantiation -- 1..8 rows: 8 row
// slots, 4 waves; 9..16: 16 slots, 8 waves -- whose rows 0..7 run the same arithmetic.
constexpr GemvRoute gemv_route(int M, int N, int K, bool ln) {
    GemvRoute r;
    if (M < 1 || M > 16 || N < 4 || N % 4 || K < 32 || K % 32) return r;
    if (ln && !gemv_ln_ok(M, K)) return r;
    r.ln = ln;
    if (gemv_dot_width(K)) {
        r.kernel = GemvKernel::Dot;
        r.nj = K / 256;
        r.maxm = M <= GD_MAXM ? GD_MAXM : 16;
        r.wv = M <= GD_MAXM ? 4 : 8;
        // one column per wave for K 5120 (fc2: half the weight bytes per workgroup, twice the workgroups); its 9..16
        // rows staged in two K halves (80 instead of 160 KB: two workgroups per CU)
        r.cpw = !ln && r.nj == 20 ? 1 : 2;
        r.ks = !ln && r.nj == 20 && r.maxm == 16 ? 2 : 1;
        r.cols = r.wv * r.cpw;
        r.grid = (N + r.cols - 1) / r.cols;
        r.block = r.wv * 64;
        // what each variant stages: the LayerNorm prologue writes padded rows [M][K + 8]; without it the rows are
        // DMA'd packed, K / KS columns at a time, in whole 1 KB pieces
        r.lds = ln ? (size_t)M * (K + 8) * 2 : ((size_t)M * (K / r.ks) * 2 + 1023) / 1024 * 1024;
        // the 16-row instantiations always raise (as they always have); the 8-row ones where 7 or 8 rows of K 5120
        // take 70 / 80 KB
        r.raise_lds = r.maxm > GD_MAXM || r.lds > (size_t)GV_LDS_DEFAULT;
        if (r.lds > (size_t)(r.raise_lds ? GD_LDS16 : GV_LDS_DEFAULT)) return GemvRoute{};
        if (ln)
            r.name = r.maxm == GD_MAXM ? CBW_GD_NAME_NJ(r.nj, "gemv_dot_kernel<true, ", ", 2, 8, 1, 4>")
                                       : CBW_GD_NAME_NJ(r.nj, "gemv_dot_kernel<true, ", ", 2, 16, 1, 8>");
        else if (r.nj == 20)
            r.name = r.maxm == GD_MAXM ? "gemv_dot_kernel<false, 20, 1, 8, 1, 4>" : "gemv_dot_kernel<false, 20, 1, 16, 2, 8>";
        else
            r.name = r.maxm == GD_MAXM ? CBW_GD_NAME_NJ(r.nj, "gemv_dot_kernel<false, ", ", 2, 8, 1, 4>")
                                       : CBW_GD_NAME_NJ(r.nj, "gemv_dot_kernel<false, ", ", 2, 16, 1, 8>");
        return r;
    }
    r.waves = gemv_waves(K);
    if (ln && r.waves > 8) return GemvRoute{};   // gemv_kernel<true> is bounded to 512 threads
    r.kernel = GemvKernel::Mfma;
    r.cols = 16;
    r.grid = (N + 15) / 16;
    r.block = 64 * r.waves;
    r.lds = ln ? (size_t)M * (K + 8) * 2 : 0;
    r.name = ln ? "gemv_kernel<true>" : "gemv_kernel<false>";
    return r;
}

// ---- the wide launch (cbw_gemv_wide): 1 <= M <= GV_WIDE_ROWS rows as ceil(M / 16) row groups in one launch
constexpr int GV_WIDE_ROWS = 80;   // = CBW_DEC_WIDE_ROWS (cbw.h): 16 windows x 5 beams

struct GemvWideRoute {
    // what every group runs: gemv_route(16, N, K, ln) -- the family of (K, ln), the tail group included on its 16-slot
    // instantiation; group.grid = the column blocks, group.lds = the LDS of a full group
    GemvRoute group;
    int groups = 0;               // ceil(M / 16); 0 = no route
    int grid_x = 0, grid_y = 0;   // groups_fast: (groups, column blocks), else (column blocks, groups)
    // "gemv_wide_kernel<LN>" / "gemv_dot_wide_kernel<LN, NJ, CPW, 16, KS, 8>": the group's kernel text, compiled as a row group
    const char* name = "";
};

constexpr GemvWideRoute gemv_wide_route(int M, int N, int K, bool ln, bool groups_fast = false) {
    GemvWideRoute w;
    if (M < 1 || M > GV_WIDE_ROWS) return w;
    const GemvRoute r = gemv_route(16, N, K, ln);
    if (r.kernel == GemvKernel::Invalid) return w;
    w.group = r;
    w.groups = (M + 15) / 16;
    w.grid_x = groups_fast ? w.groups : r.grid;
    w.grid_y = groups_fast ? r.grid : w.groups;
    if (r.kernel == GemvKernel::Mfma) w.name = ln ? "gemv_wide_kernel<true>" : "gemv_wide_kernel<false>";
    else if (ln) w.name = CBW_GD_NAME_NJ(r.nj, "gemv_dot_wide_kernel<true, ", ", 2, 16, 1, 8>");
    else if (r.nj == 20) w.name = "gemv_dot_wide_kernel<false, 20, 1, 16, 2, 8>";
    else w.name = CBW_GD_NAME_NJ(r.nj, "gemv_dot_wide_kernel<false, ", ", 2, 16, 1, 8>");
    return w;
}
