// Row-stationary streaming 1x1 convolution for the HBM-bound ResNet-50 expand convs (gfx950).
//
// Serves the 1x1 stride-1 convs with a short reduction (K = Cin + Cin2 in {128, 256, 384, 512}) and a wide
// output: the identity-residual expand convs of stages 2 and 3 (HF ResNetBottleNeckLayer's last
// ResNetConvLayer + identity shortcut + ReLU, efficient_kws/resnet.py:51-58) and the stage-1 / stage-2
// first-block expand with the shortcut 1x1 conv folded in as a second K-source (ConvArgs::x2).  At LEF
// sizes these layers move 1-2 KB per output pixel (residual in, output out) against only K x Cout
// MACs, so they are HBM-bound (arithmetic intensity 57-116 FLOP/B for the identity expands).
//
// Design (why not a tile GEMM): a 128x128 tile kernel re-reads its A rows once per N-tile and its weight
// tile once per M-tile through L2, and must hide the residual's HBM latency inside one tile's short
// K loop.  Here the weights are STATIONARY in LDS and the rows in REGISTERS:
//   * each workgroup (one per CU, persistent) loads an N-slice of the folded weights W[n][k] (<= 128 KB,
//     XOR-swizzled 16-byte chunks) into LDS once, plus its bias slice;
//   * each wave is an independent streamer (no barrier after the setup): it takes a 32-pixel unit,
//     loads the unit's activation rows (32 x K bf16) straight into VGPRs as MFMA B-fragments, then
//     walks the slice in 64-channel steps: 4 x 2 x (K/32) mfma_f32_16x16x32_bf16 per step with the
//     weight fragments read from LDS by ds_read_b128, epilogue bias + residual + ReLU from the
//     accumulators, 8-byte stores;
//   * the residual of step s+2 is issued right after step s's epilogue (two steps in flight), so
//     every wave keeps ~8 KB of HBM reads outstanding besides its stores; 8-12 waves per CU do the
//     rest of the latency hiding;
//   * the output channels of a step are permuted across the MFMA fragments (perm_row) so that a lane
//     ends with 8 contiguous channels per fragment pair: residual loads and output stores are 16 bytes
//     per lane, 64 contiguous bytes per pixel per wave-instruction;
//   * when the weights need several slices (stage 3: 512 KB -> 4 x 128 KB), the workgroups of one
//     row group sit on the same XCD (blockIdx % 8) and walk the same units in the same order, so the
//     rows are fetched from HBM once and re-read from that XCD's L2.
// MFMAs run transposed (C^T = W . X^T): the pixel sits on the lane (fr), the channel on the register.
#include <climits>

#include "cbw_common.h"
#include "cbw_kernels.h"
#include "conv_route.h"

typedef int cs_i32x4 __attribute__((ext_vector_type(4)));
// raw buffer load / store (LLVM intrinsics by asm label): 32-bit offsets against one descriptor; the
// hardware range check returns 0 for / drops out-of-range lanes
__device__ cs_i32x4 cs_raw_load(cs_i32x4 rsrc, int voffset, int soffset, int aux)
    __asm("llvm.amdgcn.raw.buffer.load.v4i32");
__device__ void cs_raw_store(cs_i32x4 vdata, cs_i32x4 rsrc, int voffset, int soffset, int aux)
    __asm("llvm.amdgcn.raw.buffer.store.v4i32");

namespace {

constexpr int CS_NSTEP = 64;            // output channels per step (4 fragments of 16)
constexpr int CS_WBYTES = 131072;       // weight slice budget in LDS
constexpr int CS_MAXSLICE = 1024;       // bias slots

CBW_DEV cs_i32x4 cs_rsrc(const void* base, uint32_t bytes) {
    const uint64_t p = (uint64_t)base;
    cs_i32x4 r{(int)(uint32_t)p, (int)(uint32_t)(p >> 32), (int)bytes, 0x00020000};
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = __builtin_amdgcn_readfirstlane(r[q]);
    return r;
}
CBW_DEV cs_i32x4 cs_load(cs_i32x4 rsrc, int voff, int soff) { return cs_raw_load(rsrc, voff, soff, 0); }
CBW_DEV void cs_store(cs_i32x4 v, cs_i32x4 rsrc, int voff, int soff) { cs_raw_store(v, rsrc, voff, soff, 0); }

CBW_DEV int cs_off(int row, int chunk, int pitch) { return row * pitch + ((chunk ^ (row & 15)) << 4); }

// Output-channel permutation of a 64-channel step: MFMA fragment c (0..3), fragment row i = 4 fq + q
// computes channel 32 (c >> 1) + 8 fq + 4 (c & 1) + q, so lane (fr, fq) ends with 8 contiguous
// channels per fragment pair.  LDS weight row 16 c + i of a step holds that channel's weights.
CBW_DEV int perm_row(int r) {
    const int st = r & ~63, c = (r >> 4) & 3, i = r & 15;
    return st + 32 * (c >> 1) + 8 * (i >> 2) + 4 * (c & 1) + (i & 3);
}

// KS = K / 32 (k-steps of one MFMA); WAVES = waves per workgroup (register budget: 512 / (WAVES / 4));
// RD = residual steps in flight; PF = 16-pixel fragments per wave unit; PN = prefetch the next unit's rows
template <int KS, int WAVES, int RD, int PF, int PN>
__global__ __launch_bounds__(WAVES * 64, 1) void conv_stream_kernel(ConvArgs a, int nslice, int slice_n, int exp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int K = KS * 32;
    constexpr int PITCH = K * 2;
    float* bias_s = (float*)(smem + slice_n * PITCH);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;

    // ---- workgroup -> (slice, row group): the nslice workgroups of a row group share an XCD
    const int G = gridDim.x;
    const int J = G / 8;                    // workgroups per XCD (G % 8 == 0, J % nslice == 0)
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int slice = j % nslice;
    const int rgs_per_xcd = J / nslice;
    const int rg = xcd * rgs_per_xcd + j / nslice;
    const int nrg = G / nslice;
    const int n_lo = slice * slice_n;

    // ---- setup: weight slice + bias slice -> LDS
    const bf16* __restrict__ Wt = (const bf16*)a.w;
    constexpr int CPR = K / 8;              // 16-byte chunks per weight row
    for (int e = tid; e < slice_n * CPR; e += WAVES * 64) {
        const int r = e / CPR, c = e - r * CPR;
        *(bf16x8*)(smem + cs_off(r, c, PITCH)) = *(const bf16x8*)(Wt + (int64_t)(n_lo + perm_row(r)) * K + c * 8);
    }
    for (int c = tid; c < slice_n; c += WAVES * 64) bias_s[c] = a.bias ? a.bias[n_lo + c] : 0.f;
    __syncthreads();

    const int M = a.M, Cin = a.Cin, Cin2 = a.x2 ? a.Cin2 : 0;
    const int HoWo = a.Ho * a.Wo, Wo = a.Wo;
    const bool relu = a.flags & CBW_EPI_RELU;
    const bool has_res = a.res != nullptr;
    const int nsteps = slice_n / CS_NSTEP;
    const int units = (M + (PF * 16) - 1) / (PF * 16);
    // buffer descriptors: 32-bit per-lane offsets, wave-uniform channel offsets in soffset; rows past M
    // get an offset past num_records (loads return 0, stores are dropped)
    const cs_i32x4 xr = cs_rsrc(a.x, (uint32_t)((int64_t)M * Cin * 2));
    const cs_i32x4 x2r = cs_rsrc(a.x2 ? a.x2 : a.x, a.x2 ? (uint32_t)((int64_t)a.N * a.H2 * a.W2 * Cin2 * 2) : 0u);
    const cs_i32x4 rr = cs_rsrc(has_res ? a.res : a.y, has_res ? (uint32_t)((int64_t)M * a.res_ld * 2) : 0u);
    const cs_i32x4 yr = cs_rsrc(a.y, (uint32_t)((int64_t)M * a.y_ld * 2));
    constexpr int OOR = 0x7ffffff0;

    // ---- a unit's rows -> B fragments (lane: pixel fr of fragment pf, k = 32 ks + 8 fq ..)
    auto load_rows = [&](int u, bf16x8 (&xv)[PF][KS], int (&ro)[PF], int (&yo)[PF]) {
#pragma unroll
        for (int pf = 0; pf < PF; ++pf) {
            const int p = u * (PF * 16) + pf * 16 + fr;
            const bool ok = p < M;
            const int xo = ok ? p * Cin * 2 + fq * 16 : OOR;
            int x2o = OOR;
            if (Cin2 && ok) {
                const int nn = p / HoWo, rem = p - nn * HoWo;
                const int oh = rem / Wo, ow = rem - oh * Wo;
                x2o = ((nn * a.H2 + oh * a.s2) * a.W2 + ow * a.s2) * Cin2 * 2 + fq * 16;
            }
            ro[pf] = ok ? p * a.res_ld * 2 + fq * 16 : OOR;
            yo[pf] = ok ? p * a.y_ld * 2 + fq * 16 : OOR;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int k = ks * 32;
                const cs_i32x4 v = k < Cin ? cs_load(xr, xo, k * 2) : cs_load(x2r, x2o, (k - Cin) * 2);
                xv[pf][ks] = __builtin_bit_cast(bf16x8, v);
            }
        }
    };
    const int ustride = nrg * WAVES;
    int roff[PF], yoff[PF], roffn[PF], yoffn[PF];
    bf16x8 xf[PF][KS], xn[PF][KS];
    int u = rg * WAVES + wid;
    if (PN && u < units) load_rows(u, xn, roffn, yoffn);
    for (; u < units; u += ustride) {
        if (PN) {   // this unit's rows were issued during the previous unit's last steps
#pragma unroll
            for (int pf = 0; pf < PF; ++pf) {
                roff[pf] = roffn[pf];
                yoff[pf] = yoffn[pf];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) xf[pf][ks] = xn[pf][ks];
            }
        } else {
            load_rows(u, xf, roff, yoff);
        }
        // ---- residual ring: steps s .. s + RD - 1 in flight.  Lane (fr, fq) owns channels
        // 32 h + 8 fq .. + 7 (h = 0, 1) of each 64-channel step: two 16-byte loads / stores per pixel
        // fragment, each wave-instruction covering 16 pixels x 64 contiguous bytes.
        cs_i32x4 res[RD][PF][2];
        auto load_res = [&](cs_i32x4 (&dst)[PF][2], int s) {
#pragma unroll
            for (int pf = 0; pf < PF; ++pf)
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    dst[pf][h] = (exp & 1) ? cs_i32x4{0, 0, 0, 0}
                                           : cs_load(rr, roff[pf], (n_lo + s * CS_NSTEP + h * 32) * 2);
        };
        if (has_res) {
#pragma unroll
            for (int r = 0; r < RD; ++r)
                if (r < nsteps) load_res(res[r], r);
        }
        auto step = [&](cs_i32x4 (&rs)[PF][2], int s) {
            f32x4 acc[PF][4];
#pragma unroll
            for (int pf = 0; pf < PF; ++pf)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[pf][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                bf16x8 wf[4];
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    wf[c] = *(const bf16x8*)(smem + cs_off(s * CS_NSTEP + c * 16 + fr, ks * 4 + fq, PITCH));
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int pf = 0; pf < PF; ++pf)
                        acc[pf][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[c], xf[pf][ks], acc[pf][c], 0, 0, 0);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int nl = s * CS_NSTEP + h * 32 + fq * 8;
                const f32x4 bv0 = *(const f32x4*)(bias_s + nl), bv1 = *(const f32x4*)(bias_s + nl + 4);
#pragma unroll
                for (int pf = 0; pf < PF; ++pf) {
                    float v[8];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        v[q] = acc[pf][2 * h][q] + bv0[q];
                        v[4 + q] = acc[pf][2 * h + 1][q] + bv1[q];
                    }
                    if (has_res) {
                        const bf16x8 rv = __builtin_bit_cast(bf16x8, rs[pf][h]);
#pragma unroll
                        for (int q = 0; q < 8; ++q) v[q] += bf2f(rv[q]);
                    }
                    bf16x8 o;
#pragma unroll
                    for (int q = 0; q < 8; ++q) o[q] = f2bf(relu ? fmaxf(v[q], 0.f) : v[q]);
                    const int yo = (exp & 2) ? (v[0] == 12345.f ? yoff[pf] : OOR) : yoff[pf];
                    cs_store(__builtin_bit_cast(cs_i32x4, o), yr, yo, (n_lo + s * CS_NSTEP + h * 32) * 2);
                }
            }
            if (has_res && s + RD < nsteps) load_res(rs, s + RD);
        };
        for (int s = 0; s < nsteps; s += RD) {   // nsteps % RD == 0 (slice_n % 128 == 0)
            // PN: the next unit's rows go out with the last RD steps (after their residual loads, so
            // waiting for those never waits for the prefetch)
            if (PN && s + RD >= nsteps && u + ustride < units) load_rows(u + ustride, xn, roffn, yoffn);
#pragma unroll
            for (int r = 0; r < RD; ++r) step(res[r], s + r);
        }
    }
}

// Chained variant for the stage-2 identity junctions: block b's expand 128 -> 512 + bias + residual + ReLU -> Y,
// and in the same pass block b + 1's reduce T1' = relu(Y . Wr^T + br) (512 -> 128), so Y is never re-read.
// A step's epilogue leaves lane (fr, fq) with the bf16x8 `o` of channels 64 s + 32 h + 8 fq .. + 7 of pixel
// 16 pf + fr for each half h: exactly the B fragment of k-step 2 s + h of the same MFMA (what load_rows loads
// for a K 512 conv), so the reduce consumes `o` from registers: 8 MFMAs per pixel fragment per half into 8
// running accumulators (the 128 reduce channels), k-steps 0 .. 15 ascending into one fp32 accumulator, bias
// after, ReLU, RNE to bf16 -- the arithmetic of conv_stream_kernel<16, 8, 2, 1, 0>, which runs that reduce as
// a launch of its own, so T1' is bit-identical to the two launches.
// The expand weights stay stationary in LDS; the reduce weights (128 KB more) do not fit beside them, so the
// A fragments of Wr are read from global memory (L2-resident: every wave of the chip reads the same 128 KB)
// in the fragment order cbw_conv_chain_pack leaves them in: [k-step 16][fragment 8][lane 64] x 16 bytes, one
// contiguous 1 KB per wave instruction.  The reduce's output channels are permuted like the expand's
// (perm_row over each 64 channels), so T1' leaves in 16-byte stores as well.
// Those reads are the kernel's cost beside its HBM bytes (128 KB per wave unit), so it runs 64-pixel units on 4 waves
// (one per SIMD, accumulators in AGPRs): each Wr fragment feeds 4 pixel fragments.
// K = 128, Cout = 512 in one slice, bf16 residual, ReLU; no row prefetch (registers).
constexpr int CC_K = 128, CC_N = 512, CC_R = 128;   // expand K, expand Cout = reduce K, reduce Cout
template <int WAVES, int RD, int PF>
__global__ __launch_bounds__(WAVES * 64, 1) void conv_stream_chain_kernel(ConvArgs a, const bf16* __restrict__ wrp,
                                                                          const float* __restrict__ br, void* t1) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KS = CC_K / 32;
    constexpr int PITCH = CC_K * 2;
    constexpr int NSTEPS = CC_N / CS_NSTEP;
    constexpr int RF = CC_R / 16;           // reduce output fragments
    float* bias_s = (float*)(smem + CC_N * PITCH);
    float* br_s = bias_s + CC_N;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;

    // ---- setup: expand weights + both biases -> LDS
    const bf16* __restrict__ Wt = (const bf16*)a.w;
    constexpr int CPR = CC_K / 8;
    for (int e = tid; e < CC_N * CPR; e += WAVES * 64) {
        const int r = e / CPR, c = e - r * CPR;
        *(bf16x8*)(smem + cs_off(r, c, PITCH)) = *(const bf16x8*)(Wt + (int64_t)perm_row(r) * CC_K + c * 8);
    }
    for (int c = tid; c < CC_N; c += WAVES * 64) bias_s[c] = a.bias ? a.bias[c] : 0.f;
    for (int c = tid; c < CC_R; c += WAVES * 64) br_s[c] = br ? br[c] : 0.f;
    __syncthreads();

    const int M = a.M;
    const int units = (M + (PF * 16) - 1) / (PF * 16);
    const cs_i32x4 xr = cs_rsrc(a.x, (uint32_t)((int64_t)M * CC_K * 2));
    const cs_i32x4 rr = cs_rsrc(a.res, (uint32_t)((int64_t)M * a.res_ld * 2));
    const cs_i32x4 yr = cs_rsrc(a.y, (uint32_t)((int64_t)M * a.y_ld * 2));
    const cs_i32x4 tr = cs_rsrc(t1, (uint32_t)((int64_t)M * CC_R * 2));
    const cs_i32x4 wr = cs_rsrc(wrp, (uint32_t)(CC_R * CC_N * 2));
    constexpr int OOR = 0x7ffffff0;

    const int ustride = gridDim.x * WAVES;
    for (int u = blockIdx.x * WAVES + wid; u < units; u += ustride) {
        int roff[PF], yoff[PF], toff[PF];
        bf16x8 xf[PF][KS];
#pragma unroll
        for (int pf = 0; pf < PF; ++pf) {
            const int p = u * (PF * 16) + pf * 16 + fr;
            const bool ok = p < M;
            const int xo = ok ? p * CC_K * 2 + fq * 16 : OOR;
            roff[pf] = ok ? p * a.res_ld * 2 + fq * 16 : OOR;
            yoff[pf] = ok ? p * a.y_ld * 2 + fq * 16 : OOR;
            toff[pf] = ok ? p * CC_R * 2 + fq * 16 : OOR;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) xf[pf][ks] = __builtin_bit_cast(bf16x8, cs_load(xr, xo, ks * 64));
        }
        cs_i32x4 res[RD][PF][2];
        auto load_res = [&](cs_i32x4 (&dst)[PF][2], int s) {
#pragma unroll
            for (int pf = 0; pf < PF; ++pf)
#pragma unroll
                for (int h = 0; h < 2; ++h) dst[pf][h] = cs_load(rr, roff[pf], (s * CS_NSTEP + h * 32) * 2);
        };
#pragma unroll
        for (int r = 0; r < RD; ++r) load_res(res[r], r);
        // the reduce's A fragments of k-step kk = 2 s + h
        auto load_wr = [&](cs_i32x4 (&dst)[RF], int kk) {
#pragma unroll
            for (int c = 0; c < RF; ++c) dst[c] = cs_load(wr, lane * 16, (kk * RF + c) * 1024);
        };
        f32x4 tacc[PF][RF];
#pragma unroll
        for (int pf = 0; pf < PF; ++pf)
#pragma unroll
            for (int c = 0; c < RF; ++c) tacc[pf][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        // half 0's Wr fragments go out ahead of the expand MFMAs, half 1's ahead of half 0's epilogue
        auto step = [&](cs_i32x4 (&rs)[PF][2], int s) {
            cs_i32x4 wr0[RF], wr1[RF];
            load_wr(wr0, 2 * s);
            f32x4 acc[PF][4];
#pragma unroll
            for (int pf = 0; pf < PF; ++pf)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[pf][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                bf16x8 wf[4];
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    wf[c] = *(const bf16x8*)(smem + cs_off(s * CS_NSTEP + c * 16 + fr, ks * 4 + fq, PITCH));
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int pf = 0; pf < PF; ++pf)
                        acc[pf][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[c], xf[pf][ks], acc[pf][c], 0, 0, 0);
            }
            load_wr(wr1, 2 * s + 1);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int nl = s * CS_NSTEP + h * 32 + fq * 8;
                const f32x4 bv0 = *(const f32x4*)(bias_s + nl), bv1 = *(const f32x4*)(bias_s + nl + 4);
#pragma unroll
                for (int pf = 0; pf < PF; ++pf) {
                    float v[8];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        v[q] = acc[pf][2 * h][q] + bv0[q];
                        v[4 + q] = acc[pf][2 * h + 1][q] + bv1[q];
                    }
                    const bf16x8 rv = __builtin_bit_cast(bf16x8, rs[pf][h]);
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] += bf2f(rv[q]);
                    bf16x8 o;
#pragma unroll
                    for (int q = 0; q < 8; ++q) o[q] = f2bf(fmaxf(v[q], 0.f));
                    cs_store(__builtin_bit_cast(cs_i32x4, o), yr, yoff[pf], (s * CS_NSTEP + h * 32) * 2);
#pragma unroll
                    for (int c = 0; c < RF; ++c)
                        tacc[pf][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            __builtin_bit_cast(bf16x8, h ? wr1[c] : wr0[c]), o, tacc[pf][c], 0, 0, 0);
                }
            }
            if (s + RD < NSTEPS) load_res(rs, s + RD);
        };
        for (int s = 0; s < NSTEPS; s += RD) {
#pragma unroll
            for (int r = 0; r < RD; ++r) step(res[r], s + r);
        }
        // ---- T1' epilogue: lane (fr, fq) holds channels 64 t + 32 h + 8 fq .. + 7 in fragments 4 t + 2 h, + 1
#pragma unroll
        for (int t = 0; t < CC_R / 64; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int nl = t * 64 + h * 32 + fq * 8;
                const f32x4 bv0 = *(const f32x4*)(br_s + nl), bv1 = *(const f32x4*)(br_s + nl + 4);
#pragma unroll
                for (int pf = 0; pf < PF; ++pf) {
                    bf16x8 o;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        o[q] = f2bf(fmaxf(tacc[pf][4 * t + 2 * h][q] + bv0[q], 0.f));
                        o[4 + q] = f2bf(fmaxf(tacc[pf][4 * t + 2 * h + 1][q] + bv1[q], 0.f));
                    }
                    cs_store(__builtin_bit_cast(cs_i32x4, o), tr, toff[pf], (t * 64 + h * 32) * 2);
                }
            }
    }
}

// Wr [128][512] row-major -> the chained kernel's fragment order: 16-byte chunk ((kk 8 + c) 64 + lane) holds
// row perm_row(16 c + fr), k = 32 kk + 8 fq .. + 7 (lane = 16 fq + fr)
__global__ void conv_chain_pack_kernel(const bf16* __restrict__ w, bf16* __restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;   // one 16-byte chunk each
    if (e >= CC_R * CC_N / 8) return;
    const int lane = e & 63, c = (e >> 6) & 7, kk = e >> 9;
    const int fr = lane & 15, fq = lane >> 4;
    *(bf16x8*)(out + (int64_t)e * 8) = *(const bf16x8*)(w + (int64_t)perm_row(16 * c + fr) * CC_N + kk * 32 + fq * 8);
}

static_assert(CS_WBYTES == CONV_CS_WBYTES && CS_MAXSLICE == CONV_CS_MAXSLICE, "conv_route.h slices for this LDS budget");
static_assert(CC_K == CONV_CC_K && CC_N == CONV_CC_N && CC_R == CONV_CC_R, "conv_route.h chains these shapes");

// the persistent grid: CBW_CS_CUS=N (A/B) sizes it for N CUs, cbw_cs_grid_cus for what the runtime leaves this stream
int cs_grid_cus() {
    static const int cap = [] {
        const char* e = getenv("CBW_CS_CUS");
        return e && atoi(e) > 0 ? atoi(e) : INT_MAX;
    }();
    const int n = std::min(cbw_num_cus(), cap);
    return cbw_cs_grid_cus > 0 ? std::min(n, cbw_cs_grid_cus) : n;
}

int cs_exp() {   // CBW_CS_EXP diagnostic builds: 1 no residual loads, 2 no stores (wrong results)
    const char* e = getenv("CBW_CS_EXP");
    return e ? atoi(e) : 0;
}

}  // namespace

thread_local int cbw_cs_grid_cus = 0;

bool cbw_conv_stream_supported(const ConvArgs& a) { return conv_stream_supported(a, conv_knobs_from_env()); }

hipError_t cbw_conv_stream(const ConvArgs& a, hipStream_t st) {
    return cbw_conv_stream(a, conv_stream_route(a, conv_knobs_from_env()), st);
}

hipError_t cbw_conv_stream(const ConvArgs& a, const ConvRoute& r, hipStream_t st) {
    // (the guard is the kernel's own: what it can run whatever the knobs prefer)
    const int ktot = a.Cin + (a.x2 ? a.Cin2 : 0);
    if (r.kernel != ConvKernel::Stream || !conv_stream_supported(a, ConvKnobs{}) || r.stream.ks * 32 != ktot)
        return hipErrorNotSupported;
    const int sn = slice_channels(a.Cout, ktot);
    const int nslice = a.Cout / sn;
    const int G = 8 * nslice * std::max(1, cs_grid_cus() / (8 * nslice));
    const size_t lds = (size_t)sn * ktot * 2 + (size_t)sn * 4;
    const ConvStreamVariant& v = r.stream;
#define CS_LAUNCH(KS, WAVES, RD, PFD, PN)                                                                         \
    if (v.ks == KS && v.waves == WAVES && v.rd == RD && v.pfd == PFD && v.pn == PN) {                             \
        hipLaunchKernelGGL((conv_stream_kernel<KS, WAVES, RD, PFD, PN>), dim3(G), dim3(WAVES * 64), lds, st, a, \
                           nslice, sn, cs_exp());                                                                \
        return hipGetLastError();                                                                                \
    }
    CS_LAUNCH(4, 8, 2, 2, 1)
    CS_LAUNCH(4, 12, 2, 2, 0)
    CS_LAUNCH(8, 8, 1, 2, 1)
    CS_LAUNCH(8, 12, 1, 2, 0)
    CS_LAUNCH(16, 8, 2, 1, 0)
    CS_LAUNCH(12, 8, 2, 2, 0)
#undef CS_LAUNCH
    return hipErrorInvalidValue;   // a variant conv_route.h names and this file does not instantiate
}

// ---- chained expand + next reduce (conv_stream_chain_kernel)
bool cbw_conv_chain_supported(const ConvArgs& a, int red_cout) {
    return conv_chain_supported(a, red_cout, conv_knobs_from_env());
}

hipError_t cbw_conv_chain_pack(const uint16_t* wr, uint16_t* packed, hipStream_t st) {
    hipLaunchKernelGGL(conv_chain_pack_kernel, dim3(CC_R * CC_N / 8 / 256), dim3(256), 0, st, (const bf16*)wr,
                       (bf16*)packed);
    return hipGetLastError();
}

hipError_t cbw_conv_chain(const ConvArgs& a, const uint16_t* wr_packed, const float* br, void* t1, hipStream_t st) {
    const ConvRoute r = conv_chain_route(a, CC_R, conv_knobs_from_env());
    if (r.kernel != ConvKernel::Chain || !wr_packed || !t1) return hipErrorNotSupported;
    const int G = 8 * std::max(1, cs_grid_cus() / 8);
    const size_t lds = (size_t)CC_N * CC_K * 2 + (size_t)(CC_N + CC_R) * 4;
    cbw_last_conv_kernel = r.name;
    hipLaunchKernelGGL((conv_stream_chain_kernel<4, 2, 4>), dim3(G), dim3(4 * 64), lds, st, a, (const bf16*)wr_packed, br,
                       t1);
    return hipGetLastError();
}
