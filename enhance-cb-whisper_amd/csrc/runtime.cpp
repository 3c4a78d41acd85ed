// libcbw native runtime: C ABI (include/cbw.h), parameter loading with
// BatchNorm folding, layer plans and workspace carving for the KWS classifier
// and the Whisper encoder.  No allocation or synchronisation happens in the
// compute entry points (cbw_kws_project / cbw_kws_score / cbw_mel /
// cbw_encoder_hs), so callers can capture them into hipGraphs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "cbw.h"
#include "cbw_kernels.h"
#include "conv_route.h"
#include "gemv_route.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(CBW_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define CHK(expr)                  \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != CBW_OK) return rc_; \
    } while (0)

int block_zero_page(const void** out);   // a device's 256-byte zero page (defined with the standalone conv entries)

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    int alloc(size_t n) {
        reset();
        if (hipMalloc(&p, n ? n : 16) != hipSuccess) { p = nullptr; return fail(CBW_ERR_OOM, "hipMalloc failed"); }
        bytes = n;
        return CBW_OK;
    }
    template <class T>
    int upload(const std::vector<T>& v) {
        CHK(alloc(v.size() * sizeof(T)));
        if (hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
            return fail(CBW_ERR_HIP, "hipMemcpy upload failed");
        return CBW_OK;
    }
    template <class T> T* as() const { return (T*)p; }
};

uint16_t f2bf_host(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

std::vector<uint16_t> to_bf16(const std::vector<float>& v) {
    std::vector<uint16_t> o(v.size());
    for (size_t i = 0; i < v.size(); ++i) o[i] = f2bf_host(v[i]);
    return o;
}

float bf16_round_host(float v) {
    const uint32_t u = (uint32_t)f2bf_host(v) << 16;
    float r;
    std::memcpy(&r, &u, 4);
    return r;
}

// the 3-term split of n fp32 weights: dst = [hi | lo | hi], n each, hi = bf16(v), lo = bf16(v - hi); the caller
// places dst (row stride, zero padding behind the 3 n values)
void split3(const float* v, int n, uint16_t* dst) {
    for (int i = 0; i < n; ++i) {
        dst[i] = dst[2 * n + i] = f2bf_host(v[i]);
        dst[n + i] = f2bf_host(v[i] - bf16_round_host(v[i]));
    }
}

struct ParamStore {
    std::map<std::string, std::vector<float>> host;
    int set(const char* name, const float* data, int64_t numel) {
        if (!name || (!data && numel > 0) || numel < 0) return fail(CBW_ERR_INVALID, "set_param: bad arguments");
        host[name] = std::vector<float>(data, data + numel);
        return CBW_OK;
    }
    const std::vector<float>* get(const std::string& n, size_t numel, int* rc) const {
        auto it = host.find(n);
        if (it == host.end()) { *rc = fail(CBW_ERR_STATE, "missing parameter " + n); return nullptr; }
        if (it->second.size() != numel) {
            *rc = fail(CBW_ERR_INVALID, "parameter " + n + ": expected " + std::to_string(numel) + " elements, got " +
                                            std::to_string(it->second.size()));
            return nullptr;
        }
        *rc = CBW_OK;
        return &it->second;
    }
};

// BatchNorm (eval) folded into a bias-free conv: w' = w * g/sqrt(v+eps), b' = beta - mean * g/sqrt(v+eps)
int fold_bn(const ParamStore& ps, const std::string& bn, int cout, std::vector<float>& scale, std::vector<float>& shift) {
    int rc;
    const auto* g = ps.get(bn + ".weight", cout, &rc); if (!g) return rc;
    const auto* b = ps.get(bn + ".bias", cout, &rc); if (!b) return rc;
    const auto* m = ps.get(bn + ".running_mean", cout, &rc); if (!m) return rc;
    const auto* v = ps.get(bn + ".running_var", cout, &rc); if (!v) return rc;
    scale.resize(cout);
    shift.resize(cout);
    for (int o = 0; o < cout; ++o) {
        const double s = (double)(*g)[o] / std::sqrt((double)(*v)[o] + 1e-5);
        scale[o] = (float)s;
        shift[o] = (float)((double)(*b)[o] - (double)(*m)[o] * s);
    }
    return CBW_OK;
}

struct ConvShape {
    int cin = 0, cout = 0, k = 1, stride = 1;
    bool relu = false;
};

// a conv (or Linear: k = 1) of any tier: its shape and its device weights in that tier's format, bias fp32
struct ConvW : ConvShape {
    DevBuf w, b;
};

// torch conv weight [Cout][Cin][k][k] + BN -> f32 [Cout][k][k][Cin] (BN scale folded) + f32 bias
int fold_conv_host(const ParamStore& ps, const std::string& prefix, int cin, int cout, int k, std::vector<float>& o,
                   std::vector<float>& sh) {
    int rc;
    const size_t n = (size_t)cout * cin * k * k;
    const auto* w = ps.get(prefix + ".convolution.weight", n, &rc);
    if (!w) return rc;
    std::vector<float> sc;
    CHK(fold_bn(ps, prefix + ".normalization", cout, sc, sh));
    o.assign(n, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int kh = 0; kh < k; ++kh)
                for (int kw = 0; kw < k; ++kw)
                    o[(((size_t)co * k + kh) * k + kw) * cin + ci] =
                        (*w)[(((size_t)co * cin + ci) * k + kh) * k + kw] * sc[co];
    return CBW_OK;
}

// conv `prefix` of shape s with BN folded: bf16 weights, or fp32 ones for the exact re-scoring path (kws_exact.hip)
int load_conv_bn(const ParamStore& ps, const std::string& prefix, const ConvShape& s, ConvW& c, bool f32 = false) {
    std::vector<float> o, sh;
    CHK(fold_conv_host(ps, prefix, s.cin, s.cout, s.k, o, sh));
    static_cast<ConvShape&>(c) = s;
    CHK(f32 ? c.w.upload(o) : c.w.upload(to_bf16(o)));
    CHK(c.b.upload(sh));
    return CBW_OK;
}

// expand 1x1 (mid -> cout) and shortcut 1x1 (cin -> cout, stride s) of one bottleneck folded
// into one K-concatenated conv: w [cout][mid + cin], bias = b_expand + b_shortcut.
int load_fused_expand_shortcut(const ParamStore& ps, const std::string& expand, const std::string& shortcut,
                               int mid, int cin, int cout, ConvW& c) {
    std::vector<float> we, be, ws, bs;
    CHK(fold_conv_host(ps, expand, mid, cout, 1, we, be));
    CHK(fold_conv_host(ps, shortcut, cin, cout, 1, ws, bs));
    std::vector<float> w((size_t)cout * (mid + cin)), b(cout);
    for (int co = 0; co < cout; ++co) {
        std::copy(we.begin() + (size_t)co * mid, we.begin() + (size_t)(co + 1) * mid, w.begin() + (size_t)co * (mid + cin));
        std::copy(ws.begin() + (size_t)co * cin, ws.begin() + (size_t)(co + 1) * cin,
                  w.begin() + (size_t)co * (mid + cin) + mid);
        b[co] = be[co] + bs[co];
    }
    CHK(c.w.upload(to_bf16(w)));
    CHK(c.b.upload(b));
    return CBW_OK;
}

// Per-launch HIP-event timing of the implicit-GEMM conv kernels (bench.py roofline):
// events recorded on the launch stream around each conv launch, read after a sync.
struct Prof {
    bool on = false;
    std::vector<hipEvent_t> ev;     // 2 per launch
    std::vector<double> flop;       // algorithmic FLOPs per recorded launch
    std::vector<int> tier;          // 0 the bf16 scoring pass, 1 the compensated re-scoring tier
    std::vector<const char*> kern;  // the kernel each recorded launch ran (cbw_last_conv_kernel: static strings)
    int cur_tier = 0;
    int used = 0;
    ~Prof() { for (auto e : ev) (void)hipEventDestroy(e); }
    // One record brackets one launch on stream st.  begin() records the first event and gives the record's slot
    // (-1: no profile, profiling off or the table full); end() is called only after the launch succeeded, so an error
    // return between the two leaves `used` unchanged.  p may be null.
    static int begin(Prof* p, hipStream_t st, int* slot) {
        *slot = (p && p->on && (size_t)(2 * p->used + 1) < p->ev.size()) ? p->used : -1;
        if (*slot >= 0) HIPCHK(hipEventRecord(p->ev[2 * *slot], st));
        return CBW_OK;
    }
    static int end(Prof* p, int slot, hipStream_t st, double flops, const char* kernel, int tier_ = -1) {
        if (slot < 0) return CBW_OK;
        HIPCHK(hipEventRecord(p->ev[2 * slot + 1], st));
        p->flop[slot] = flops;
        p->tier[slot] = tier_ < 0 ? p->cur_tier : tier_;
        p->kern[slot] = kernel;
        p->used++;
        return CBW_OK;
    }
};

// cur_tier for the records of one scoring call, put back on every path out of the scope
struct TierScope {
    Prof& p;
    const int saved;
    TierScope(Prof& p_, int tier) : p(p_), saved(p_.cur_tier) { p.cur_tier = tier; }
    ~TierScope() { p.cur_tier = saved; }
    TierScope(const TierScope&) = delete;
    TierScope& operator=(const TierScope&) = delete;
};

struct Src2 {   // second K-source of a fused 1x1 conv (ConvArgs::x2)
    const void* x;
    int cin, H, W, stride;
};

// output extent of a k-tap, "same"-padded (k / 2) conv or pool over h; k = 1: a strided 1x1 (the shortcuts)
int out_dim(int h, int k, int stride) { return (h + 2 * (k / 2) - k) / stride + 1; }

// the geometry fields ConvArgs, F32ConvArgs and F8ConvArgs share, for a KH x KW conv over x [N][H][W][Cin]
template <class Args>
void conv_geometry(Args& a, int N, int H, int W, int Cin, int Cout, int KH, int KW, int sh, int sw, int ph, int pw) {
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.KH = KH; a.KW = KW;
    a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw;
    a.Ho = (H + 2 * ph - KH) / sh + 1;
    a.Wo = (W + 2 * pw - KW) / sw + 1;
    a.M = N * a.Ho * a.Wo;
}
// ... for the square, "same"-padded conv c (out_dim's extents)
template <class Args>
void conv_geometry(Args& a, const ConvShape& c, int N, int H, int W) {
    conv_geometry(a, N, H, W, c.cin, c.cout, c.k, c.k, c.stride, c.stride, c.k / 2, c.k / 2);
}
// the plain GEMM y[M][N] = x[M][K] . w[N][K]^T as a 1x1 conv over one row of M pixels (operands left to the caller)
ConvArgs linear_args(int M, int K, int N) {
    ConvArgs a{};
    conv_geometry(a, 1, 1, M, K, N, 1, 1, 1, 1, 0, 0);
    a.res_ld = a.y_ld = N;
    return a;
}

int launch_conv(const ConvW& c, const void* x, int N, int H, int W, void* y, const void* res, int flags,
                const void* zero, hipStream_t st, Prof* prof = nullptr, const Src2* src2 = nullptr,
                float* splitk_ws = nullptr) {
    ConvArgs a{};
    a.x = x; a.w = c.w.p; a.bias = c.b.as<float>(); a.res = res; a.y = y; a.zero = zero;
    if (src2) { a.x2 = src2->x; a.Cin2 = src2->cin; a.H2 = src2->H; a.W2 = src2->W; a.s2 = src2->stride; }
    conv_geometry(a, c, N, H, W);
    a.res_ld = a.y_ld = c.cout;
    a.flags = flags | (c.relu ? CBW_EPI_RELU : 0);
    int slot;
    CHK(Prof::begin(prof, st, &slot));
    if (splitk_ws) HIPCHK(cbw_conv_igemm_splitk(a, cbw_conv_splitk_factor(a), splitk_ws, st));
    else HIPCHK(cbw_conv_igemm(a, st));
    return Prof::end(prof, slot, st, 2.0 * a.M * a.Cout * ((double)a.Cin * a.KH * a.KW + (a.x2 ? a.Cin2 : 0)),
                     cbw_last_conv_kernel);
}

// Block b's identity expand (c2: t2 -> y with residual res and ReLU) and block b + 1's 1x1 reduce (r0: y -> t1n) as
// one chained launch (cbw_conv_chain) when both convs run on the streaming kernel today and the shapes are the
// chain's; *done = false leaves both launches to the caller.  One profile record: the two convs' FLOPs summed.
int launch_chain(const ConvW& c2, const ConvW& r0, const DevBuf& r0_packed, const void* t2, int N, int H, int W, void* y,
                 const void* res, void* t1n, const void* zero, hipStream_t st, Prof* prof, bool* done) {
    *done = false;
    if (!r0_packed.p || !res || c2.relu) return CBW_OK;   // (the block's ReLU follows the residual add)
    ConvArgs a{}, r{};   // the two convs as their own launches would see them
    a.x = t2; a.w = c2.w.p; a.bias = c2.b.as<float>(); a.res = res; a.y = y; a.zero = zero;
    conv_geometry(a, c2, N, H, W);
    a.res_ld = a.y_ld = c2.cout;
    a.flags = CBW_EPI_RELU;
    r.x = y; r.w = r0.w.p; r.bias = r0.b.as<float>(); r.y = t1n; r.zero = zero;
    conv_geometry(r, r0, N, a.Ho, a.Wo);
    r.res_ld = r.y_ld = r0.cout;
    r.flags = r0.relu ? CBW_EPI_RELU : 0;
    if (conv_junction_route(a, r, conv_knobs_from_env()).kernel != ConvKernel::Chain) return CBW_OK;
    int slot;
    CHK(Prof::begin(prof, st, &slot));
    HIPCHK(cbw_conv_chain(a, r0_packed.as<uint16_t>(), r0.b.as<float>(), t1n, st));
    CHK(Prof::end(prof, slot, st, 2.0 * a.M * a.Cout * (double)a.Cin + 2.0 * a.M * r0.cout * (double)r0.cin,
                  cbw_last_conv_kernel));
    *done = true;
    return CBW_OK;
}

size_t align_up(size_t n) { return (n + 255) & ~(size_t)255; }

// ------------------------------------------------------------------ ResNet topology
// HF ResNetConfig defaults as instantiated by efficient_kws/resnet.py:22-38:
// embedding 64, stages [256,512,1024,2048]x[3,4,6,3] bottleneck (resnet-50),
// [64,128,256,512] basic for resnet-18/34; stride 2 in the first layer of stages
// 2-4, in the 3x3 (downsample_in_bottleneck = False); shortcut when shape changes.
// One block of the network as the reference builds it; relu is the conv module's own activation (the block's
// ReLU after the residual sum is the tiers' business).  cbw_kws_finalize builds the list once (cbw_kws::topo) and
// every tier's loader, walker and planner reads it.
struct BlockTopo {
    std::string prefix;   // parameter prefix of the block
    int stage = 0;        // 1..4
    int nconv = 0;        // 3 bottleneck, 2 basic
    ConvShape conv[3];
    bool has_sc = false;  // projection shortcut (1x1, the block's stride)
    ConvShape sc;
};

int resnet_topology(int depth, std::vector<BlockTopo>& topo) {
    std::vector<int> hs, depths;
    bool bottleneck = true;
    switch (depth) {
        case 50: hs = {256, 512, 1024, 2048}; depths = {3, 4, 6, 3}; break;
        case 34: hs = {64, 128, 256, 512}; depths = {3, 4, 6, 3}; bottleneck = false; break;
        case 18: hs = {64, 128, 256, 512}; depths = {2, 2, 2, 2}; bottleneck = false; break;
        default: return fail(CBW_ERR_INVALID, "resnet_depth must be 18, 34 or 50");
    }
    topo.clear();
    int cin = 64;
    for (size_t s = 0; s < hs.size(); ++s) {
        const int cout = hs[s];
        for (int li = 0; li < depths[s]; ++li) {
            const int stride = (li == 0 && s > 0) ? 2 : 1;
            BlockTopo b;
            b.prefix = "model.feature_extractor.encoder.stages." + std::to_string(s) + ".layers." + std::to_string(li);
            b.stage = (int)s + 1;
            b.has_sc = cin != cout || stride != 1;
            if (b.has_sc) b.sc = {cin, cout, 1, stride, false};
            if (bottleneck) {
                const int mid = cout / 4;
                b.nconv = 3;
                b.conv[0] = {cin, mid, 1, 1, true};
                b.conv[1] = {mid, mid, 3, stride, true};
                b.conv[2] = {mid, cout, 1, 1, false};
            } else {
                b.nconv = 2;
                b.conv[0] = {cin, cout, 3, stride, true};
                b.conv[1] = {cout, cout, 3, 1, false};
            }
            topo.push_back(std::move(b));
            cin = cout;
        }
    }
    return CBW_OK;
}

// the stem conv over the L map channels (the max-pool 3x3 stride 2 follows)
ConvShape stem_shape(int L) { return {L, 64, 7, 2, true}; }

// extents of a block's tensors over an H x W input: the first conv's output, the block's output (the second conv's:
// a bottleneck's third is 1x1 stride 1) and the projection shortcut's output
struct BlockDims {
    int h1, w1, Ho, Wo, hs, ws;
};
BlockDims block_dims(const BlockTopo& b, int H, int W) {
    BlockDims d;
    d.h1 = out_dim(H, b.conv[0].k, b.conv[0].stride);
    d.w1 = out_dim(W, b.conv[0].k, b.conv[0].stride);
    d.Ho = out_dim(d.h1, b.conv[1].k, b.conv[1].stride);
    d.Wo = out_dim(d.w1, b.conv[1].k, b.conv[1].stride);
    d.hs = out_dim(H, 1, b.sc.stride);
    d.ws = out_dim(W, 1, b.sc.stride);
    return d;
}

// one block's device weights in one tier: the bf16 scoring network, the fp32 copy (BN folded in fp32, no shortcut
// fusion) or the compensated one
struct BlockW {
    ConvW conv[3];
    int nconv = 0;
    bool has_sc = false;
    bool fused_sc = false;   // shortcut folded into conv[2] as a second K-source (bottleneck)
    ConvW sc;
    DevBuf chain_w;          // conv[0]'s weights in cbw_conv_chain's fragment order (stage-2 identity blocks: the
                             // previous block's expand launch computes this block's reduce too)
};

// e4m3 conv of the fp8 tier (conv_fp8.hip): w [Cout][k][k][Cin] e4m3 = q(w_folded * s_in / alpha), alpha [Cout]
struct ConvF8 : ConvW {
    DevBuf alpha;
};
struct BlockF8 {
    ConvF8 conv[3];
    bool has_sc = false;
    ConvF8 sc;
    float s_x = 1.f, s_t1 = 1.f, s_t2 = 1.f, s_sc = 1.f;   // activation scales of the block's tensors
    float s_out = 1.f;                                      // the next block's s_x (unused when out_bf16)
    bool out_bf16 = false;                                  // the network's last block: bf16 for the pool / fc
};

// compensated bf16 (3-term split) copy of a conv for the middle re-scoring tier: BN folded in fp32, then
// w [Cout][k][k][3 Cin] = [w_hi | w_lo | w_hi] (w_hi = bf16(w), w_lo = bf16(w - w_hi)) against activations
// stored [x_hi | x_lo] (CBW_EPI_SPLIT3) and read as the K-segments [x_hi | x_hi | x_lo] (ConvArgs::xfold),
// so one bf16 MFMA conv over 3 Cin K-channels accumulates x_hi.w_hi + x_hi.w_lo + x_lo.w_hi in fp32 (only
// x_lo.w_lo, ~2^-16 relative, is dropped)
int load_conv_bn_x3(const ParamStore& ps, const std::string& prefix, const ConvShape& s, bool relu, ConvW& c) {
    std::vector<float> o, sh;
    CHK(fold_conv_host(ps, prefix, s.cin, s.cout, s.k, o, sh));
    const size_t taps = (size_t)s.cout * s.k * s.k;
    std::vector<uint16_t> w(taps * 3 * s.cin);
    for (size_t t = 0; t < taps; ++t) split3(&o[t * s.cin], s.cin, &w[t * 3 * s.cin]);
    static_cast<ConvShape&>(c) = {3 * s.cin, s.cout, s.k, s.stride, relu};
    CHK(c.w.upload(w));
    CHK(c.b.upload(sh));
    return CBW_OK;
}

// one conv of the compensated tier: x bf16 [N][H][W][2C] = [hi | lo] (c.cin = 3C K-channels), y per flags
// (SPLIT3: bf16 [M][2 Cout] [hi | lo] + optional fp32 copy y32; OUT_F32: fp32 [M][Cout]); residual fp32
// [M][Cout] (res_split false) or a [hi | lo] tensor (res_split true)
// (w / bias: the conv's device operands, c.w / c.b of a loaded ConvW or the caller's for cbw_conv2d_x3)
int launch_conv_x3(const ConvShape& c, const void* w, const float* bias, const void* x, int N, int H, int W, void* y,
                   float* y32, const void* res, bool res_split, int flags, const void* zero, hipStream_t st, Prof* prof) {
    ConvArgs a{};
    a.x = x; a.w = w; a.bias = bias; a.res = res; a.y = y; a.y32 = y32; a.zero = zero;
    a.xfold = c.cin / 3; a.x_ld = 2 * (c.cin / 3);
    conv_geometry(a, c, N, H, W);
    a.res_ld = res_split ? 2 * c.cout : c.cout;
    a.y_ld = (flags & CBW_EPI_SPLIT3) ? 2 * c.cout : c.cout;
    a.flags = flags | (res ? (res_split ? CBW_EPI_RES_SPLIT : CBW_EPI_RES_F32) : 0) | (c.relu ? CBW_EPI_RELU : 0);
    int slot;
    CHK(Prof::begin(prof, st, &slot));
    HIPCHK(cbw_conv_igemm(a, st));
    // the compensated conv's GEMM: K over the three split segments; always tier 1
    return Prof::end(prof, slot, st, 2.0 * a.M * a.Cout * (double)a.Cin * a.KH * a.KW, cbw_last_conv_kernel, 1);
}
int launch_conv_x3(const ConvW& c, const void* x, int N, int H, int W, void* y, float* y32, const void* res,
                   bool res_split, int flags, const void* zero, hipStream_t st, Prof* prof) {
    return launch_conv_x3(c, c.w.p, c.b.as<float>(), x, N, H, W, y, y32, res, res_split, flags, zero, st, prof);
}

int launch_conv32(const ConvW& c, const float* x, int N, int H, int W, float* y, const float* res, bool relu,
                  hipStream_t st) {
    F32ConvArgs a{};
    a.x = x; a.w = c.w.as<float>(); a.bias = c.b.as<float>(); a.res = res; a.y = y;
    conv_geometry(a, c, N, H, W);
    a.relu = relu ? 1 : 0;
    HIPCHK(cbw_conv_f32(a, st));
    return CBW_OK;
}

bool sc_fusion_enabled() {   // CBW_NO_SC_FUSION=1 keeps the separate shortcut conv (A/B experiments)
    const char* e = getenv("CBW_NO_SC_FUSION");
    return !(e && atoi(e) != 0);
}

constexpr int KWS_MAX_STREAMS = 4;
// the scoring side streams' priority (CBW_KWS_PRIO, read when the handle creates them; default 0 = normal; -1 = high:
// with the caller's stream also high priority, a normal-priority stream's work -- bench.py's re-scoring tier -- only
// takes the CUs the scoring pass leaves free), clamped to the device's range
hipError_t side_stream_create(hipStream_t* s) {
    const char* e = getenv("CBW_KWS_PRIO");
    int prio = e ? atoi(e) : 0;
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess)
        prio = std::max(greatest, std::min(least, prio));
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, prio);
}

// keyword chunks round-robin over the caller's stream and kws_streams() - 1 side streams; CBW_KWS_STREAMS=1 runs every
// chunk on the caller's stream (A/B experiments).  3 with 1112-pair chunks (9 per 10k database, 3 per stream) measured
// 6.15-6.16 utt/s vs 6.07-6.10 with 2 x 834 and 5.92-5.96 with 1 (profiles/r06c_chunk_sweep.txt)
int kws_streams() {
    const char* e = getenv("CBW_KWS_STREAMS");
    const int n = e ? atoi(e) : 3;
    return std::max(1, std::min(KWS_MAX_STREAMS, n));
}

// map channels the stem reads: NHWC4 for the efficient_kws classifiers (n_layers <= 4), NHWC16 for
// the original 12-channel CB-Whisper CNN (model/model.py:55-58)
int stem_channels(int n_layers) { return n_layers <= 4 ? 4 : 16; }

bool bottleneck_first_enabled() {   // CBW_NO_BOTTLENECK_FIRST=1 keeps the stage-1 first block on three convs
    const char* e = getenv("CBW_NO_BOTTLENECK_FIRST");
    return !(e && atoi(e));
}
// the last stage-1 block stores the fp8 tier's first tensor in e4m3 itself (default; CBW_FP8_Q8=0: a bf16 tensor and
// the cbw_quant_fp8 pass, bit-identical).  r05b A/B, fp8-first bench at the realistic point: 5.853 vs 5.680 / 5.666
// utt/s, fp8 tier 115.4 vs 119.9 / 121.6 ms per clip, same spotted digest (profiles/r05b_ab.txt)
bool fp8_q8_enabled() {
    const char* e = getenv("CBW_FP8_Q8");
    return !(e && atoi(e) == 0);
}

bool bottleneck_fusion_enabled() {   // CBW_NO_BOTTLENECK_FUSION=1 runs stage-1 blocks as three convs
    const char* e = getenv("CBW_NO_BOTTLENECK_FUSION");
    return !(e && atoi(e) != 0);
}

bool stem_fusion_enabled() {   // CBW_NO_STEM_FUSION=1 runs the separate stem conv + maxpool (A/B experiments)
    const char* e = getenv("CBW_NO_STEM_FUSION");
    return !(e && atoi(e) != 0);
}

}  // namespace

struct cbw_kws {
    cbw_kws_config cfg{};
    ParamStore ps;
    bool finalized = false;
    DevBuf zero;
    DevBuf stem_w, stem_b;
    std::vector<BlockTopo> topo;   // the network (resnet_topology); blocks, blocks32 and blocks3 run parallel to it
    std::vector<BlockW> blocks;
    int hidden = 2048;
    DevBuf fc_w, fc_b;
    DevBuf fc_b16;   // the bf16 scoring pass's classifier bias: fc_b + the calibrated logit offset (cbw_kws_set_score_offset)
    DevBuf fc_b8;    // the fp8 tier's classifier bias: fc_b + its own logit offset (cbw_kws_set_score_offset_fp8)
    // projector (LE/LEF)
    std::vector<ConvW> p1, p2;
    DevBuf tp_w, tp_b;   // LEF time projector, BN folded: f32 [L][3][U][U] (k, in, out), [L][U]
    Prof prof;
    // fp32 network (exact re-scoring): stem [64][7][7][L], blocks with a separate shortcut, projector
    ConvW stem32;
    DevBuf stem16x3_w;   // compensated tier's stem: [64][7][8][16] bf16 = [w_hi | w_lo | w_hi | 0] (3 L <= 16)
    std::vector<BlockW> blocks32;
    std::vector<BlockW> blocks3;   // compensated bf16 (3-term split) convs of the middle re-scoring tier
    std::vector<ConvW> p1_32, p2_32;
    // keyword chunks rotate over the caller's stream and these side streams, so one chunk's
    // partially filled launches (tile tails, the short stage-4 convs) and memory-bound layers
    // overlap another chunk's work; fork/join by events, so the whole score call stays
    // capturable into a hipGraph.
    hipStream_t side[KWS_MAX_STREAMS - 1] = {};
    hipEvent_t fork_ev = nullptr, join_ev[KWS_MAX_STREAMS - 1] = {};
    // fp8 first tier (cbw_kws_calibrate_fp8 / cbw_kws_score_fp8): stages 2-4 of ResNet-50 on e4m3 operands,
    // blocks8[i] mirrors blocks[f8_first + i]; the stem and stage 1 run the bf16 network
    std::vector<BlockF8> blocks8;
    int f8_first = -1;
    float f8_in_scale = 1.f;   // scale of the stage-1 output, quantized by cbw_quant_fp8
    // rescore_impl's dispatch throttle: one event per RESCORE_THROTTLE passes, the host waits for the one two back
    hipEvent_t throttle_ev[2] = {};
    ~cbw_kws() {
        for (auto s : side) if (s) (void)hipStreamDestroy(s);
        for (auto e : join_ev) if (e) (void)hipEventDestroy(e);
        if (fork_ev) (void)hipEventDestroy(fork_ev);
        for (auto e : throttle_ev) if (e) (void)hipEventDestroy(e);
    }
};

struct LNorm {
    DevBuf g, b;
};
// the fields a pre-LN Whisper layer has in the encoder and the decoder alike: self-attention (ln1 -> fused qkv ->
// attention -> out) and MLP (ln_mlp -> fc1 + GELU -> fc2), each added to the fp32 residual stream
struct XfLayer {
    LNorm ln1, ln_mlp;
    ConvW qkv, out, fc1, fc2;
};

struct cbw_encoder {
    cbw_encoder_config cfg{};
    ParamStore ps;
    bool finalized = false;
    int cpad = 128;
    DevBuf zero;
    ConvW conv1, conv2;
    DevBuf pos;
    std::vector<XfLayer> layers;
    LNorm lnf;
};

namespace {

int build_resnet(cbw_kws* h) {
    const int L = h->cfg.n_layers;
    h->hidden = h->topo.back().conv[h->topo.back().nconv - 1].cout;
    const std::string root = "model.feature_extractor";
    // stem: [64][L][7][7] + BN -> bf16 [64][7][8][4]
    {
        int rc;
        const auto* w = h->ps.get(root + ".embedder.embedder.convolution.weight", (size_t)64 * L * 49, &rc);
        if (!w) return rc;
        std::vector<float> sc, sh;
        CHK(fold_bn(h->ps, root + ".embedder.embedder.normalization", 64, sc, sh));
        const int C = stem_channels(L);
        std::vector<float> o((size_t)64 * 7 * 8 * C, 0.f);
        for (int co = 0; co < 64; ++co)
            for (int c = 0; c < L; ++c)
                for (int kh = 0; kh < 7; ++kh)
                    for (int kw = 0; kw < 7; ++kw)
                        o[((co * 7 + kh) * 8 + kw) * C + c] = (*w)[((co * L + c) * 7 + kh) * 7 + kw] * sc[co];
        CHK(h->stem_w.upload(to_bf16(o)));
        CHK(h->stem_b.upload(sh));
    }
    h->blocks.clear();
    for (const BlockTopo& t : h->topo) {
        const int cin = t.conv[0].cin, mid = t.conv[0].cout, cout = t.conv[t.nconv - 1].cout;
        BlockW b;
        b.nconv = t.nconv;
        b.has_sc = t.has_sc;
        if (t.has_sc) CHK(load_conv_bn(h->ps, t.prefix + ".shortcut", t.sc, b.sc));
        for (int j = 0; j < t.nconv; ++j) {
            if (t.nconv == 3 && j == 2 && t.has_sc && cout % 128 == 0 && sc_fusion_enabled()) {
                static_cast<ConvShape&>(b.conv[2]) = t.conv[2];
                CHK(load_fused_expand_shortcut(h->ps, t.prefix + ".layer.2", t.prefix + ".shortcut", mid, cin, cout,
                                               b.conv[2]));
                b.fused_sc = true;
            } else {
                CHK(load_conv_bn(h->ps, t.prefix + ".layer." + std::to_string(j), t.conv[j], b.conv[j]));
            }
        }
        if (t.nconv == 3 && !t.has_sc && cin == 512 && mid == 128) {   // the weights never change after this (bias
            CHK(b.chain_w.alloc((size_t)mid * cin * 2));               // calibration rewrites biases only)
            HIPCHK(cbw_conv_chain_pack(b.conv[0].w.as<uint16_t>(), b.chain_w.as<uint16_t>(), nullptr));
            HIPCHK(hipStreamSynchronize(nullptr));
        }
        h->blocks.push_back(std::move(b));
    }
    int rc;
    const auto* fw = h->ps.get("model.classifier.1.weight", (size_t)2 * h->hidden, &rc);
    if (!fw) return rc;
    const auto* fb = h->ps.get("model.classifier.1.bias", 2, &rc);
    if (!fb) return rc;
    CHK(h->fc_w.upload(*fw));
    CHK(h->fc_b.upload(*fb));
    CHK(h->fc_b16.upload(*fb));
    CHK(h->fc_b8.upload(*fb));
    return CBW_OK;
}

// the projector Linears of every layer: bf16 copies, and fp32 ones beside them when the fp32 path is built
int build_projector(cbw_kws* h, bool f32) {
    const int L = h->cfg.n_layers, D = h->cfg.embedding_dim, U = h->cfg.proj_units;
    for (auto* v : {&h->p1, &h->p2, &h->p1_32, &h->p2_32}) {
        v->clear();
        v->resize(L);
    }
    for (int l = 0; l < L; ++l) {
        int rc;
        const std::string p = "projector." + std::to_string(l);
        const auto* w1 = h->ps.get(p + ".0.weight", (size_t)(D / 2) * D, &rc); if (!w1) return rc;
        const auto* b1 = h->ps.get(p + ".0.bias", D / 2, &rc); if (!b1) return rc;
        const auto* w2 = h->ps.get(p + ".2.weight", (size_t)U * (D / 2), &rc); if (!w2) return rc;
        const auto* b2 = h->ps.get(p + ".2.bias", U, &rc); if (!b2) return rc;
        auto upload = [&](const ConvShape& s, const std::vector<float>& w, const std::vector<float>& b, ConvW& c16,
                          ConvW& c32) -> int {
            static_cast<ConvShape&>(c16) = static_cast<ConvShape&>(c32) = s;
            CHK(c16.w.upload(to_bf16(w)));
            CHK(c16.b.upload(b));
            if (f32) CHK(c32.w.upload(w));
            if (f32) CHK(c32.b.upload(b));
            return CBW_OK;
        };
        CHK(upload({D, D / 2, 1, 1, true}, *w1, *b1, h->p1[l], h->p1_32[l]));
        CHK(upload({D / 2, U, 1, 1, false}, *w2, *b2, h->p2[l], h->p2_32[l]));
    }
    if (h->cfg.variant == 2) {
        std::vector<float> tw((size_t)L * 3 * U * U), tb((size_t)L * U);
        for (int l = 0; l < L; ++l) {
            int rc;
            const std::string p = "time_projector." + std::to_string(l);
            const auto* w = h->ps.get(p + ".0.weight", (size_t)U * U * 3, &rc); if (!w) return rc;
            const auto* b = h->ps.get(p + ".0.bias", U, &rc); if (!b) return rc;
            std::vector<float> sc, sh;
            CHK(fold_bn(h->ps, p + ".1", U, sc, sh));
            for (int o = 0; o < U; ++o) {
                tb[(size_t)l * U + o] = (*b)[o] * sc[o] + sh[o];
                for (int i = 0; i < U; ++i)
                    for (int k = 0; k < 3; ++k)
                        tw[(((size_t)l * 3 + k) * U + i) * U + o] = (*w)[((size_t)o * U + i) * 3 + k] * sc[o];
            }
        }
        CHK(h->tp_w.upload(tw));
        CHK(h->tp_b.upload(tb));
    }
    return CBW_OK;
}

// the fp32 network and the compensated one; the conv modules' ReLUs: fp32 per launch (launch_conv32), compensated
// in the record, where the last conv's is the block's ReLU after the residual sum
int build_f32(cbw_kws* h) {
    const int L = h->cfg.n_layers;
    const std::string stem = "model.feature_extractor.embedder.embedder";
    CHK(load_conv_bn(h->ps, stem, stem_shape(L), h->stem32, true));
    if (3 * L <= 16) {   // the compensated stem (cbw_stem16_pool_x3): taps kw padded to 8, channels [hi | lo | hi | 0]
        std::vector<float> o, sh;
        CHK(fold_conv_host(h->ps, stem, L, 64, 7, o, sh));
        std::vector<uint16_t> w16((size_t)64 * 7 * 8 * 16, 0);
        for (int co = 0; co < 64; ++co)
            for (int kh = 0; kh < 7; ++kh)
                for (int kw = 0; kw < 7; ++kw)
                    split3(&o[(((size_t)co * 7 + kh) * 7 + kw) * L], L, &w16[(((size_t)co * 7 + kh) * 8 + kw) * 16]);
        CHK(h->stem16x3_w.upload(w16));
    }
    h->blocks32.clear();
    h->blocks3.clear();
    for (const BlockTopo& t : h->topo) {
        BlockW b, b3;
        b.nconv = b3.nconv = t.nconv;
        b.has_sc = b3.has_sc = t.has_sc;
        if (t.has_sc) {
            CHK(load_conv_bn(h->ps, t.prefix + ".shortcut", t.sc, b.sc, true));
            CHK(load_conv_bn_x3(h->ps, t.prefix + ".shortcut", t.sc, false, b3.sc));
        }
        for (int j = 0; j < t.nconv; ++j) {
            const std::string p = t.prefix + ".layer." + std::to_string(j);
            CHK(load_conv_bn(h->ps, p, t.conv[j], b.conv[j], true));
            CHK(load_conv_bn_x3(h->ps, p, t.conv[j], true, b3.conv[j]));
        }
        h->blocks32.push_back(std::move(b));
        h->blocks3.push_back(std::move(b3));
    }
    return CBW_OK;
}

// OCP e4m3 (e4m3fn: bias 7, max 448, no infinities) of a float, round to nearest even, saturating
uint8_t f2e4m3_host(float f) {
    const uint8_t sign = std::signbit(f) ? 0x80 : 0;
    float a = std::fabs(f);
    if (std::isnan(a)) return 0x7F;
    if (a >= 448.f) return sign | 0x7E;
    int e;
    const float fr = std::frexp(a, &e);   // a = fr * 2^e, fr in [0.5, 1)
    if (a == 0.f) return sign;
    int E = e - 1;                        // a = 1.m * 2^E
    if (E < -6) {                         // subnormal: multiples of 2^-9
        const float q = std::nearbyint(a * 512.f);   // default rounding mode: to nearest even
        return sign | (uint8_t)q;                    // q == 8 is the smallest normal (exp field 1, mantissa 0)
    }
    float m = std::nearbyint((fr * 2.f - 1.f) * 8.f);
    if (m == 8.f) { m = 0.f; ++E; }
    if (E > 8 || (E == 8 && m == 7.f)) return sign | 0x7E;
    return sign | (uint8_t)(((E + 7) << 3) | (int)m);
}

// a folded conv (torch weight + BN of `prefix`) quantized for the fp8 tier: input tensor scale s_in folded into
// the weights, per-output-channel alpha = max_k |w s_in| / 448
float e4m3_value_host(uint8_t c) {
    const int e = (c >> 3) & 15, m = c & 7;
    const float v = e == 0 ? std::ldexp((float)m / 8.f, -6) : std::ldexp(1.f + (float)m / 8.f, e - 7);
    return (c & 0x80) ? -v : v;
}

// ... with m (the conv input's per-channel means over the calibration pairs, or null) the bias also absorbs the
// mean shift of the rounded weights, sum_{taps, c} m[c] (w - w_e4m3 alpha / s_in) -- the bf16 tier's bias
// correction (apply_bias_correction) for the e4m3 weights
int load_conv_f8(const ParamStore& ps, const std::string& prefix, const ConvShape& s, bool relu, float s_in, ConvF8& c,
                 const double* m = nullptr) {
    const int cin = s.cin, cout = s.cout;
    std::vector<float> o, sh;
    CHK(fold_conv_host(ps, prefix, cin, cout, s.k, o, sh));
    const size_t row = (size_t)s.k * s.k * cin;
    std::vector<uint8_t> q(o.size());
    std::vector<float> alpha(cout);
    for (int co = 0; co < cout; ++co) {
        float mx = 0.f;
        for (size_t i = 0; i < row; ++i) mx = std::max(mx, std::fabs(o[co * row + i] * s_in));
        const float al = mx > 0.f ? mx / 448.f : 1.f;
        alpha[co] = al;
        double corr = 0.0;
        for (size_t i = 0; i < row; ++i) {
            q[co * row + i] = f2e4m3_host(o[co * row + i] * s_in / al);
            if (m) corr += m[i % cin] * ((double)o[co * row + i] - (double)e4m3_value_host(q[co * row + i]) * al / s_in);
        }
        sh[co] = (float)((double)sh[co] + corr);
    }
    static_cast<ConvShape&>(c) = {cin, cout, s.k, s.stride, relu};
    CHK(c.w.upload(q));
    CHK(c.alpha.upload(alpha));
    CHK(c.b.upload(sh));
    return CBW_OK;
}

int launch_conv_f8(const cbw_kws* h, const ConvF8& c, const uint8_t* x, int N, int H, int W, void* y,
                   const uint8_t* res, float res_scale, bool out_bf16, float y_scale, hipStream_t st, Prof* prof) {
    F8ConvArgs a{};
    a.x = x; a.w = c.w.as<uint8_t>(); a.alpha = c.alpha.as<float>(); a.bias = c.b.as<float>();
    a.res = res; a.res_scale = res_scale; a.y = y; a.y_inv_scale = 1.f / y_scale; a.out_bf16 = out_bf16 ? 1 : 0;
    a.zero = h->zero.p;
    conv_geometry(a, c, N, H, W);
    a.relu = c.relu ? 1 : 0;
    if (!cbw_conv_fp8_supported(a)) return fail(CBW_ERR_INVALID, "fp8 conv shape not supported");
    int slot;
    CHK(Prof::begin(prof, st, &slot));
    HIPCHK(cbw_conv_fp8(a, st));
    return Prof::end(prof, slot, st, 2.0 * a.M * a.Cout * (double)a.Cin * a.KH * a.KW, cbw_last_conv_kernel);
}

// activation sizes of one pair through the network (elements): the stem conv's output, the largest of the max-pool's
// and the blocks' outputs (a projection shortcut's output has its block's output shape), the largest tensor inside
// a block
struct NetPlan {
    size_t stem = 0, big = 0, small = 0;
};

NetPlan net_plan(const cbw_kws* h, int Tk, int Tu) {
    NetPlan p;
    int H = out_dim(Tk, 7, 2), W = out_dim(Tu, 7, 2);
    p.stem = (size_t)H * W * 64;
    H = out_dim(H, 3, 2);
    W = out_dim(W, 3, 2);
    p.big = (size_t)H * W * 64;
    for (const BlockTopo& b : h->topo) {
        const BlockDims d = block_dims(b, H, W);
        p.small = std::max(p.small, (size_t)d.h1 * d.w1 * b.conv[0].cout);
        if (b.nconv == 3) p.small = std::max(p.small, (size_t)d.Ho * d.Wo * b.conv[1].cout);
        p.big = std::max(p.big, (size_t)d.Ho * d.Wo * b.conv[b.nconv - 1].cout);
        H = d.Ho;
        W = d.Wo;
    }
    return p;
}

// one chunk of the bf16 scoring pass: the stem's output shares the block buffers
struct KwsPlan {
    size_t maps = 0, big = 0, small = 0;
};

KwsPlan kws_plan(const cbw_kws* h, int Tk, int Tu, int chunk) {
    const NetPlan q = net_plan(h, Tk, Tu);
    const size_t n = (size_t)chunk;
    return {n * Tk * Tu * stem_channels(h->cfg.n_layers), n * std::max(q.stem, q.big), n * q.small};
}

}  // namespace

extern "C" {

int cbw_version(void) { return 1; }
const char* cbw_last_error(void) { return g_err.c_str(); }

// ------------------------------------------------------------------ KWS
int cbw_kws_create(const cbw_kws_config* cfg, cbw_kws** out) {
    if (!cfg || !out) return fail(CBW_ERR_INVALID, "null argument");
    if (cfg->n_layers < 1 || cfg->n_layers > 16)
        return fail(CBW_ERR_INVALID, "n_layers must be in [1, 16] (ResNet input channels: NHWC4 or NHWC16 maps)");
    if (cfg->n_layers > 4 && cfg->variant != 0)
        return fail(CBW_ERR_INVALID, "more than 4 layers only without projection (variant 0: the 12-channel CNN)");
    if (cfg->variant < 0 || cfg->variant > 2) return fail(CBW_ERR_INVALID, "variant must be 0 (L), 1 (LE), 2 (LEF)");
    if (cfg->variant > 0 && (cfg->embedding_dim % 128 != 0 || cfg->proj_units != 64))
        return fail(CBW_ERR_INVALID, "LE/LEF need embedding_dim % 128 == 0 and proj_mlp_units == 64");
    if (cfg->variant == 0 && cfg->embedding_dim % 32 != 0)
        return fail(CBW_ERR_INVALID, "L variant needs embedding_dim % 32 == 0");
    auto h = std::make_unique<cbw_kws>();
    h->cfg = *cfg;
    CHK(h->zero.alloc(256));
    HIPCHK(hipMemset(h->zero.p, 0, 256));
    *out = h.release();
    return CBW_OK;
}

int cbw_kws_destroy(cbw_kws* h) {
    delete h;
    return CBW_OK;
}

int cbw_kws_set_param(cbw_kws* h, const char* name, const float* host, int64_t numel) {
    if (!h) return fail(CBW_ERR_INVALID, "null handle");
    h->finalized = false;
    return h->ps.set(name, host, numel);
}

int cbw_kws_finalize(cbw_kws* h) {
    if (!h) return fail(CBW_ERR_INVALID, "null handle");
    const bool f32 = h->cfg.n_layers <= 4;   // the fp32 and compensated networks (the fp32 stem's input channels)
    CHK(resnet_topology(h->cfg.resnet_depth, h->topo));
    CHK(build_resnet(h));
    if (h->cfg.variant > 0) CHK(build_projector(h, f32));
    if (f32) CHK(build_f32(h));
    if (!h->fork_ev) {
        // only the side streams CBW_KWS_STREAMS asks for (more are created on first use, ChunkStreams::begin):
        // a process gets GPU_MAX_HW_QUEUES = 4 hardware queues, and streams beyond that share one in order
        HIPCHK(hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
        for (int i = 0; i < KWS_MAX_STREAMS - 1; ++i) HIPCHK(hipEventCreateWithFlags(&h->join_ev[i], hipEventDisableTiming));
        const char* all = getenv("CBW_KWS_ALL_SIDE");   // 1: all three side streams up front (the round-1 setup, A/B)
        const int nside = (all && atoi(all) == 1) ? KWS_MAX_STREAMS - 1 : kws_streams() - 1;
        for (int i = 0; i < nside; ++i) HIPCHK(side_stream_create(&h->side[i]));
    }
    h->finalized = true;
    return CBW_OK;
}

int64_t cbw_kws_project_workspace_bytes(cbw_kws* h, int B, int T) {
    if (!h) return -1;
    const int L = h->cfg.n_layers, D = h->cfg.embedding_dim, U = h->cfg.proj_units;
    const size_t rows = (size_t)L * B * T;
    return (int64_t)(align_up(rows * D * 2) + align_up(rows * (D / 2) * 2) + align_up(rows * U * 4));
}

int cbw_kws_project(cbw_kws* h, const float* x, const float* mask, int B, int T, uint16_t* out, float* mask_out,
                    void* ws, int64_t ws_bytes, cbw_stream_t stream) {
    if (!h || !x || !mask || !out || !mask_out) return fail(CBW_ERR_INVALID, "null argument");
    if (!h->finalized) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called");
    if (B <= 0 || T <= 0) return fail(CBW_ERR_INVALID, "B and T must be positive");
    hipStream_t st = (hipStream_t)stream;
    const int L = h->cfg.n_layers, D = h->cfg.embedding_dim, U = h->cfg.proj_units;
    const float eps = 1e-6f;
    if (h->cfg.variant == 0) {
        HIPCHK(cbw_normalize_rows(x, 1, out, 0, 1, B * L, T, D, eps, 0, st));
        HIPCHK(hipMemcpyAsync(mask_out, mask, sizeof(float) * B * L * T, hipMemcpyDeviceToDevice, st));
        return CBW_OK;
    }
    if (ws_bytes < cbw_kws_project_workspace_bytes(h, B, T)) return fail(CBW_ERR_OOM, "projection workspace too small");
    const size_t rows_l = (size_t)B * T;
    char* p = (char*)ws;
    uint16_t* xb = (uint16_t*)p; p += align_up(rows_l * L * D * 2);
    uint16_t* h1 = (uint16_t*)p; p += align_up(rows_l * L * (D / 2) * 2);
    float* h2 = (float*)p;
    HIPCHK(cbw_cast_permute_lbtd(x, xb, B, L, T, D, st));
    for (int l = 0; l < L; ++l) {
        CHK(launch_conv(h->p1[l], xb + (size_t)l * rows_l * D, 1, 1, (int)rows_l, h1 + (size_t)l * rows_l * (D / 2),
                        nullptr, 0, h->zero.p, st));
        CHK(launch_conv(h->p2[l], h1 + (size_t)l * rows_l * (D / 2), 1, 1, (int)rows_l, h2 + (size_t)l * rows_l * U,
                        nullptr, CBW_EPI_OUT_F32, h->zero.p, st));
    }
    if (h->cfg.variant == 1) {
        HIPCHK(cbw_normalize_rows(h2, 1, out, 0, L, B, T, U, eps, 1, st));
        HIPCHK(hipMemcpyAsync(mask_out, mask, sizeof(float) * B * L * T, hipMemcpyDeviceToDevice, st));
    } else {
        HIPCHK(cbw_lef_time_project(h2, h->tp_w.as<float>(), h->tp_b.as<float>(), out, 0, mask, mask_out, L, B, T, U, eps,
                                    st));
    }
    return CBW_OK;
}

}  // extern "C"

namespace {
int64_t chunk_ws_bytes(const cbw_kws* h, int Tk, int Tu, int chunk) {
    const KwsPlan p = kws_plan(h, Tk, Tu, chunk);
    return (int64_t)(align_up(p.maps * 2) + 3 * align_up(p.big * 2) + 2 * align_up(p.small * 2));
}
}  // namespace

extern "C" {

int64_t cbw_kws_workspace_bytes(cbw_kws* h, int Tk, int Tu, int chunk) {
    if (!h || !h->finalized || chunk <= 0) return -1;
    return kws_streams() * chunk_ws_bytes(h, Tk, Tu, chunk);
}

namespace {
// Chunk i runs on stream i % n (0 = caller's stream, then the handle's side streams) with
// workspace slot i % n.  begin(): the side streams wait for work already queued on the caller's
// stream (inputs); end(): the caller's stream waits for every side stream, so completion on the
// caller's stream means every chunk is done.
// With several streams the streaming 1x1 convs (HBM-bound) size their persistent grid for 3/8 of the CUs (96 of 256),
// leaving the rest to the other streams' MFMA-bound convs (CBW_CS_SHARED_CUS overrides; 0 = the whole chip): 6.16 vs
// 6.10 utt/s in the bench (r06l, profiles/r06l_cs_cus_ab.txt).
int cs_shared_cus() {
    const char* e = getenv("CBW_CS_SHARED_CUS");
    if (e) return atoi(e);
    return cbw_num_cus() * 3 / 8;
}
struct ChunkStreams {
    cbw_kws* h;
    hipStream_t st;
    int n;
    int saved_cus;
    // the fewest streams that keep the same number of chunk rounds (4 chunks: 2 streams x 2, not 3 streams with one
    // running its second chunk alone; C2's 1000 keywords in chunks of 250)
    static int balanced(int want, int nchunks) {
        const int n = std::max(1, std::min(want, nchunks));
        const int rounds = (nchunks + n - 1) / n;
        return std::max(1, (nchunks + rounds - 1) / rounds);
    }
    ChunkStreams(cbw_kws* h_, hipStream_t st_, int nchunks)
        : h(h_), st(st_), n(h_->fork_ev ? balanced(kws_streams(), nchunks) : 1), saved_cus(cbw_cs_grid_cus) {
        if (n > 1) cbw_cs_grid_cus = cs_shared_cus();
    }
    ~ChunkStreams() { cbw_cs_grid_cus = saved_cus; }
    ChunkStreams(const ChunkStreams&) = delete;
    ChunkStreams& operator=(const ChunkStreams&) = delete;
    int begin() {
        if (n > 1) {
            HIPCHK(hipEventRecord(h->fork_ev, st));
            for (int i = 0; i + 1 < n; ++i) {
                if (!h->side[i]) HIPCHK(side_stream_create(&h->side[i]));
                HIPCHK(hipStreamWaitEvent(h->side[i], h->fork_ev, 0));
            }
        }
        return CBW_OK;
    }
    hipStream_t stream(int i) const { return (i % n) ? h->side[i % n - 1] : st; }
    int slot(int i) const { return i % n; }
    int end() {
        for (int i = 0; i + 1 < n; ++i) {
            HIPCHK(hipEventRecord(h->join_ev[i], h->side[i]));
            HIPCHK(hipStreamWaitEvent(st, h->join_ev[i], 0));
        }
        return CBW_OK;
    }
};

// ResNet over NHWC4 / NHWC16 maps already in `maps` (chunk of kc pairs) -> logits
int resnet_chunk(cbw_kws* h, const KwsPlan& plan, char* ws, int kc, int Tk, int Tu, float* logits, hipStream_t st,
                 bool fp8 = false) {
    char* p = ws + align_up(plan.maps * 2);
    uint16_t* maps = (uint16_t*)ws;
    uint16_t* X = (uint16_t*)p; p += align_up(plan.big * 2);
    uint16_t* Y = (uint16_t*)p; p += align_up(plan.big * 2);
    uint16_t* SC = (uint16_t*)p; p += align_up(plan.big * 2);
    uint16_t* T1 = (uint16_t*)p; p += align_up(plan.small * 2);
    uint16_t* T2 = (uint16_t*)p;
    const int Hs = out_dim(Tk, 7, 2), Ws = out_dim(Tu, 7, 2);
    const int Hp = out_dim(Hs, 3, 2), Wp = out_dim(Ws, 3, 2);
    const int L = h->cfg.n_layers;

    // stem + max-pool of pairs [n0, n0 + nn) into X (every tensor of the chunk is [pair][H][W][C], so a pair range
    // is a contiguous slice of each buffer)
    auto stem = [&](int n0, int nn) -> int {
        uint16_t* xo = X + (size_t)n0 * Hp * Wp * 64;
        const uint16_t* mo = maps + (size_t)n0 * Tk * Tu * stem_channels(L);
        if (stem_channels(L) == 16) {
            HIPCHK(cbw_stem16_pool(mo, h->stem_w.as<uint16_t>(), h->stem_b.as<float>(), xo, nn, Tk, Tu, Hs, Ws, Hp, Wp,
                                   st));
        } else if (stem_fusion_enabled()) {
            HIPCHK(cbw_stem_pool(mo, h->stem_w.as<uint16_t>(), h->stem_b.as<float>(), xo, nn, Tk, Tu, Hs, Ws, Hp, Wp,
                                 st));
        } else {
            uint16_t* yo = Y + (size_t)n0 * Hs * Ws * 64;
            HIPCHK(cbw_stem_conv(mo, h->stem_w.as<uint16_t>(), h->stem_b.as<float>(), yo, nn, Tk, Tu, Hs, Ws, st));
            HIPCHK(cbw_maxpool3s2(yo, xo, nn, Hs, Ws, 64, Hp, Wp, st));
        }
        return CBW_OK;
    };
    // blocks [b0, b1) over pairs [n0, n0 + nn): x / y are the ping-pong buffers' bases, swapped per block
    auto blocks = [&](size_t b0, size_t b1, int n0, int nn, uint16_t*& x, uint16_t*& y, int& H, int& W,
                      int& C) -> int {
        auto at = [&](uint16_t* base, int hh, int ww, int cc) { return base + (size_t)n0 * hh * ww * cc; };
        bool t1_ready = false;   // the previous block's chained expand launch already wrote this block's T1
        for (size_t bi = b0; bi < b1; ++bi) {
            const auto& b = h->blocks[bi];
            const BlockDims d = block_dims(h->topo[bi], H, W);
            const int Ho = d.Ho, Wo = d.Wo;
            uint16_t* xo = at(x, H, W, C);
            const void* res = xo;
            const bool s1_first = b.nconv == 3 && b.has_sc && b.fused_sc && b.sc.stride == 1 && b.sc.cin == 64 &&
                                  b.conv[0].cin == 64 && b.conv[0].cout == 64 && b.conv[1].stride == 1 &&
                                  b.conv[2].cout == 256 && bottleneck_fusion_enabled() && bottleneck_first_enabled();
            if (b.has_sc && !b.fused_sc) {
                uint16_t* sco = at(SC, d.hs, d.ws, b.sc.cout);
                CHK(launch_conv(b.sc, xo, nn, H, W, sco, nullptr, 0, h->zero.p, st, &h->prof));
                res = sco;
            }
            if (s1_first || (b.nconv == 3 && !b.has_sc && b.conv[0].cin == 256 && b.conv[0].cout == 64 &&
                             b.conv[2].cout == 256 && bottleneck_fusion_enabled())) {
                // stage-1 block as one fused kernel (bottleneck.hip): the identity blocks, and the first block with
                // its shortcut folded into the expand
                uint16_t* yo = at(y, H, W, 256);
                int slot;
                CHK(Prof::begin(&h->prof, st, &slot));
                if (s1_first)
                    HIPCHK(cbw_bottleneck_s1_first(xo, yo, b.conv[0].w.as<uint16_t>(), b.conv[0].b.as<float>(),
                                                   b.conv[1].w.as<uint16_t>(), b.conv[1].b.as<float>(),
                                                   b.conv[2].w.as<uint16_t>(), b.conv[2].b.as<float>(), h->zero.p, nn,
                                                   H, W, st));
                else
                    HIPCHK(cbw_bottleneck_s1(xo, yo, b.conv[0].w.as<uint16_t>(), b.conv[0].b.as<float>(),
                                             b.conv[1].w.as<uint16_t>(), b.conv[1].b.as<float>(),
                                             b.conv[2].w.as<uint16_t>(), b.conv[2].b.as<float>(), h->zero.p, nn, H, W,
                                             st));
                const double cin = s1_first ? 64.0 : 256.0;
                CHK(Prof::end(&h->prof, slot, st,
                              2.0 * nn * H * W * (cin * 64 + 64.0 * 576 + 64.0 * 256 + (s1_first ? 64.0 * 256 : 0.0)),
                              s1_first ? "bottleneck_kernel<64>" : "bottleneck_ring_kernel"));
            } else if (b.nconv == 3) {
                const auto &c0 = b.conv[0], &c1 = b.conv[1], &c2 = b.conv[2];
                uint16_t* t1 = at(T1, d.h1, d.w1, c0.cout);
                uint16_t* t2 = at(T2, Ho, Wo, c1.cout);
                uint16_t* yo = at(y, Ho, Wo, c2.cout);
                if (!t1_ready) CHK(launch_conv(c0, xo, nn, H, W, t1, nullptr, 0, h->zero.p, st, &h->prof));
                CHK(launch_conv(c1, t1, nn, d.h1, d.w1, t2, nullptr, 0, h->zero.p, st, &h->prof));
                // identity block followed by an identity block whose reduce qualifies (ResNet-50 s2b1 -> s2b2 -> s2b3):
                // T1 is free here (c1 above consumed it earlier on this stream) and takes the next block's reduce
                t1_ready = false;
                if (!b.has_sc && bi + 1 < b1 && h->blocks[bi + 1].nconv == 3 && !h->blocks[bi + 1].has_sc) {
                    const auto& nb = h->blocks[bi + 1];
                    CHK(launch_chain(c2, nb.conv[0], nb.chain_w, t2, nn, Ho, Wo, yo, res, at(T1, Ho, Wo, nb.conv[0].cout),
                                     h->zero.p, st, &h->prof, &t1_ready));
                }
                if (t1_ready) {   // y and the next T1 are written
                } else if (b.fused_sc) {   // y = relu([T2 | x strided] . [W_expand ; W_shortcut] + b): no shortcut tensor
                    const Src2 s2{xo, b.sc.cin, H, W, b.sc.stride};
                    CHK(launch_conv(c2, t2, nn, Ho, Wo, yo, nullptr, CBW_EPI_RELU, h->zero.p, st, &h->prof, &s2));
                } else {
                    CHK(launch_conv(c2, t2, nn, Ho, Wo, yo, res, CBW_EPI_RELU, h->zero.p, st, &h->prof));
                }
            } else {
                const auto &c0 = b.conv[0], &c1 = b.conv[1];
                uint16_t* t1 = at(T1, Ho, Wo, c0.cout);
                uint16_t* yo = at(y, Ho, Wo, c1.cout);
                CHK(launch_conv(c0, xo, nn, H, W, t1, nullptr, 0, h->zero.p, st, &h->prof));
                CHK(launch_conv(c1, t1, nn, Ho, Wo, yo, res, CBW_EPI_RELU, h->zero.p, st, &h->prof));
            }
            std::swap(x, y);
            H = Ho;
            W = Wo;
            C = b.conv[b.nconv - 1].cout;
        }
        return CBW_OK;
    };

    if (fp8) {   // the fp8 tier: stem + stage 1 in bf16, then the e4m3 blocks (conv_fp8.hip)
        int H = Hp, W = Wp, C = 64;
        uint16_t *x = X, *y = Y;
        CHK(stem(0, kc));
        // the last stage-1 block stores its output in e4m3 when it runs fused (bottleneck.hip, Q8; CBW_FP8_Q8=0 off):
        // no separate quantization pass; otherwise the bf16 output is quantized by cbw_quant_fp8 (same values)
        if (h->f8_first < 1) return fail(CBW_ERR_STATE, "fp8 tier: no bf16 stage before the e4m3 blocks");
        const size_t lb = (size_t)h->f8_first - 1;
        const auto& b1 = h->blocks[lb];
        const bool q8 = fp8_q8_enabled() && b1.nconv == 3 && !b1.has_sc && b1.conv[0].cin == 256 &&
                        b1.conv[0].cout == 64 && b1.conv[2].cout == 256 && bottleneck_fusion_enabled();
        CHK(blocks(0, q8 ? lb : (size_t)h->f8_first, 0, kc, x, y, H, W, C));
        uint8_t* cur = (uint8_t*)y;
        uint8_t* other = (uint8_t*)x;
        if (q8) {
            int slot;
            CHK(Prof::begin(&h->prof, st, &slot));
            HIPCHK(cbw_bottleneck_s1_q8(x, cur, b1.conv[0].w.as<uint16_t>(), b1.conv[0].b.as<float>(),
                                        b1.conv[1].w.as<uint16_t>(), b1.conv[1].b.as<float>(), b1.conv[2].w.as<uint16_t>(),
                                        b1.conv[2].b.as<float>(), 1.f / h->f8_in_scale, kc, H, W, st));
            CHK(Prof::end(&h->prof, slot, st, 2.0 * kc * H * W * (256.0 * 64 + 64.0 * 576 + 64.0 * 256),
                          "bottleneck_ring_kernel (e4m3 out)"));
            C = 256;
        } else {
            HIPCHK(cbw_quant_fp8(x, cur, (int64_t)kc * H * W * C, 1.f / h->f8_in_scale, st));
        }
        uint8_t* sc8 = (uint8_t*)SC;
        uint8_t* t1 = (uint8_t*)T1;
        uint8_t* t2 = (uint8_t*)T2;
        for (size_t i = 0; i < h->blocks8.size(); ++i) {
            const BlockF8& b = h->blocks8[i];
            const BlockDims d = block_dims(h->topo[h->f8_first + i], H, W);
            const uint8_t* res = cur;
            float rs = b.s_x;
            if (b.has_sc) {
                CHK(launch_conv_f8(h, b.sc, cur, kc, H, W, sc8, nullptr, 0.f, false, b.s_sc, st, &h->prof));
                res = sc8;
                rs = b.s_sc;
            }
            CHK(launch_conv_f8(h, b.conv[0], cur, kc, H, W, t1, nullptr, 0.f, false, b.s_t1, st, &h->prof));
            CHK(launch_conv_f8(h, b.conv[1], t1, kc, d.h1, d.w1, t2, nullptr, 0.f, false, b.s_t2, st, &h->prof));
            CHK(launch_conv_f8(h, b.conv[2], t2, kc, d.Ho, d.Wo, other, res, rs, b.out_bf16, b.s_out, st, &h->prof));
            std::swap(cur, other);
            H = d.Ho;
            W = d.Wo;
            C = b.conv[2].cout;
        }
        HIPCHK(cbw_pool_fc((const uint16_t*)cur, h->fc_w.as<float>(), h->fc_b8.as<float>(), logits, kc, H * W, C, st));
        return CBW_OK;
    }
    int H = Hp, W = Wp, C = 64;
    uint16_t *x = X, *y = Y;
    CHK(stem(0, kc));
    CHK(blocks(0, h->blocks.size(), 0, kc, x, y, H, W, C));
    HIPCHK(cbw_pool_fc(x, h->fc_w.as<float>(), h->fc_b16.as<float>(), logits, kc, H * W, C, st));
    return CBW_OK;
}

// The chunk loop of the scoring entry points: maps [0, n) in chunks of `chunk`, chunk i on ChunkStreams' stream and
// workspace slot i % n.  Per chunk, in this order on its stream: fill(p0, pc, maps, stream) writes the NHWC maps of
// [p0, p0 + pc) into the slot, the optional fp32 copy goes to features [n][L][Tk][Tu], then the network writes
// logits [n][2].  The callers have validated everything but the workspace size.
extern "C++" {
template <class Fill>
int score_chunks(cbw_kws* h, int n, int Tk, int Tu, float* logits, float* features, int chunk, void* ws,
                 int64_t ws_bytes, hipStream_t st, bool fp8, Fill fill) {
    const int L = h->cfg.n_layers;
    const KwsPlan plan = kws_plan(h, Tk, Tu, chunk);
    const int64_t per = chunk_ws_bytes(h, Tk, Tu, chunk);
    if (ws_bytes < kws_streams() * per) return fail(CBW_ERR_OOM, "score workspace too small");
    ChunkStreams cs(h, st, (n + chunk - 1) / chunk);
    CHK(cs.begin());
    for (int p0 = 0, i = 0; p0 < n; p0 += chunk, ++i) {
        const int pc = std::min(chunk, n - p0);
        hipStream_t s = cs.stream(i);
        char* w = (char*)ws + cs.slot(i) * per;
        CHK(fill(p0, pc, (uint16_t*)w, s));
        if (features) HIPCHK(cbw_sim_to_nchw((uint16_t*)w, features + (size_t)p0 * L * Tk * Tu, pc, L, Tk, Tu, s));
        CHK(resnet_chunk(h, plan, w, pc, Tk, Tu, logits + (size_t)p0 * 2, s, fp8));
    }
    return cs.end();
}

// fill for one utterance against keywords [p0, p0 + pc) (cbw_kws_score, cbw_kws_score_fp8)
auto sim_maps_fill(const cbw_kws* h, const uint16_t* utt, const float* utt_mask, const uint16_t* kwd,
                   const float* kwd_mask, int Tk, int Tu) {
    const int L = h->cfg.n_layers;
    const int E = h->cfg.variant == 0 ? h->cfg.embedding_dim : h->cfg.proj_units;
    return [=](int p0, int pc, uint16_t* maps, hipStream_t s) -> int {
        HIPCHK(cbw_sim_maps(kwd + (size_t)p0 * L * Tk * E, kwd_mask + (size_t)p0 * L * Tk, utt, utt_mask, maps, pc, L,
                            Tk, Tu, E, s));
        return CBW_OK;
    };
}
}  // extern "C++"
}  // namespace

int cbw_kws_score(cbw_kws* h, const uint16_t* utt, const float* utt_mask, const uint16_t* kwd, const float* kwd_mask,
                  int K, int Tk, int Tu, float* logits, float* features, int chunk, void* ws, int64_t ws_bytes,
                  cbw_stream_t stream) {
    if (!h || !utt || !utt_mask || (K > 0 && (!kwd || !kwd_mask || !logits))) return fail(CBW_ERR_INVALID, "null argument");
    if (!h->finalized) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called");
    if (K == 0) return CBW_OK;
    if (K < 0 || Tk < 7 || Tu < 7 || chunk <= 0) return fail(CBW_ERR_INVALID, "bad K/Tk/Tu/chunk");
    return score_chunks(h, K, Tk, Tu, logits, features, chunk, ws, ws_bytes, (hipStream_t)stream, false,
                        sim_maps_fill(h, utt, utt_mask, kwd, kwd_mask, Tk, Tu));
}

int cbw_kws_score_pairs(cbw_kws* h, const uint16_t* utt, const float* utt_mask, int B, const uint16_t* kwd,
                        const float* kwd_mask, int K, int Tk, int Tu, const int32_t* pair_utt, const int32_t* pair_kwd,
                        int P, float* logits, float* features, int chunk, void* ws, int64_t ws_bytes,
                        cbw_stream_t stream) {
    if (!h || (P > 0 && (!utt || !utt_mask || !kwd || !kwd_mask || !logits))) return fail(CBW_ERR_INVALID, "null argument");
    if (!h->finalized) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called");
    if (B < 1 || P < 0) return fail(CBW_ERR_INVALID, "bad B/P");
    if (P == 0) return CBW_OK;
    if (K < 1 || Tk < 7 || Tu < 7 || chunk <= 0) return fail(CBW_ERR_INVALID, "bad K/Tk/Tu/chunk");
    if ((pair_utt == nullptr) != (pair_kwd == nullptr))
        return fail(CBW_ERR_INVALID, "pair_utt and pair_kwd must both be given or both be null");
    if (!pair_utt && (int64_t)P != (int64_t)B * K)
        return fail(CBW_ERR_INVALID, "without index arrays P must be B * K (every utterance against every keyword)");
    const int L = h->cfg.n_layers;
    const int E = h->cfg.variant == 0 ? h->cfg.embedding_dim : h->cfg.proj_units;
    return score_chunks(h, P, Tk, Tu, logits, features, chunk, ws, ws_bytes, (hipStream_t)stream, false,
                        [=](int p0, int pc, uint16_t* maps, hipStream_t s) -> int {
                            HIPCHK(cbw_sim_maps_pairs(kwd, kwd_mask, K, utt, utt_mask, B,
                                                      pair_utt ? pair_utt + p0 : nullptr,
                                                      pair_kwd ? pair_kwd + p0 : nullptr, p0, maps, pc, L, Tk, Tu, E, s));
                            return CBW_OK;
                        });
}

int cbw_kws_score_fp8(cbw_kws* h, const uint16_t* utt, const float* utt_mask, const uint16_t* kwd,
                      const float* kwd_mask, int K, int Tk, int Tu, float* logits, int chunk, void* ws, int64_t ws_bytes,
                      cbw_stream_t stream) {
    if (!h || !utt || !utt_mask || (K > 0 && (!kwd || !kwd_mask || !logits))) return fail(CBW_ERR_INVALID, "null argument");
    if (!h->finalized) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called");
    if (h->blocks8.empty() || h->f8_first < 0) return fail(CBW_ERR_STATE, "fp8 tier not calibrated (cbw_kws_calibrate_fp8)");
    if (K == 0) return CBW_OK;
    if (K < 0 || Tk < 7 || Tu < 7 || chunk <= 0) return fail(CBW_ERR_INVALID, "bad K/Tk/Tu/chunk");
    const TierScope tier(h->prof, 2);   // this call's profile records are the fp8 tier's
    return score_chunks(h, K, Tk, Tu, logits, nullptr, chunk, ws, ws_bytes, (hipStream_t)stream, true,
                        sim_maps_fill(h, utt, utt_mask, kwd, kwd_mask, Tk, Tu));
}

int cbw_kws_set_score_offset_fp8(cbw_kws* h, const float* offset) {
    if (!h || !offset) return fail(CBW_ERR_INVALID, "null argument");
    if (!h->finalized || h->fc_b8.bytes != 2 * sizeof(float)) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called");
    int rc;
    const auto* fb = h->ps.get("model.classifier.1.bias", 2, &rc);
    if (!fb) return rc;
    const float b[2] = {(*fb)[0] + offset[0], (*fb)[1] + offset[1]};
    // the bias is read by scoring launches on any stream: drain the device before overwriting it in place
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h->fc_b8.p, b, sizeof(b), hipMemcpyHostToDevice));
    return CBW_OK;
}

int cbw_kws_fp8_scales(cbw_kws* h, float* scales, int max_n) {
    if (!h || (max_n > 0 && !scales)) return fail(CBW_ERR_INVALID, "null argument");
    const int n = (int)h->blocks8.size() * 4 + 1;
    if (max_n >= 1) scales[0] = h->f8_in_scale;
    for (size_t i = 0; i < h->blocks8.size(); ++i) {
        const BlockF8& b = h->blocks8[i];
        const float v[4] = {b.s_x, b.s_t1, b.s_t2, b.has_sc ? b.s_sc : 0.f};
        for (int j = 0; j < 4; ++j)
            if ((int)(1 + 4 * i + j) < max_n) scales[1 + 4 * i + j] = v[j];
    }
    return n;
}

int cbw_conv2d_fp8(const uint8_t* x, const uint8_t* w, const float* alpha, const float* bias, const uint8_t* res,
                   float res_scale, void* y, float y_scale, int out_bf16, int relu, int N, int H, int W, int Cin,
                   int Cout, int k, int stride, cbw_stream_t stream) {
    const void* zp = nullptr;
    CHK(block_zero_page(&zp));
    F8ConvArgs a{};
    a.x = x; a.w = w; a.alpha = alpha; a.bias = bias; a.res = res; a.res_scale = res_scale; a.y = y;
    a.y_inv_scale = 1.f / y_scale; a.out_bf16 = out_bf16; a.zero = zp; a.relu = relu;
    conv_geometry(a, {Cin, Cout, k, stride}, N, H, W);
    if (!cbw_conv_fp8_supported(a) || y_scale <= 0.f)
        return fail(CBW_ERR_INVALID, "cbw_conv2d_fp8: 1x1 / 3x3, Cin % 128 == 0, Cout % 128 == 0, positive scales");
    HIPCHK(cbw_conv_fp8(a, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_fp8_probe(int what, const void* a, const void* b, void* out, void* out2, int n, cbw_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    if (what >= 0 && what <= 3) {   // the MFMA operand map: a = A [16][128] e4m3, b = B^T [16][128], out = C f32 [16][16]
        HIPCHK(cbw_mfma_fp8_probe((const uint8_t*)a, (const uint8_t*)b, (float*)out, what, st));
        return CBW_OK;
    }
    if (what == 4) {   // conversions: a = f32 [n] -> out = e4m3 [n] (saturating), out2 = f32 [n] decoded
        HIPCHK(cbw_cvt_fp8_probe((const float*)a, (uint8_t*)out, (float*)out2, n, st));
        return CBW_OK;
    }
    return fail(CBW_ERR_INVALID, "cbw_fp8_probe: what in 0..4");
}

int cbw_kws_classify(cbw_kws* h, const float* maps_nchw, int K, int Tk, int Tu, float* logits, int chunk, void* ws,
                     int64_t ws_bytes, cbw_stream_t stream) {
    if (!h || (K > 0 && (!maps_nchw || !logits))) return fail(CBW_ERR_INVALID, "null argument");
    if (!h->finalized) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called");
    if (K == 0) return CBW_OK;
    if (K < 0 || Tk < 7 || Tu < 7 || chunk <= 0) return fail(CBW_ERR_INVALID, "bad K/Tk/Tu/chunk");
    const int L = h->cfg.n_layers;
    return score_chunks(h, K, Tk, Tu, logits, nullptr, chunk, ws, ws_bytes, (hipStream_t)stream, false,
                        [=](int p0, int pc, uint16_t* maps, hipStream_t s) -> int {
                            const float* src = maps_nchw + (size_t)p0 * L * Tk * Tu;
                            if (stem_channels(L) == 16) HIPCHK(cbw_nchw_to_nhwc16(src, maps, pc, L, Tk, Tu, s));
                            else HIPCHK(cbw_nchw_to_nhwc4(src, maps, pc, L, Tk, Tu, s));
                            return CBW_OK;
                        });
}

// ---- CB-Whisper original spotter (cb_whisper.py:93-129, :189-210)
namespace {
struct ResizedWs {
    int TuP = 0;
    int64_t rmax = 0, utt_bytes = 0, sim_bytes = 0, chunk_bytes = 0;
};
int resized_ws(const cbw_kws* h, const int32_t* off_host, int K, int Tu, int D, int Ho, int Wo, int chunk,
               ResizedWs& r) {
    if (!off_host || K < 0 || Tu <= 0 || D <= 0 || Ho < 7 || Wo < 7 || chunk <= 0)
        return fail(CBW_ERR_INVALID, "bad arguments");
    const int L = h->cfg.n_layers;
    r.TuP = (Tu + 127) / 128 * 128;
    r.rmax = 0;
    for (int k0 = 0; k0 < K; k0 += chunk) {
        const int kc = std::min(chunk, K - k0);
        const int64_t rows = (int64_t)off_host[k0 + kc] - off_host[k0];
        for (int k = k0; k < k0 + kc; ++k)
            if (off_host[k + 1] <= off_host[k]) return fail(CBW_ERR_INVALID, "every keyword needs >= 1 frame");
        r.rmax = std::max(r.rmax, rows);
    }
    r.utt_bytes = (int64_t)align_up((size_t)L * r.TuP * D * 2);
    r.sim_bytes = (int64_t)align_up((size_t)L * std::max<int64_t>(r.rmax, 1) * r.TuP * 4);
    r.chunk_bytes = chunk_ws_bytes(h, Ho, Wo, chunk);
    return CBW_OK;
}
}  // namespace

int64_t cbw_kws_score_resized_workspace_bytes(cbw_kws* h, const int32_t* off_host, int K, int Tu, int D, int Ho,
                                              int Wo, int chunk) {
    if (!h || !h->finalized) return -1;
    ResizedWs r;
    if (resized_ws(h, off_host, K, Tu, D, Ho, Wo, chunk, r) != CBW_OK) return -1;
    return r.utt_bytes + r.sim_bytes + r.chunk_bytes;
}

int cbw_kws_score_resized(cbw_kws* h, const uint16_t* utt, int Tu, const uint16_t* kwd, int R, int D,
                          const int32_t* off_dev, const int32_t* off_host, int K, int Ho, int Wo, float* logits,
                          int chunk, void* ws, int64_t ws_bytes, cbw_stream_t stream) {
    if (!h || !utt || (K > 0 && (!kwd || !off_dev || !off_host || !logits))) return fail(CBW_ERR_INVALID, "null argument");
    if (!h->finalized) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called");
    if (h->cfg.variant != 0) return fail(CBW_ERR_INVALID, "the resized-similarity path takes raw hs (variant 0)");
    if (K == 0) return CBW_OK;
    if (D % 64) return fail(CBW_ERR_INVALID, "D must be a multiple of 64");
    ResizedWs r;
    CHK(resized_ws(h, off_host, K, Tu, D, Ho, Wo, chunk, r));
    if (off_host[0] < 0 || off_host[K] > R) return fail(CBW_ERR_INVALID, "keyword rows out of range");
    if (ws_bytes < r.utt_bytes + r.sim_bytes + r.chunk_bytes) return fail(CBW_ERR_OOM, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int L = h->cfg.n_layers;
    char* p = (char*)ws;
    uint16_t* uttP = (uint16_t*)p; p += r.utt_bytes;
    float* sims = (float*)p; p += r.sim_bytes;
    char* cws = p;
    // utterance rows zero-padded to a multiple of 128: they are the GEMM's output channels
    HIPCHK(hipMemsetAsync(uttP, 0, r.utt_bytes, st));
    HIPCHK(hipMemcpy2DAsync(uttP, (size_t)r.TuP * D * 2, utt, (size_t)Tu * D * 2, (size_t)Tu * D * 2, L,
                            hipMemcpyDeviceToDevice, st));
    const KwsPlan plan = kws_plan(h, Ho, Wo, chunk);
    for (int k0 = 0; k0 < K; k0 += chunk) {
        const int kc = std::min(chunk, K - k0);
        const int rows = off_host[k0 + kc] - off_host[k0];
        for (int l = 0; l < L; ++l) {   // sim[l] = kwd[l] . utt[l]^T  (cb_whisper.py:196, inputs normalised)
            ConvArgs a{};
            a.x = kwd + ((size_t)l * R + off_host[k0]) * D;
            a.w = uttP + (size_t)l * r.TuP * D;
            a.y = sims + (size_t)l * r.rmax * r.TuP;
            a.zero = h->zero.p;
            a.N = 1; a.H = 1; a.W = rows; a.Cin = D; a.Ho = 1; a.Wo = rows; a.Cout = r.TuP; a.KH = a.KW = 1;
            a.sh = a.sw = 1; a.M = rows; a.res_ld = a.y_ld = r.TuP; a.flags = CBW_EPI_OUT_F32;
            HIPCHK(cbw_conv_igemm(a, st));
        }
        HIPCHK(cbw_sim_resize(sims, r.rmax * r.TuP, r.TuP, off_dev, k0, kc, L, Tu, Ho, Wo, (uint16_t*)cws, st));
        CHK(resnet_chunk(h, plan, cws, kc, Ho, Wo, logits + (size_t)k0 * 2, st));
    }
    return CBW_OK;
}

// ---- the same spotter for a batch of segments (cb_whisper.py:87-129): pair p = b * K + k, chunks of pairs
namespace {
struct ResizedBatchWs {
    int TuP = 0;
    int64_t rmax = 0, sim_bytes = 0, chunk_bytes = 0;
};
// the row of pair p's first frame with every pair's frames laid one after another in pair order
int64_t pair_row(const int32_t* off_host, int K, int64_t p) {
    const int64_t b = p / K, k = p - b * K;
    return b * ((int64_t)off_host[K] - off_host[0]) + (off_host[k] - off_host[0]);
}
// the rows of the longest run (a keyword range of one utterance) of pairs [p0, p0 + pc)
int max_run_rows(const int32_t* off_host, int K, int64_t p0, int pc) {
    int best = 0;
    for (int64_t p = p0; p < p0 + pc;) {
        const int kf = (int)(p % K), kl = (int)std::min<int64_t>(K, kf + (p0 + pc - p));
        best = std::max(best, off_host[kl] - off_host[kf]);
        p += kl - kf;
    }
    return best;
}
int resized_batch_ws(const cbw_kws* h, const int32_t* off_host, int K, int B, int Tu, int D, int Ho, int Wo, int chunk,
                     ResizedBatchWs& r) {
    if (!off_host || K < 0 || B < 1 || Tu <= 0 || D <= 0 || Ho < 7 || Wo < 7 || chunk <= 0 ||
        (int64_t)B * K > INT32_MAX)
        return fail(CBW_ERR_INVALID, "bad arguments");
    for (int k = 0; k < K; ++k)
        if (off_host[k + 1] <= off_host[k]) return fail(CBW_ERR_INVALID, "every keyword needs >= 1 frame");
    const int64_t P = (int64_t)B * K;
    r.TuP = (Tu + 127) / 128 * 128;
    r.rmax = 0;
    for (int64_t p0 = 0; p0 < P; p0 += chunk) {   // the rows scratch: the largest pair chunk's
        const int64_t p1 = std::min<int64_t>(p0 + chunk, P);
        r.rmax = std::max(r.rmax, pair_row(off_host, K, p1) - pair_row(off_host, K, p0));
    }
    if (r.rmax > INT32_MAX) return fail(CBW_ERR_INVALID, "a chunk's similarity rows exceed 2^31: use a smaller chunk");
    r.sim_bytes = (int64_t)align_up((size_t)h->cfg.n_layers * std::max<int64_t>(r.rmax, 1) * r.TuP * 4);
    r.chunk_bytes = chunk_ws_bytes(h, Ho, Wo, chunk);
    return CBW_OK;
}
}  // namespace

int64_t cbw_kws_score_resized_batch_workspace_bytes(cbw_kws* h, const int32_t* off_host, int K, int B, int Tu, int D,
                                                    int Ho, int Wo, int chunk) {
    if (!h || !h->finalized) return -1;
    ResizedBatchWs r;
    if (resized_batch_ws(h, off_host, K, B, Tu, D, Ho, Wo, chunk, r) != CBW_OK) return -1;
    return r.sim_bytes + r.chunk_bytes;
}

int cbw_kws_score_resized_batch(cbw_kws* h, const uint16_t* utt, int B, int Tu, const uint16_t* kwd, int R, int D,
                                const int32_t* off_dev, const int32_t* off_host, int K, int Ho, int Wo, float* logits,
                                int chunk, void* ws, int64_t ws_bytes, cbw_stream_t stream) {
    if (!h || !utt || (K > 0 && (!kwd || !off_dev || !off_host || !logits))) return fail(CBW_ERR_INVALID, "null argument");
    if (!h->finalized) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called");
    if (h->cfg.variant != 0) return fail(CBW_ERR_INVALID, "the resized-similarity path takes raw hs (variant 0)");
    if (B < 1) return fail(CBW_ERR_INVALID, "B must be >= 1");
    if (K == 0) return CBW_OK;
    if (D % 64) return fail(CBW_ERR_INVALID, "D must be a multiple of 64");
    ResizedBatchWs r;
    CHK(resized_batch_ws(h, off_host, K, B, Tu, D, Ho, Wo, chunk, r));
    if (off_host[0] < 0 || off_host[K] > R) return fail(CBW_ERR_INVALID, "keyword rows out of range");
    if ((uintptr_t)utt % 16 || (uintptr_t)kwd % 16) return fail(CBW_ERR_INVALID, "utt and kwd must be 16-byte aligned");
    if (ws_bytes < r.sim_bytes + r.chunk_bytes) return fail(CBW_ERR_OOM, "workspace too small");
    if (!ws) return fail(CBW_ERR_INVALID, "null workspace");
    hipStream_t st = (hipStream_t)stream;
    const int L = h->cfg.n_layers;
    float* sims = (float*)ws;
    char* cws = (char*)ws + r.sim_bytes;
    const KwsPlan plan = kws_plan(h, Ho, Wo, chunk);
    const int64_t P = (int64_t)B * K;
    for (int64_t p0 = 0; p0 < P; p0 += chunk) {
        const int pc = (int)std::min<int64_t>(chunk, P - p0);
        const int64_t rows = pair_row(off_host, K, p0 + pc) - pair_row(off_host, K, p0);
        // sim[l] = kwd[l] . utt[b][l]^T for the chunk's runs (cb_whisper.py:196, inputs normalised), all layers at once
        HIPCHK(cbw_sim_rows_bf16(utt, kwd, off_dev, B, K, R, L, Tu, D, (int)p0, pc, max_run_rows(off_host, K, p0, pc),
                                 rows, r.TuP, sims, st));
        HIPCHK(cbw_sim_resize_batch(sims, r.TuP, off_dev, (int)p0, pc, K, R, rows, L, Tu, Ho, Wo, (uint16_t*)cws, st));
        CHK(resnet_chunk(h, plan, cws, pc, Ho, Wo, logits + (size_t)p0 * 2, st));
    }
    return CBW_OK;
}

int cbw_kws_sim_rows_bf16(const uint16_t* utt, int B, int Tu, const uint16_t* kwd, int R, int D, int L,
                          const int32_t* off_dev, int K, int p0, int pc, int ld, float* rows, cbw_stream_t stream) {
    if (!utt || !kwd || !off_dev || !rows) return fail(CBW_ERR_INVALID, "null argument");
    if (D <= 0 || D % 64) return fail(CBW_ERR_INVALID, "D must be a multiple of 64");
    if (Tu < 1 || R < 1 || L < 1 || L > 16 || K < 1 || B < 1 || (int64_t)B * K > INT32_MAX || p0 < 0 || pc < 1 ||
        (int64_t)p0 + pc > (int64_t)B * K || ld < Tu)
        return fail(CBW_ERR_INVALID, "bad sizes");
    if ((uintptr_t)utt % 16 || (uintptr_t)kwd % 16) return fail(CBW_ERR_INVALID, "utt and kwd must be 16-byte aligned");
    // without host offsets R bounds a run's rows and pc * R the chunk's
    HIPCHK(cbw_sim_rows_bf16(utt, kwd, off_dev, B, K, R, L, Tu, D, p0, pc, R, (int64_t)pc * R, ld, rows,
                             (hipStream_t)stream));
    return CBW_OK;
}

int cbw_kws_profile(cbw_kws* h, int max_launches) {
    if (!h || max_launches < 0) return fail(CBW_ERR_INVALID, "bad arguments");
    for (auto e : h->prof.ev) (void)hipEventDestroy(e);
    h->prof.ev.clear();
    h->prof.flop.assign(max_launches, 0.0);
    h->prof.tier.assign(max_launches, 0);
    h->prof.kern.assign(max_launches, "");
    h->prof.cur_tier = 0;
    h->prof.used = 0;
    h->prof.on = max_launches > 0;
    for (int i = 0; i < 2 * max_launches; ++i) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        h->prof.ev.push_back(e);
    }
    return CBW_OK;
}

int cbw_kws_profile_records(cbw_kws* h, double* start_ms, double* end_ms, double* flop, int max_records) {
    if (!h || max_records < 0 || (max_records > 0 && (!start_ms || !end_ms || !flop)))
        return fail(CBW_ERR_INVALID, "bad arguments");
    const int n = std::min(max_records, h->prof.used);
    for (int i = 0; i < n; ++i) {
        float a = 0.f, b = 0.f;
        HIPCHK(hipEventSynchronize(h->prof.ev[2 * i + 1]));
        HIPCHK(hipEventElapsedTime(&a, h->prof.ev[0], h->prof.ev[2 * i]));
        HIPCHK(hipEventElapsedTime(&b, h->prof.ev[0], h->prof.ev[2 * i + 1]));
        start_ms[i] = a;
        end_ms[i] = b;
        flop[i] = h->prof.flop[i];
    }
    return h->prof.used;
}

int cbw_kws_profile_tiers(cbw_kws* h, int32_t* tier, int max_records) {
    if (!h || max_records < 0 || (max_records > 0 && !tier)) return fail(CBW_ERR_INVALID, "bad arguments");
    const int n = std::min(max_records, h->prof.used);
    for (int i = 0; i < n; ++i) tier[i] = h->prof.tier[i];
    return h->prof.used;
}

int cbw_kws_profile_kernels(cbw_kws* h, const char** kernel, int max_records) {
    if (!h || max_records < 0 || (max_records > 0 && !kernel)) return fail(CBW_ERR_INVALID, "bad arguments");
    const int n = std::min(max_records, h->prof.used);
    for (int i = 0; i < n; ++i) kernel[i] = h->prof.kern[i];
    return h->prof.used;
}

int cbw_kws_profile_read(cbw_kws* h, double* ms, double* flop, int* n) {
    if (!h || !ms || !flop || !n) return fail(CBW_ERR_INVALID, "bad arguments");
    // busy time of the conv family = union of the launch intervals (chunks on two streams overlap)
    double f = 0.0;
    std::vector<std::pair<double, double>> iv;
    for (int i = 0; i < h->prof.used; ++i) {
        float a = 0.f, b = 0.f;
        HIPCHK(hipEventSynchronize(h->prof.ev[2 * i + 1]));
        HIPCHK(hipEventElapsedTime(&a, h->prof.ev[0], h->prof.ev[2 * i]));
        HIPCHK(hipEventElapsedTime(&b, h->prof.ev[0], h->prof.ev[2 * i + 1]));
        iv.emplace_back(a, b);
        f += h->prof.flop[i];
    }
    std::sort(iv.begin(), iv.end());
    double t = 0.0, cs = -1e300, ce = -1e300;
    for (const auto& p : iv) {
        if (p.first > ce) {
            if (ce > cs) t += ce - cs;
            cs = p.first;
            ce = p.second;
        } else {
            ce = std::max(ce, p.second);
        }
    }
    if (ce > cs) t += ce - cs;
    *ms = t;
    *flop = f;
    *n = h->prof.used;
    h->prof.used = 0;
    return CBW_OK;
}

// ------------------------------------------------------------------ fp32 re-scoring (kws_exact.hip)
namespace {
constexpr int EXACT_CHUNK = 32;
constexpr int RESCORE_THROTTLE = 8;   // passes per throttle event in rescore_impl (<= 16 passes, ~1 000 dispatches)

struct ExactPlan {
    size_t maps = 0, stem = 0, big = 0, small = 0;
};

// one pass of the re-scoring tiers: the stem's output kept in its own buffer
extern "C++" ExactPlan exact_plan(const cbw_kws* h, int Tk, int Tu, int n) {
    const NetPlan q = net_plan(h, Tk, Tu);
    const size_t N = (size_t)n;
    return {N * Tk * Tu * h->cfg.n_layers, N * q.stem, N * q.big, N * q.small};
}
}  // namespace

int64_t cbw_kws_project_f32_workspace_bytes(cbw_kws* h, int B, int T) {
    if (!h) return -1;
    const int L = h->cfg.n_layers, D = h->cfg.embedding_dim, U = h->cfg.proj_units;
    const size_t rows = (size_t)L * B * T;
    return (int64_t)(align_up(rows * D * 4) + align_up(rows * (D / 2) * 4) + align_up(rows * U * 4));
}

int cbw_kws_project_f32(cbw_kws* h, const float* x, const float* mask, int B, int T, float* out, float* mask_out,
                        void* ws, int64_t ws_bytes, cbw_stream_t stream) {
    if (!h || !x || !mask || !out || !mask_out) return fail(CBW_ERR_INVALID, "null argument");
    if (!h->finalized || h->stem32.cout == 0) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called (or no fp32 path)");
    if (B <= 0 || T <= 0) return fail(CBW_ERR_INVALID, "B and T must be positive");
    hipStream_t st = (hipStream_t)stream;
    const int L = h->cfg.n_layers, D = h->cfg.embedding_dim, U = h->cfg.proj_units;
    const float eps = 1e-6f;
    if (h->cfg.variant == 0) {
        HIPCHK(cbw_normalize_rows(x, 1, out, 1, 1, B * L, T, D, eps, 0, st));
        HIPCHK(hipMemcpyAsync(mask_out, mask, sizeof(float) * B * L * T, hipMemcpyDeviceToDevice, st));
        return CBW_OK;
    }
    if (ws_bytes < cbw_kws_project_f32_workspace_bytes(h, B, T)) return fail(CBW_ERR_OOM, "workspace too small");
    const size_t rows_l = (size_t)B * T;
    char* p = (char*)ws;
    float* xp = (float*)p; p += align_up(rows_l * L * D * 4);
    float* h1 = (float*)p; p += align_up(rows_l * L * (D / 2) * 4);
    float* h2 = (float*)p;
    HIPCHK(cbw_permute_lbtd_f32(x, xp, B, L, T, D, st));
    for (int l = 0; l < L; ++l) {
        CHK(launch_conv32(h->p1_32[l], xp + (size_t)l * rows_l * D, 1, 1, (int)rows_l, h1 + (size_t)l * rows_l * (D / 2),
                          nullptr, true, st));
        CHK(launch_conv32(h->p2_32[l], h1 + (size_t)l * rows_l * (D / 2), 1, 1, (int)rows_l, h2 + (size_t)l * rows_l * U,
                          nullptr, false, st));
    }
    if (h->cfg.variant == 1) {
        HIPCHK(cbw_normalize_rows(h2, 1, out, 1, L, B, T, U, eps, 1, st));
        HIPCHK(hipMemcpyAsync(mask_out, mask, sizeof(float) * B * L * T, hipMemcpyDeviceToDevice, st));
    } else {
        HIPCHK(cbw_lef_time_project(h2, h->tp_w.as<float>(), h->tp_b.as<float>(), out, 1, mask, mask_out, L, B, T, U,
                                    eps, st));
    }
    return CBW_OK;
}

int64_t cbw_kws_rescore_workspace_bytes(cbw_kws* h, int Tk, int Tu) {
    if (!h || !h->finalized || h->stem32.cout == 0) return -1;
    const ExactPlan p = exact_plan(h, Tk, Tu, EXACT_CHUNK);
    return (int64_t)(align_up(p.maps * 4) + align_up(p.stem * 4) + 3 * align_up(p.big * 4) + 2 * align_up(p.small * 4));
}

}  // extern "C"
namespace {
// channel sums of the fp32 network's conv inputs (cbw_kws_calibrate_bias): point 0 the maps, then per block
// 1 + 3 i its input, 2 + 3 i the first conv's output, 3 + 3 i the second's (bottleneck)
struct ConvInputStats {
    std::vector<int> ch;          // channels per point (0: unused)
    std::vector<size_t> off;      // float offset of point i's [G][C] partial sums in part
    std::vector<double> rows;     // rows summed per point
    DevBuf part;                  // the partial sums, zeroed on st by init()
    int G = 0;
    // absolute maxima (the fp8 tier's activation scales): per block i, point 4 i + {0 input, 1 first conv's
    // output, 2 second conv's output, 3 shortcut output}; amax[p * groups + g] = workgroup g's partial
    float* amax = nullptr;
    int init(const cbw_kws* h, hipStream_t st) {
        G = cbw_channel_sum_groups();
        ch = {h->cfg.n_layers};
        for (const BlockTopo& b : h->topo)
            ch.insert(ch.end(), {b.conv[0].cin, b.conv[0].cout, b.nconv == 3 ? b.conv[1].cout : 0});
        size_t tot = 0;
        for (int c : ch) { off.push_back(tot); tot += (size_t)G * c; }
        rows.assign(ch.size(), 0.0);
        CHK(part.alloc(tot * sizeof(float)));
        HIPCHK(hipMemsetAsync(part.p, 0, part.bytes, st));
        return CBW_OK;
    }
    // per point the channel means over the rows added (empty: nothing added); the stream's work must be complete
    int means(std::vector<std::vector<double>>& m) const {
        std::vector<float> host(part.bytes / sizeof(float));
        HIPCHK(hipMemcpy(host.data(), part.p, part.bytes, hipMemcpyDeviceToHost));
        m.assign(ch.size(), std::vector<double>());
        for (size_t i = 0; i < ch.size(); ++i) {
            if (!ch[i] || rows[i] <= 0) continue;
            m[i].assign(ch[i], 0.0);
            for (int g = 0; g < G; ++g)
                for (int c = 0; c < ch[i]; ++c) m[i][c] += host[off[i] + (size_t)g * ch[i] + c];
            for (double& v : m[i]) v /= rows[i];
        }
        return CBW_OK;
    }
    int add(size_t i, const float* x, int64_t M, hipStream_t st) {
        rows[i] += (double)M;
        HIPCHK(cbw_channel_sum_f32(x, M, ch[i], part.as<float>() + off[i], st));
        return CBW_OK;
    }
    int absmax(size_t p, const float* x, int64_t n, hipStream_t st) {
        if (!amax) return CBW_OK;
        HIPCHK(cbw_absmax_f32(x, n, amax + p * cbw_absmax_groups(), st));
        return CBW_OK;
    }
};

// The utterances and the pair list of a re-scoring call: utt f32 [B][L][Tu][E], and sel indexes the P pairs, which
// are the rows of logits; pair q = (pair_utt[q], pair_kwd[q]) (device int32 [P]) or, both null, q = b * K + k.  The
// per-utterance entry points are one_utterance(K): B = 1, no index arrays, pair q = keyword q.
struct RescorePairs {
    int B;
    const int32_t *pair_utt, *pair_kwd;
    int P;
    bool single() const { return B == 1 && !pair_utt; }
};
RescorePairs one_utterance(int K) { return {1, nullptr, nullptr, K}; }

// the argument checks of cbw_kws_rescore_pairs / cbw_kws_rescore_x3_pairs
int check_rescore_pairs(const RescorePairs& pr, int K, int n_sel) {
    if (pr.B < 1 || pr.P < 0 || K < 0) return fail(CBW_ERR_INVALID, "bad B/K/P");
    if (n_sel > pr.P) return fail(CBW_ERR_INVALID, "n_sel exceeds the P pairs sel indexes");
    if (pr.P == 0) return CBW_OK;   // an empty pair list needs no index arrays (then n_sel <= 0: nothing is launched)
    if (K < 1) return fail(CBW_ERR_INVALID, "pairs given but no keywords");
    if ((pr.pair_utt == nullptr) != (pr.pair_kwd == nullptr))
        return fail(CBW_ERR_INVALID, "pair_utt and pair_kwd must both be given or both be null");
    if (!pr.pair_utt && (int64_t)pr.P != (int64_t)pr.B * K)
        return fail(CBW_ERR_INVALID, "without index arrays P must be B * K (every utterance against every keyword)");
    return CBW_OK;
}

// the fp32 similarity maps of pairs sel[c0 .. c0 + cn) of a pass: the per-utterance kernels for one utterance (their
// launches are what they were), the pair kernels otherwise
int sim_f32_pass(const cbw_kws* h, const float* utt, const float* utt_mask, const float* kwd, const float* kwd_mask,
                 int K, const RescorePairs& pr, const int32_t* sel, int c0, int cn, float* maps, int Tk, int Tu,
                 hipStream_t st) {
    const int L = h->cfg.n_layers;
    const int E = h->cfg.variant == 0 ? h->cfg.embedding_dim : h->cfg.proj_units;
    if (pr.single())
        HIPCHK(cbw_sim_f32(kwd, kwd_mask, utt, utt_mask, sel, c0, cn, maps, L, Tk, Tu, E, st));
    else
        HIPCHK(cbw_sim_f32_pairs(kwd, kwd_mask, K, utt, utt_mask, pr.B, pr.pair_utt, pr.pair_kwd, pr.P, sel, c0, cn, maps,
                                 L, Tk, Tu, E, st));
    return CBW_OK;
}

// the fp32 re-scoring network over the n_sel > 0 selected maps of [Tk][Tu] pixels, in passes of EXACT_CHUNK;
// fill(c0, cn, maps) writes the fp32 NHWC maps [cn][Tk][Tu][L] of sel[c0 .. c0 + cn) (sim_f32_pass for the
// efficient_kws spotter, the similarity rows + resize for CB-Whisper's own); ws holds cbw_kws_rescore_workspace_bytes;
// logits null: no classifier (statistics only)
template <class Fill>
int rescore_passes(cbw_kws* h, int Tk, int Tu, const int32_t* sel, int n_sel, float* logits, void* ws, hipStream_t st,
                   ConvInputStats* stats, Fill&& fill) {
    const ExactPlan plan = exact_plan(h, Tk, Tu, EXACT_CHUNK);
    char* p = (char*)ws;
    float* maps = (float*)p; p += align_up(plan.maps * 4);
    float* stem = (float*)p; p += align_up(plan.stem * 4);
    float* X = (float*)p; p += align_up(plan.big * 4);
    float* Y = (float*)p; p += align_up(plan.big * 4);
    float* SC = (float*)p; p += align_up(plan.big * 4);
    float* T1 = (float*)p; p += align_up(plan.small * 4);
    float* T2 = (float*)p;
    // a call over all 10 000 pairs enqueues ~19 000 dispatches (313 passes x ~60 launches); under rocprofv3
    // --pmc such a call faulted inside hipLaunchKernel (profiles/r05b_pmc_f32_one_call_sigsegv.log.txt) while the same
    // passes in host-synchronised calls of 512 pairs (~1 000 dispatches each) ran clean.  So one call keeps at most
    // 2 x RESCORE_THROTTLE passes in flight: every RESCORE_THROTTLE passes it records an event and waits on the host
    // for the previous one.  Not while the stream is being captured (the call stays graph-capturable); results
    // unchanged.  Round 6: with 128 passes (~7 700 dispatches) in flight the one-call audit under --pmc still failed
    // (unspecified launch failure, 3 956 dispatches incomplete: profiles/r06b_pmc_f32_one_call_throttle128.log.txt),
    // so the bound is the r05b passes' ~1 000 dispatches.  The pairs form (cbw_kws_rescore_pairs) runs the same passes
    // over its selected pairs, whatever their utterances: the throttle applies to it unchanged.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(st, &cap));
    const bool throttle = cap == hipStreamCaptureStatusNone && n_sel > RESCORE_THROTTLE * EXACT_CHUNK;
    if (throttle)
        for (auto& e : h->throttle_ev)
            if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    int pass = 0;
    for (int c0 = 0; c0 < n_sel; c0 += EXACT_CHUNK, ++pass) {
        const int cn = std::min(EXACT_CHUNK, n_sel - c0);
        if (throttle && pass > 0 && pass % RESCORE_THROTTLE == 0) {
            const int k = (pass / RESCORE_THROTTLE) & 1;
            if (pass >= 2 * RESCORE_THROTTLE) HIPCHK(hipEventSynchronize(h->throttle_ev[k]));
            HIPCHK(hipEventRecord(h->throttle_ev[k], st));
        }
        CHK(fill(c0, cn, maps));
        if (stats) CHK(stats->add(0, maps, (int64_t)cn * Tk * Tu, st));
        const int Hs = out_dim(Tk, 7, 2), Ws = out_dim(Tu, 7, 2);
        CHK(launch_conv32(h->stem32, maps, cn, Tk, Tu, stem, nullptr, true, st));
        int H = out_dim(Hs, 3, 2), W = out_dim(Ws, 3, 2), C = 64;
        HIPCHK(cbw_maxpool_f32(stem, X, cn, Hs, Ws, 64, H, W, st));
        float *x = X, *y = Y;
        for (size_t bi = 0; bi < h->blocks32.size(); ++bi) {
            const auto& b = h->blocks32[bi];
            const BlockDims d = block_dims(h->topo[bi], H, W);
            const int h1 = d.h1, w1 = d.w1, Ho = d.Ho, Wo = d.Wo;
            const float* res = x;
            if (stats) CHK(stats->add(1 + 3 * bi, x, (int64_t)cn * H * W, st));
            if (stats) CHK(stats->absmax(4 * bi, x, (int64_t)cn * H * W * C, st));
            if (b.has_sc) {
                CHK(launch_conv32(b.sc, x, cn, H, W, SC, nullptr, false, st));
                res = SC;
                if (stats) CHK(stats->absmax(4 * bi + 3, SC, (int64_t)cn * d.hs * d.ws * b.sc.cout, st));
            }
            if (b.nconv == 3) {
                CHK(launch_conv32(b.conv[0], x, cn, H, W, T1, nullptr, true, st));
                if (stats) CHK(stats->add(2 + 3 * bi, T1, (int64_t)cn * h1 * w1, st));
                if (stats) CHK(stats->absmax(4 * bi + 1, T1, (int64_t)cn * h1 * w1 * b.conv[0].cout, st));
                CHK(launch_conv32(b.conv[1], T1, cn, h1, w1, T2, nullptr, true, st));
                if (stats) CHK(stats->add(3 + 3 * bi, T2, (int64_t)cn * Ho * Wo, st));
                if (stats) CHK(stats->absmax(4 * bi + 2, T2, (int64_t)cn * Ho * Wo * b.conv[1].cout, st));
                CHK(launch_conv32(b.conv[2], T2, cn, Ho, Wo, y, res, true, st));
            } else {
                CHK(launch_conv32(b.conv[0], x, cn, H, W, T1, nullptr, true, st));
                if (stats) CHK(stats->add(2 + 3 * bi, T1, (int64_t)cn * Ho * Wo, st));
                CHK(launch_conv32(b.conv[1], T1, cn, Ho, Wo, y, res, true, st));
            }
            std::swap(x, y);
            H = Ho;
            W = Wo;
            C = b.conv[b.nconv - 1].cout;
        }
        if (logits)
            HIPCHK(cbw_pool_fc_f32(x, h->fc_w.as<float>(), h->fc_b.as<float>(), sel, c0, cn, logits, H * W, C, st));
    }
    return CBW_OK;
}

// the efficient_kws spotter's fp32 tier (cbw_kws_rescore, cbw_kws_rescore_pairs, the calibrations)
int rescore_impl(cbw_kws* h, const float* utt, const float* utt_mask, const float* kwd, const float* kwd_mask, int K,
                 const RescorePairs& pr, int Tk, int Tu, const int32_t* sel, int n_sel, float* logits, void* ws,
                 int64_t ws_bytes, hipStream_t st, ConvInputStats* stats) {
    if (!h->finalized || h->stem32.cout == 0) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called (or no fp32 path)");
    if (K < 0 || n_sel < 0 || n_sel > pr.P || Tk <= 0 || Tu <= 0) return fail(CBW_ERR_INVALID, "bad sizes");
    if (n_sel == 0) return CBW_OK;
    if (ws_bytes < cbw_kws_rescore_workspace_bytes(h, Tk, Tu)) return fail(CBW_ERR_OOM, "workspace too small");
    return rescore_passes(h, Tk, Tu, sel, n_sel, logits, ws, st, stats, [&](int c0, int cn, float* maps) {
        return sim_f32_pass(h, utt, utt_mask, kwd, kwd_mask, K, pr, sel, c0, cn, maps, Tk, Tu, st);
    });
}

// the folded fp32 bias of a conv plus, with input channel means m, the bias correction
// sum_{kh, kw, c} m[c] (w - bf16(w)): the mean shift the bf16 weights put on each output channel
int corrected_bias(const ParamStore& ps, const std::string& prefix, const ConvShape& shape, const double* m,
                   std::vector<double>& b) {
    const int cin = shape.cin, cout = shape.cout;
    std::vector<float> w, sh;
    CHK(fold_conv_host(ps, prefix, cin, cout, shape.k, w, sh));
    b.assign(sh.begin(), sh.end());
    if (!m) return CBW_OK;
    const size_t taps = (size_t)shape.k * shape.k;
    for (int o = 0; o < cout; ++o) {
        double s = 0.0;
        for (size_t t = 0; t < taps; ++t) {
            const float* row = &w[((size_t)o * taps + t) * cin];
            for (int c = 0; c < cin; ++c) s += m[c] * ((double)row[c] - (double)bf16_round_host(row[c]));
        }
        b[o] += s;
    }
    return CBW_OK;
}

// rewrite a bias vector in place (same allocation: captured graphs and in-flight plans keep their pointers)
int overwrite_bias(DevBuf& d, const std::vector<double>& v) {
    if (d.bytes != v.size() * sizeof(float)) return fail(CBW_ERR_STATE, "bias size mismatch");
    const std::vector<float> f(v.begin(), v.end());
    HIPCHK(hipMemcpy(d.p, f.data(), d.bytes, hipMemcpyHostToDevice));
    return CBW_OK;
}

// the bf16 scoring network's biases from the parameters, corrected with the conv-input means m (ConvInputStats
// points) or, m null, as folded (cbw_kws_finalize's values)
int apply_bias_correction(cbw_kws* h, const std::vector<std::vector<double>>* m) {
    // the folded biases are read by scoring launches on any stream: drain the device before rewriting them
    HIPCHK(hipDeviceSynchronize());
    auto mean = [&](size_t i) -> const double* { return m && !(*m)[i].empty() ? (*m)[i].data() : nullptr; };
    std::vector<double> b, b2;
    CHK(corrected_bias(h->ps, "model.feature_extractor.embedder.embedder", stem_shape(h->cfg.n_layers), mean(0), b));
    CHK(overwrite_bias(h->stem_b, b));
    for (size_t bi = 0; bi < h->blocks.size(); ++bi) {
        BlockW& blk = h->blocks[bi];
        const BlockTopo& t = h->topo[bi];
        const double* in[3] = {mean(1 + 3 * bi), mean(2 + 3 * bi), mean(3 + 3 * bi)};
        if (blk.has_sc && !blk.fused_sc) {
            CHK(corrected_bias(h->ps, t.prefix + ".shortcut", t.sc, in[0], b));
            CHK(overwrite_bias(blk.sc.b, b));
        }
        for (int j = 0; j < t.nconv; ++j) {
            CHK(corrected_bias(h->ps, t.prefix + ".layer." + std::to_string(j), t.conv[j], in[j], b));
            if (j == 2 && blk.fused_sc) {   // + the shortcut's bias and correction (K-concatenated conv)
                CHK(corrected_bias(h->ps, t.prefix + ".shortcut", t.sc, in[0], b2));
                for (size_t o = 0; o < b.size(); ++o) b[o] += b2[o];
            }
            CHK(overwrite_bias(blk.conv[j].b, b));
        }
    }
    return CBW_OK;
}
}  // namespace
extern "C" {

int cbw_kws_rescore(cbw_kws* h, const float* utt, const float* utt_mask, const float* kwd, const float* kwd_mask, int K,
                    int Tk, int Tu, const int32_t* sel, int n_sel, float* logits, void* ws, int64_t ws_bytes,
                    cbw_stream_t stream) {
    if (!h || !utt || !utt_mask || !kwd || !kwd_mask || !logits || (n_sel > 0 && !sel))
        return fail(CBW_ERR_INVALID, "null argument");
    return rescore_impl(h, utt, utt_mask, kwd, kwd_mask, K, one_utterance(K), Tk, Tu, sel, n_sel, logits, ws, ws_bytes,
                        (hipStream_t)stream, nullptr);
}

int cbw_kws_rescore_pairs(cbw_kws* h, const float* utt, const float* utt_mask, int B, const float* kwd,
                          const float* kwd_mask, int K, int Tk, int Tu, const int32_t* pair_utt, const int32_t* pair_kwd,
                          int P, const int32_t* sel, int n_sel, float* logits, void* ws, int64_t ws_bytes,
                          cbw_stream_t stream) {
    if (!h) return fail(CBW_ERR_INVALID, "null handle");
    const RescorePairs pr{B, pair_utt, pair_kwd, P};
    CHK(check_rescore_pairs(pr, K, n_sel));
    if (n_sel > 0 && (!utt || !utt_mask || !kwd || !kwd_mask || !logits || !sel))
        return fail(CBW_ERR_INVALID, "null argument");
    return rescore_impl(h, utt, utt_mask, kwd, kwd_mask, K, pr, Tk, Tu, sel, n_sel, logits, ws, ws_bytes,
                        (hipStream_t)stream, nullptr);
}

int cbw_kws_set_score_offset(cbw_kws* h, const float* offset) {
    if (!h || !offset) return fail(CBW_ERR_INVALID, "null argument");
    if (!h->finalized || h->fc_b16.bytes != 2 * sizeof(float)) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called");
    int rc;
    const auto* fb = h->ps.get("model.classifier.1.bias", 2, &rc);
    if (!fb) return rc;
    const float b[2] = {(*fb)[0] + offset[0], (*fb)[1] + offset[1]};
    // the bias is read by scoring launches on any stream: drain the device before overwriting it in place
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h->fc_b16.p, b, sizeof(b), hipMemcpyHostToDevice));
    return CBW_OK;
}

int cbw_kws_calibrate_bias(cbw_kws* h, const float* utt, const float* utt_mask, const float* kwd, const float* kwd_mask,
                           int K, int Tk, int Tu, const int32_t* sel, int n_sel, void* ws, int64_t ws_bytes,
                           cbw_stream_t stream) {
    if (!h) return fail(CBW_ERR_INVALID, "null handle");
    if (!h->finalized || h->stem32.cout == 0) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called (or no fp32 path)");
    hipStream_t st = (hipStream_t)stream;
    if (n_sel == 0) {   // back to the folded biases (and no logit offset)
        HIPCHK(hipDeviceSynchronize());
        const float zero2[2] = {0.f, 0.f};
        CHK(cbw_kws_set_score_offset(h, zero2));
        return apply_bias_correction(h, nullptr);
    }
    if (!utt || !utt_mask || !kwd || !kwd_mask || !sel) return fail(CBW_ERR_INVALID, "null argument");
    ConvInputStats s;
    CHK(s.init(h, st));
    CHK(rescore_impl(h, utt, utt_mask, kwd, kwd_mask, K, one_utterance(K), Tk, Tu, sel, n_sel, nullptr, ws, ws_bytes, st,
                     &s));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<std::vector<double>> m;
    CHK(s.means(m));
    return apply_bias_correction(h, &m);
}

int cbw_kws_calibrate_fp8(cbw_kws* h, const float* utt, const float* utt_mask, const float* kwd, const float* kwd_mask,
                          int K, int Tk, int Tu, const int32_t* sel, int n_sel, float margin, void* ws, int64_t ws_bytes,
                          cbw_stream_t stream) {
    if (!h || !utt || !utt_mask || !kwd || !kwd_mask || !sel || n_sel <= 0) return fail(CBW_ERR_INVALID, "null argument");
    if (!h->finalized || h->stem32.cout == 0) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called (or no fp32 path)");
    if (h->cfg.resnet_depth != 50) return fail(CBW_ERR_INVALID, "the fp8 tier covers ResNet-50 (bottleneck stages 2-4)");
    if (!(margin > 0.f)) return fail(CBW_ERR_INVALID, "margin must be positive");
    hipStream_t st = (hipStream_t)stream;
    const size_t nb = h->topo.size();
    const char* bc = getenv("CBW_FP8_BIAS_CORR");   // 0: the folded biases (A/B)
    const bool bias_corr = !(bc && atoi(bc) == 0);
    const int G = cbw_absmax_groups();
    DevBuf amax;
    CHK(amax.alloc(nb * 4 * G * sizeof(float)));
    HIPCHK(hipMemsetAsync(amax.p, 0, nb * 4 * G * sizeof(float), st));
    ConvInputStats s;
    s.amax = amax.as<float>();
    // + the conv inputs' channel sums (the bias correction of the e4m3 weights), points as cbw_kws_calibrate_bias
    CHK(s.init(h, st));
    CHK(rescore_impl(h, utt, utt_mask, kwd, kwd_mask, K, one_utterance(K), Tk, Tu, sel, n_sel, nullptr, ws, ws_bytes, st,
                     &s));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<float> host(nb * 4 * G);
    HIPCHK(hipMemcpy(host.data(), amax.p, host.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<std::vector<double>> mean;
    CHK(s.means(mean));
    auto mp = [&](size_t i) -> const double* { return bias_corr && !mean[i].empty() ? mean[i].data() : nullptr; };
    auto scale = [&](size_t p) {
        float m = 0.f;
        for (int g = 0; g < G; ++g) m = std::max(m, host[p * G + g]);
        return m > 0.f ? m * margin / 448.f : 1.f;
    };
    int first = -1;
    for (size_t i = 0; i < nb; ++i)
        if (h->topo[i].stage >= 2) { first = (int)i; break; }
    if (first < 0) return fail(CBW_ERR_STATE, "no stage-2 blocks");
    std::vector<BlockF8> b8(nb - first);
    for (size_t i = first; i < nb; ++i) {
        const BlockTopo& b = h->topo[i];
        BlockF8& q = b8[i - first];
        if (b.nconv != 3) return fail(CBW_ERR_INVALID, "bottleneck blocks only");
        const std::string& p = b.prefix;
        q.s_x = scale(4 * i); q.s_t1 = scale(4 * i + 1); q.s_t2 = scale(4 * i + 2);
        q.has_sc = b.has_sc;
        if (b.has_sc) {
            q.s_sc = scale(4 * i + 3);
            CHK(load_conv_f8(h->ps, p + ".shortcut", b.sc, false, q.s_x, q.sc, mp(1 + 3 * i)));
        }
        const float s_in[3] = {q.s_x, q.s_t1, q.s_t2};   // each conv's input scale; the third's ReLU follows the sum
        for (int j = 0; j < 3; ++j)
            CHK(load_conv_f8(h->ps, p + ".layer." + std::to_string(j), b.conv[j], true, s_in[j], q.conv[j],
                             mp(1 + j + 3 * i)));
        q.out_bf16 = i + 1 == nb;
        q.s_out = q.out_bf16 ? 1.f : scale(4 * (i + 1));
    }
    HIPCHK(hipDeviceSynchronize());   // setup-time: no scoring may be in flight on any stream while the tier changes
    h->blocks8 = std::move(b8);
    h->f8_first = first;
    h->f8_in_scale = h->blocks8[0].s_x;
    return CBW_OK;
}

int x3_stem32() {   // CBW_X3_STEM32=1: the compensated tier's stem in fp32 (conv_f32 + max-pool + split)
    const char* e = getenv("CBW_X3_STEM32");
    return e ? atoi(e) : 0;
}

// pairs per compensated-tier pass (CBW_X3_CHUNK overrides; read once per process).  bench.py, 855 band pairs
// per clip: 128 -> 58.4 ms, 256 -> 55.8, 512 -> 51.9, 1024 -> 51.2 (workspace ~21 MB per pair at LEF maps)
int x3_chunk() {
    static const int c = [] {
        const char* e = getenv("CBW_X3_CHUNK");
        const int v = e ? atoi(e) : 512;
        return v > 0 ? v : 512;
    }();
    return c;
}

// the compensated tier's workspace for passes of `chunk` maps
static int64_t x3_ws_bytes(const cbw_kws* h, int Tk, int Tu, int chunk) {
    const ExactPlan p = exact_plan(h, Tk, Tu, chunk);
    return (int64_t)(align_up(p.maps * 4) + align_up(p.stem * 4) + 2 * align_up(p.big * 4) + 2 * align_up(p.big * 4) +
                     2 * align_up(p.small * 4));
}

int64_t cbw_kws_rescore_x3_workspace_bytes(cbw_kws* h, int Tk, int Tu) {
    if (!h || !h->finalized || h->stem32.cout == 0 || h->blocks3.empty() || Tk <= 0 || Tu <= 0) return -1;
    return x3_ws_bytes(h, Tk, Tu, x3_chunk());
}

// the compensated re-scoring network over the n_sel > 0 selected maps in passes of X3_CHUNK; fill as rescore_passes
// takes it; ws holds x3_ws_bytes(h, Tk, Tu, X3_CHUNK)
extern "C++" {
template <class Fill>
int rescore_x3_passes(cbw_kws* h, int Tk, int Tu, int X3_CHUNK, const int32_t* sel, int n_sel, float* logits, void* ws,
                      hipStream_t st, Fill&& fill) {
    const int L = h->cfg.n_layers;
    const ExactPlan plan = exact_plan(h, Tk, Tu, X3_CHUNK);
    char* p = (char*)ws;
    float* maps = (float*)p; p += align_up(plan.maps * 4);
    float* stem = (float*)p; p += align_up(plan.stem * 4);
    float* X32 = (float*)p; p += align_up(plan.big * 4);     // stem/max-pool output, then the network output
    float* SC32 = (float*)p; p += align_up(plan.big * 4);    // projection shortcuts
    uint16_t* X3 = (uint16_t*)p; p += align_up(plan.big * 4);   // [hi | lo] activations, 4 bytes per element
    uint16_t* Y3 = (uint16_t*)p; p += align_up(plan.big * 4);
    uint16_t* T1 = (uint16_t*)p; p += align_up(plan.small * 4);
    uint16_t* T2 = (uint16_t*)p;
    const void* zp = h->zero.p;
    const size_t nb = h->blocks3.size();
    for (int c0 = 0; c0 < n_sel; c0 += X3_CHUNK) {
        const int cn = std::min(X3_CHUNK, n_sel - c0);
        // similarity maps in fp32, then the stem + max-pool: compensated bf16 in one pass (maps split into
        // [hi | hi | lo] channels of an NHWC16 image, cbw_stem16_pool_x3; CBW_X3_STEM32=1 or 3 L > 16: the fp32
        // stem, max-pool and split)
        CHK(fill(c0, cn, maps));
        const int Hs = out_dim(Tk, 7, 2), Ws = out_dim(Tu, 7, 2);
        int H = out_dim(Hs, 3, 2), W = out_dim(Ws, 3, 2), C = 64;
        if (h->stem16x3_w.p && !x3_stem32()) {
            uint16_t* m16 = (uint16_t*)stem;   // [cn][Tk][Tu][16] bf16 fits the fp32 stem buffer
            HIPCHK(cbw_maps_split16(maps, m16, cn, L, Tk, Tu, st));
            HIPCHK(cbw_stem16_pool_x3(m16, h->stem16x3_w.as<uint16_t>(), h->stem32.b.as<float>(), X3, cn, Tk, Tu, Hs,
                                      Ws, H, W, st));
        } else {
            CHK(launch_conv32(h->stem32, maps, cn, Tk, Tu, stem, nullptr, true, st));
            HIPCHK(cbw_maxpool_f32(stem, X32, cn, Hs, Ws, 64, H, W, st));
            HIPCHK(cbw_split3(X32, X3, (int64_t)cn * H * W, 64, st));
        }
        uint16_t *x3 = X3, *y3 = Y3;
        for (size_t bi = 0; bi < nb; ++bi) {
            const auto& b = h->blocks3[bi];
            const BlockDims d = block_dims(h->topo[bi], H, W);
            const int Ho = d.Ho, Wo = d.Wo;
            const void* res = x3;   // identity shortcut: the block input's [hi | lo]
            bool res_split = true;
            if (b.has_sc) {
                CHK(launch_conv_x3(b.sc, x3, cn, H, W, SC32, nullptr, nullptr, false, CBW_EPI_OUT_F32, zp, st,
                                   &h->prof));
                res = SC32;
                res_split = false;
            }
            float* out32 = bi + 1 == nb ? X32 : nullptr;   // fp32 network output for the pool + classifier
            if (b.nconv == 3) {
                CHK(launch_conv_x3(b.conv[0], x3, cn, H, W, T1, nullptr, nullptr, false, CBW_EPI_SPLIT3, zp, st,
                                   &h->prof));
                CHK(launch_conv_x3(b.conv[1], T1, cn, d.h1, d.w1, T2, nullptr, nullptr, false, CBW_EPI_SPLIT3, zp, st,
                                   &h->prof));
                CHK(launch_conv_x3(b.conv[2], T2, cn, Ho, Wo, y3, out32, res, res_split, CBW_EPI_SPLIT3, zp, st,
                                   &h->prof));
            } else {
                CHK(launch_conv_x3(b.conv[0], x3, cn, H, W, T1, nullptr, nullptr, false, CBW_EPI_SPLIT3, zp, st,
                                   &h->prof));
                CHK(launch_conv_x3(b.conv[1], T1, cn, Ho, Wo, y3, out32, res, res_split, CBW_EPI_SPLIT3, zp, st,
                                   &h->prof));
            }
            std::swap(x3, y3);
            H = Ho;
            W = Wo;
            C = b.conv[b.nconv - 1].cout;
        }
        HIPCHK(cbw_pool_fc_f32(X32, h->fc_w.as<float>(), h->fc_b.as<float>(), sel, c0, cn, logits, H * W, C, st));
    }
    return CBW_OK;
}
}  // extern "C++"

// the efficient_kws spotter's compensated tier (cbw_kws_rescore_x3, cbw_kws_rescore_x3_pairs)
static int rescore_x3_impl(cbw_kws* h, const float* utt, const float* utt_mask, const float* kwd, const float* kwd_mask,
                           int K, const RescorePairs& pr, int Tk, int Tu, const int32_t* sel, int n_sel, float* logits,
                           void* ws, int64_t ws_bytes, hipStream_t st) {
    if (!h->finalized || h->stem32.cout == 0 || h->blocks3.empty())
        return fail(CBW_ERR_STATE, "cbw_kws_finalize not called (or no re-scoring path)");
    if (K < 0 || n_sel < 0 || n_sel > pr.P || Tk <= 0 || Tu <= 0) return fail(CBW_ERR_INVALID, "bad sizes");
    if (n_sel == 0) return CBW_OK;
    if (ws_bytes < cbw_kws_rescore_x3_workspace_bytes(h, Tk, Tu)) return fail(CBW_ERR_OOM, "workspace too small");
    return rescore_x3_passes(h, Tk, Tu, x3_chunk(), sel, n_sel, logits, ws, st, [&](int c0, int cn, float* maps) {
        return sim_f32_pass(h, utt, utt_mask, kwd, kwd_mask, K, pr, sel, c0, cn, maps, Tk, Tu, st);
    });
}

int cbw_kws_rescore_x3(cbw_kws* h, const float* utt, const float* utt_mask, const float* kwd, const float* kwd_mask,
                       int K, int Tk, int Tu, const int32_t* sel, int n_sel, float* logits, void* ws, int64_t ws_bytes,
                       cbw_stream_t stream) {
    if (!h || !utt || !utt_mask || !kwd || !kwd_mask || !logits || (n_sel > 0 && !sel))
        return fail(CBW_ERR_INVALID, "null argument");
    return rescore_x3_impl(h, utt, utt_mask, kwd, kwd_mask, K, one_utterance(K), Tk, Tu, sel, n_sel, logits, ws, ws_bytes,
                           (hipStream_t)stream);
}

int cbw_kws_rescore_x3_pairs(cbw_kws* h, const float* utt, const float* utt_mask, int B, const float* kwd,
                             const float* kwd_mask, int K, int Tk, int Tu, const int32_t* pair_utt,
                             const int32_t* pair_kwd, int P, const int32_t* sel, int n_sel, float* logits, void* ws,
                             int64_t ws_bytes, cbw_stream_t stream) {
    if (!h) return fail(CBW_ERR_INVALID, "null handle");
    const RescorePairs pr{B, pair_utt, pair_kwd, P};
    CHK(check_rescore_pairs(pr, K, n_sel));
    if (n_sel > 0 && (!utt || !utt_mask || !kwd || !kwd_mask || !logits || !sel))
        return fail(CBW_ERR_INVALID, "null argument");
    return rescore_x3_impl(h, utt, utt_mask, kwd, kwd_mask, K, pr, Tk, Tu, sel, n_sel, logits, ws, ws_bytes,
                           (hipStream_t)stream);
}

// ---- CB-Whisper's own spotter (cb_whisper.py:110-128): the exact tiers over the resized maps
int cbw_kws_build_exact(cbw_kws* h) {
    if (!h) return fail(CBW_ERR_INVALID, "null handle");
    if (!h->finalized) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called");
    if (h->stem32.cout != 0 && !h->blocks3.empty()) return CBW_OK;   // cbw_kws_finalize (n_layers <= 4) or an earlier call
    if (h->cfg.variant != 0) return fail(CBW_ERR_INVALID, "a projector's fp32 copy is built by cbw_kws_finalize");
    HIPCHK(hipDeviceSynchronize());   // setup-time: no scoring may be in flight on any stream while the tiers appear
    const int rc = build_f32(h);
    if (rc != CBW_OK) {   // all or nothing: a half-built network must not pass for one
        h->stem32 = ConvW{};
        h->blocks32.clear();
        h->blocks3.clear();
        return rc;
    }
    HIPCHK(hipDeviceSynchronize());
    return CBW_OK;
}

// pairs per compensated pass over resized maps: x3_chunk()'s 512 is sized for the efficient_kws maps (~21 MB of
// workspace per pair); a (150, 750) map of 12 channels takes ~50 MB and up to ~14 MB of similarity rows, so 512 of them
// would ask for ~32 GB.  64 keeps a pass near 4 GB, and its convs (M = 64 x 38 x 188 pixels and up) still fill the GPU.
constexpr int RESIZED_X3_CHUNK = 64;
static int resized_x3_chunk() { return std::min(x3_chunk(), RESIZED_X3_CHUNK); }

struct ResizedExact {
    int tk_max = 0, ld = 0;
    int64_t rows_bytes = 0;   // one pass's similarity rows, f32 [chunk][L][tk_max][ld]
};

// the argument checks the two resized tiers share (cbw_kws_score_resized's, for fp32 rows) and the rows scratch
static int resized_exact_args(const cbw_kws* h, const int32_t* off_host, int K, int Tu, int R, int D, int Ho, int Wo,
                              int chunk, ResizedExact& r) {
    if (h->cfg.variant != 0) return fail(CBW_ERR_INVALID, "the resized-similarity path takes raw hs (variant 0)");
    if (D <= 0 || D % 16) return fail(CBW_ERR_INVALID, "D must be a multiple of 16");
    if (!off_host || K < 0 || Tu <= 0 || R < 0) return fail(CBW_ERR_INVALID, "bad arguments");
    if (off_host[0] < 0 || off_host[K] > R) return fail(CBW_ERR_INVALID, "keyword rows out of range");
    r.tk_max = 0;
    for (int k = 0; k < K; ++k) {
        if (off_host[k + 1] <= off_host[k]) return fail(CBW_ERR_INVALID, "every keyword needs >= 1 frame");
        r.tk_max = std::max(r.tk_max, off_host[k + 1] - off_host[k]);
    }
    if (Ho < 7 || Wo < 7) return fail(CBW_ERR_INVALID, "Ho and Wo must be >= 7 (the stem's kernel)");
    r.ld = (Tu + 63) / 64 * 64;
    r.rows_bytes = (int64_t)align_up((size_t)chunk * h->cfg.n_layers * std::max(r.tk_max, 1) * r.ld * 4);
    return CBW_OK;
}

static int64_t resized_exact_ws(cbw_kws* h, const int32_t* off_host, int K, int Tu, int D, int Ho, int Wo, bool x3) {
    if (!h || !h->finalized || h->stem32.cout == 0 || h->blocks3.empty() || !off_host || K < 0) return -1;
    ResizedExact r;
    const int chunk = x3 ? resized_x3_chunk() : EXACT_CHUNK;
    if (resized_exact_args(h, off_host, K, Tu, off_host[K], D, Ho, Wo, chunk, r) != CBW_OK) return -1;
    return r.rows_bytes + (x3 ? x3_ws_bytes(h, Ho, Wo, chunk) : cbw_kws_rescore_workspace_bytes(h, Ho, Wo));
}

int64_t cbw_kws_rescore_resized_workspace_bytes(cbw_kws* h, const int32_t* off_host, int K, int Tu, int D, int Ho,
                                                int Wo) {
    return resized_exact_ws(h, off_host, K, Tu, D, Ho, Wo, false);
}

int64_t cbw_kws_rescore_resized_x3_workspace_bytes(cbw_kws* h, const int32_t* off_host, int K, int Tu, int D, int Ho,
                                                   int Wo) {
    return resized_exact_ws(h, off_host, K, Tu, D, Ho, Wo, true);
}

// B = 1 with batch false: the per-utterance entry points, sel = keywords; batch: sel indexes the B * K pairs b * K + k
static int rescore_resized_impl(cbw_kws* h, const float* utt, int B, bool batch, int Tu, const float* kwd, int R, int D,
                                const int32_t* off_dev, const int32_t* off_host, int K, int Ho, int Wo,
                                const int32_t* sel, int n_sel, float* logits, void* ws, int64_t ws_bytes, hipStream_t st,
                                bool x3) {
    if (!h) return fail(CBW_ERR_INVALID, "null handle");
    if (!h->finalized) return fail(CBW_ERR_STATE, "cbw_kws_finalize not called");
    if (B < 1 || (int64_t)B * std::max(K, 0) > INT32_MAX) return fail(CBW_ERR_INVALID, "B must be >= 1 and B * K < 2^31");
    ResizedExact r;
    const int chunk = x3 ? resized_x3_chunk() : EXACT_CHUNK;
    CHK(resized_exact_args(h, off_host, K, Tu, R, D, Ho, Wo, chunk, r));
    if (h->stem32.cout == 0 || h->blocks3.empty())
        return fail(CBW_ERR_STATE, "no fp32 network: call cbw_kws_build_exact first");
    if (n_sel < 0) return fail(CBW_ERR_INVALID, "n_sel must be >= 0");
    if (batch && n_sel > (int64_t)B * K) return fail(CBW_ERR_INVALID, "more pairs selected than B * K");
    if (n_sel == 0) return CBW_OK;
    if (K < 1) return fail(CBW_ERR_INVALID, "keywords selected but none given");
    if (!utt || !kwd || !off_dev || !sel || !logits || !ws) return fail(CBW_ERR_INVALID, "null argument");
    if ((uintptr_t)utt % 16 || (uintptr_t)kwd % 16) return fail(CBW_ERR_INVALID, "utt and kwd must be 16-byte aligned");
    if (ws_bytes < resized_exact_ws(h, off_host, K, Tu, D, Ho, Wo, x3)) return fail(CBW_ERR_OOM, "workspace too small");
    const int L = h->cfg.n_layers;
    float* rows = (float*)ws;
    void* tier_ws = (char*)ws + r.rows_bytes;
    // a pass's maps: the similarity rows of its keywords (cb_whisper.py:196), resized to (Ho, Wo) (:206)
    auto fill = [&](int c0, int cn, float* maps) {
        HIPCHK(cbw_sim_rows_f32(utt, B, kwd, off_dev, sel, c0, cn, K, R, L, Tu, D, r.tk_max, r.ld, rows, st));
        HIPCHK(cbw_sim_resize_f32(rows, B, off_dev, sel, c0, cn, K, R, L, Tu, r.tk_max, r.ld, Ho, Wo, maps, st));
        return (int)CBW_OK;
    };
    if (x3) return rescore_x3_passes(h, Ho, Wo, chunk, sel, n_sel, logits, tier_ws, st, fill);
    return rescore_passes(h, Ho, Wo, sel, n_sel, logits, tier_ws, st, nullptr, fill);
}

int cbw_kws_rescore_resized(cbw_kws* h, const float* utt, int Tu, const float* kwd, int R, int D, const int32_t* off_dev,
                            const int32_t* off_host, int K, int Ho, int Wo, const int32_t* sel, int n_sel, float* logits,
                            void* ws, int64_t ws_bytes, cbw_stream_t stream) {
    return rescore_resized_impl(h, utt, 1, false, Tu, kwd, R, D, off_dev, off_host, K, Ho, Wo, sel, n_sel, logits, ws,
                                ws_bytes, (hipStream_t)stream, false);
}

int cbw_kws_rescore_resized_x3(cbw_kws* h, const float* utt, int Tu, const float* kwd, int R, int D,
                               const int32_t* off_dev, const int32_t* off_host, int K, int Ho, int Wo, const int32_t* sel,
                               int n_sel, float* logits, void* ws, int64_t ws_bytes, cbw_stream_t stream) {
    return rescore_resized_impl(h, utt, 1, false, Tu, kwd, R, D, off_dev, off_host, K, Ho, Wo, sel, n_sel, logits, ws,
                                ws_bytes, (hipStream_t)stream, true);
}

// the two tiers for a batch of segments (cb_whisper.py:87-129): utt f32 [B][L][Tu][D], sel indexes the B * K pairs
int cbw_kws_rescore_resized_batch(cbw_kws* h, const float* utt, int B, int Tu, const float* kwd, int R, int D,
                                  const int32_t* off_dev, const int32_t* off_host, int K, int Ho, int Wo,
                                  const int32_t* sel, int n_sel, float* logits, void* ws, int64_t ws_bytes,
                                  cbw_stream_t stream) {
    return rescore_resized_impl(h, utt, B, true, Tu, kwd, R, D, off_dev, off_host, K, Ho, Wo, sel, n_sel, logits, ws,
                                ws_bytes, (hipStream_t)stream, false);
}

int cbw_kws_rescore_resized_x3_batch(cbw_kws* h, const float* utt, int B, int Tu, const float* kwd, int R, int D,
                                     const int32_t* off_dev, const int32_t* off_host, int K, int Ho, int Wo,
                                     const int32_t* sel, int n_sel, float* logits, void* ws, int64_t ws_bytes,
                                     cbw_stream_t stream) {
    return rescore_resized_impl(h, utt, B, true, Tu, kwd, R, D, off_dev, off_host, K, Ho, Wo, sel, n_sel, logits, ws,
                                ws_bytes, (hipStream_t)stream, true);
}

// the two stages one by one (tests): rows f32 [n_sel][L][tk_max][ld], then maps f32 NHWC [n_sel][Ho][Wo][L]
int cbw_kws_sim_rows_f32(const float* utt, int Tu, const float* kwd, int R, int D, int L, const int32_t* off_dev, int K,
                         const int32_t* sel, int n_sel, int tk_max, int ld, float* rows, cbw_stream_t stream) {
    if (!utt || !kwd || !off_dev || !sel || !rows) return fail(CBW_ERR_INVALID, "null argument");
    if (D <= 0 || D % 16) return fail(CBW_ERR_INVALID, "D must be a multiple of 16");
    if (Tu < 1 || R < 1 || L < 1 || L > 16 || K < 1 || n_sel < 1 || n_sel > 65535 || tk_max < 1 || ld < Tu)
        return fail(CBW_ERR_INVALID, "bad sizes");
    if ((uintptr_t)utt % 16 || (uintptr_t)kwd % 16) return fail(CBW_ERR_INVALID, "utt and kwd must be 16-byte aligned");
    HIPCHK(cbw_sim_rows_f32(utt, 1, kwd, off_dev, sel, 0, n_sel, K, R, L, Tu, D, tk_max, ld, rows, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_kws_sim_resize_f32(const float* rows, int Tu, int R, int L, const int32_t* off_dev, int K, const int32_t* sel,
                           int n_sel, int tk_max, int ld, int Ho, int Wo, float* maps, cbw_stream_t stream) {
    if (!rows || !off_dev || !sel || !maps) return fail(CBW_ERR_INVALID, "null argument");
    if (Tu < 1 || R < 1 || L < 1 || L > 16 || K < 1 || n_sel < 1 || tk_max < 1 || ld < Tu || Ho < 1 || Wo < 1)
        return fail(CBW_ERR_INVALID, "bad sizes");
    HIPCHK(cbw_sim_resize_f32(rows, 1, off_dev, sel, 0, n_sel, K, R, L, Tu, tk_max, ld, Ho, Wo, maps,
                              (hipStream_t)stream));
    return CBW_OK;
}

int cbw_kws_spot(const float* logits, const float* ghost, int K, float thr, int mode, float* prob, int32_t* idx,
                 int32_t* n, cbw_stream_t stream) {
    if (!idx || !n || K < 0 || (K > 0 && !logits)) return fail(CBW_ERR_INVALID, "bad arguments");
    if (K == 0) {
        HIPCHK(hipMemsetAsync(n, 0, sizeof(int32_t), (hipStream_t)stream));
        return CBW_OK;
    }
    if (mode != 0 && mode != 1) return fail(CBW_ERR_INVALID, "cbw_kws_spot: mode must be 0 (threshold) or 1 (argmax)");
    HIPCHK(cbw_spot(logits, ghost, K, thr, 0.f, mode, prob, idx, n, (hipStream_t)stream));
    return CBW_OK;
}

int64_t cbw_checksum_workspace_bytes(void) { return cbw_checksum_scratch_bytes(); }

int cbw_checksum(const void* data, int64_t bytes, uint64_t* out, void* ws, int64_t ws_bytes, cbw_stream_t stream) {
    if (!out || !ws || bytes < 0 || (bytes > 0 && !data)) return fail(CBW_ERR_INVALID, "null argument");
    if ((uintptr_t)data & 15) return fail(CBW_ERR_INVALID, "cbw_checksum: data must be 16-byte aligned");
    if (ws_bytes < cbw_checksum_scratch_bytes()) return fail(CBW_ERR_OOM, "checksum workspace too small");
    HIPCHK(cbw_checksum64(data, bytes, out, (uint64_t*)ws, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_kws_band(const float* logits, const float* ghost, int K, float thr, float band, int32_t* idx, int32_t* n,
                 cbw_stream_t stream) {
    if (!idx || !n || K < 0 || (K > 0 && !logits) || !(band >= 0.f)) return fail(CBW_ERR_INVALID, "bad arguments");
    if (K == 0) {
        HIPCHK(hipMemsetAsync(n, 0, sizeof(int32_t), (hipStream_t)stream));
        return CBW_OK;
    }
    HIPCHK(cbw_spot(logits, ghost, K, thr, band, 2, nullptr, idx, n, (hipStream_t)stream));
    return CBW_OK;
}
int cbw_kws_band_scaled(const float* logits, const float* ghost, int K, float thr, float coef, int32_t* idx, int32_t* n,
                        cbw_stream_t stream) {
    if (!idx || !n || K < 0 || (K > 0 && !logits) || !(coef >= 0.f)) return fail(CBW_ERR_INVALID, "bad arguments");
    if (K == 0) {
        HIPCHK(hipMemsetAsync(n, 0, sizeof(int32_t), (hipStream_t)stream));
        return CBW_OK;
    }
    HIPCHK(cbw_spot(logits, ghost, K, thr, coef, 3, nullptr, idx, n, (hipStream_t)stream));
    return CBW_OK;
}

// ------------------------------------------------------------------ resample + downmix
namespace {
struct ResamplePlan {
    int o = 1, n = 1, width = 0, T = 0;   // reduced rates, half width, taps per phase (T = 0: orig == new)
    int64_t entries = 0;                  // n * T
};

// torchaudio _get_sinc_resample_kernel's sizes (lowpass_filter_width 6, rolloff 0.99), in its float64 arithmetic
int resample_plan(int orig, int new_, ResamplePlan* p) {
    if (orig < 1 || new_ < 1) return fail(CBW_ERR_INVALID, "resample: sample rates must be >= 1");
    const int g = std::gcd(orig, new_);
    p->o = orig / g;
    p->n = new_ / g;
    if (p->o == p->n) return CBW_OK;
    const double base = std::min(p->o, p->n) * 0.99;
    const double width = std::ceil(6.0 * p->o / base);
    const double entries = (2.0 * width + p->o) * p->n;
    if (entries > (double)CBW_RESAMPLE_MAX_TABLE)
        return fail(CBW_ERR_INVALID, "resample: " + std::to_string(orig) + " -> " + std::to_string(new_) + " needs " +
                                         std::to_string(p->n) + " phases x " + std::to_string((int64_t)(2.0 * width + p->o)) +
                                         " taps, above CBW_RESAMPLE_MAX_TABLE entries");
    p->width = (int)width;
    p->T = 2 * p->width + p->o;
    p->entries = (int64_t)p->n * p->T;
    return CBW_OK;
}

// kernel[j][k] in float64, rounded to fp32 once, stored phase-minor: tab[k * n + j]
void resample_table(const ResamplePlan& p, float* tab) {
    const double base = std::min(p.o, p.n) * 0.99, scale = base / p.o;
    for (int k = 0; k < p.T; ++k)
        for (int j = 0; j < p.n; ++j) {
            double t = (-(double)j / p.n + (double)(k - p.width) / p.o) * base;
            t = std::min(6.0, std::max(-6.0, t));
            const double c = std::cos(t * M_PI / 12.0), a = t * M_PI;
            tab[(size_t)k * p.n + j] = (float)((a == 0.0 ? 1.0 : std::sin(a) / a) * c * c * scale);
        }
}

// a rate pair's table in pinned host memory, built on first use and kept for the process (the source of the
// stream-ordered upload must outlive the call)
int resample_host_table(const ResamplePlan& p, const float** out) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, float*> tables;
    std::lock_guard<std::mutex> lock(mu);
    auto it = tables.find({p.o, p.n});
    if (it == tables.end()) {
        void* host = nullptr;
        if (hipHostMalloc(&host, (size_t)p.entries * sizeof(float), hipHostMallocPortable) != hipSuccess)
            return fail(CBW_ERR_OOM, "resample: hipHostMalloc of the coefficient table failed");
        resample_table(p, (float*)host);
        it = tables.emplace(std::make_pair(p.o, p.n), (float*)host).first;
    }
    *out = it->second;
    return CBW_OK;
}

int resample_len(int64_t n, const ResamplePlan& p, int64_t* out) {
    if (n < 0) return fail(CBW_ERR_INVALID, "resample: n < 0");
    if (n > (std::numeric_limits<int64_t>::max() - p.o) / p.n) return fail(CBW_ERR_INVALID, "resample: n * new_ overflows");
    *out = (n * p.n + p.o - 1) / p.o;
    return CBW_OK;
}
}  // namespace

int64_t cbw_resample_len(int64_t n, int orig, int new_) {
    ResamplePlan p;
    int64_t len = 0;
    if (n < 0) return fail(CBW_ERR_INVALID, "resample: n < 0");
    CHK(resample_plan(orig, new_, &p));
    CHK(resample_len(n, p, &len));
    return len;
}

int64_t cbw_resample_ws_bytes(int orig, int new_) {
    ResamplePlan p;
    CHK(resample_plan(orig, new_, &p));
    return p.entries * (int64_t)sizeof(float);
}

int cbw_resample(const float* pcm, int channels, int64_t n, int orig, int new_, float* out, void* ws, int64_t ws_bytes,
                 cbw_stream_t stream) {
    if (!pcm || !out) return fail(CBW_ERR_INVALID, "cbw_resample: null pcm or out");
    if (channels < 1) return fail(CBW_ERR_INVALID, "cbw_resample: channels < 1");
    if (n < 0) return fail(CBW_ERR_INVALID, "cbw_resample: n < 0");
    ResamplePlan p;
    int64_t out_len = 0;
    CHK(resample_plan(orig, new_, &p));
    CHK(resample_len(n, p, &out_len));
    if (n > std::numeric_limits<int64_t>::max() / channels)
        return fail(CBW_ERR_INVALID, "cbw_resample: channels * n overflows");
    if ((std::max(out_len, n) + 255) / 256 > 0x7fffffffLL)
        return fail(CBW_ERR_INVALID, "cbw_resample: more than 2^31 - 1 blocks of 256 samples");
    if (p.T && (!ws || ((uintptr_t)ws & 3) || ws_bytes < p.entries * (int64_t)sizeof(float)))
        return fail(CBW_ERR_INVALID, "cbw_resample: ws null, misaligned or smaller than cbw_resample_ws_bytes");
    if (n == 0) return CBW_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!p.T) {
        if (channels == 1) HIPCHK(hipMemcpyAsync(out, pcm, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
        else HIPCHK(cbw_downmix(pcm, channels, n, out, st));
        return CBW_OK;
    }
    const float* host = nullptr;
    CHK(resample_host_table(p, &host));
    HIPCHK(hipMemcpyAsync(ws, host, (size_t)p.entries * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(cbw_resample_taps(pcm, channels, n, (const float*)ws, p.o, p.n, p.width, p.T, out, out_len, st));
    return CBW_OK;
}

// ------------------------------------------------------------------ mel
namespace {
int mel_impl(const float* pcm, int64_t n, int n_mel, float* out, uint16_t* packed, int cpad, void* ws,
             cbw_stream_t stream, bool long_form) {
    static thread_local std::map<std::pair<int, int>, std::shared_ptr<DevBuf>> tables;   // (device, n_mel) -> [filters|twiddle]
    if (!pcm || !out || !ws || n < 0 || n_mel <= 0 || n_mel > 256) return fail(CBW_ERR_INVALID, "bad arguments");
    if (packed && (cpad < n_mel || cpad % 64)) return fail(CBW_ERR_INVALID, "cpad must be >= n_mel and a multiple of 64");
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    auto key = std::make_pair(dev, n_mel);
    auto it = tables.find(key);
    if (it == tables.end()) {
        // slaney mel filter bank (HF audio_utils.mel_filter_bank(norm='slaney', mel_scale='slaney')), [201][n_mel]
        const int nf = 201;
        auto hz2mel = [](double f) { return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) * (27.0 / std::log(6.4)) : 3.0 * f / 200.0; };
        auto mel2hz = [](double m) { return m >= 15.0 ? 1000.0 * std::exp(std::log(6.4) / 27.0 * (m - 15.0)) : 200.0 * m / 3.0; };
        std::vector<double> ff(n_mel + 2);
        const double m0 = hz2mel(0.0), m1 = hz2mel(8000.0);
        for (int i = 0; i < n_mel + 2; ++i) ff[i] = mel2hz(m0 + (m1 - m0) * i / (n_mel + 1));
        std::vector<float> tab((size_t)nf * n_mel + 800);
        for (int f = 0; f < nf; ++f) {
            const double fr = 8000.0 * f / (nf - 1);
            for (int m = 0; m < n_mel; ++m) {
                const double down = (fr - ff[m]) / (ff[m + 1] - ff[m]);
                const double up = (ff[m + 2] - fr) / (ff[m + 2] - ff[m + 1]);
                const double v = std::max(0.0, std::min(down, up)) * 2.0 / (ff[m + 2] - ff[m]);
                tab[(size_t)f * n_mel + m] = (float)v;
            }
        }
        for (int k = 0; k < 400; ++k) {
            tab[(size_t)nf * n_mel + k] = (float)std::cos(2.0 * M_PI * k / 400.0);
            tab[(size_t)nf * n_mel + 400 + k] = (float)-std::sin(2.0 * M_PI * k / 400.0);
        }
        auto buf = std::make_shared<DevBuf>();
        CHK(buf->upload(tab));
        it = tables.emplace(key, buf).first;
    }
    const float* filters = it->second->as<float>();
    const float* tw = filters + (size_t)201 * n_mel;
    hipStream_t st = (hipStream_t)stream;
    if (long_form) {
        const int frames = (int)(n / 160);
        HIPCHK(cbw_mel_frames(pcm, (int)n, filters, tw, out, n_mel, st, (int)n, frames));
        HIPCHK(cbw_mel_finish(out, n_mel, (float*)ws, nullptr, 0, st, frames));
        return CBW_OK;
    }
    HIPCHK(cbw_mel_frames(pcm, (int)std::min<int64_t>(n, 480000), filters, tw, out, n_mel, st));
    HIPCHK(cbw_mel_finish(out, n_mel, (float*)ws, packed, packed ? cpad : 0, st));
    return CBW_OK;
}
}  // namespace

int cbw_mel(const float* pcm, int64_t n, int n_mel, float* out, uint16_t* packed, int cpad, void* ws,
            cbw_stream_t stream) {
    return mel_impl(pcm, n, n_mel, out, packed, cpad, ws, stream, false);
}

int cbw_mel_long(const float* pcm, int64_t n, int n_mel, float* out, void* ws, cbw_stream_t stream) {
    if (n < 400 || n > 0x7fffffffLL) return fail(CBW_ERR_INVALID, "cbw_mel_long: 400 <= n_samples < 2^31");
    return mel_impl(pcm, n, n_mel, out, nullptr, 0, ws, stream, true);
}



// ------------------------------------------------------------------ encoder
int cbw_encoder_create(const cbw_encoder_config* cfg, cbw_encoder** out) {
    if (!cfg || !out) return fail(CBW_ERR_INVALID, "null argument");
    if (cfg->n_heads < 1 || cfg->d_model % 128 || cfg->d_model / cfg->n_heads != 64 || cfg->ffn_dim % 128 ||
        cfg->n_layers < 1)
        return fail(CBW_ERR_INVALID, "encoder needs d_model % 128 == 0, head_dim 64, ffn_dim % 128 == 0");
    auto h = std::make_unique<cbw_encoder>();
    h->cfg = *cfg;
    h->cpad = (cfg->n_mel + 63) / 64 * 64;
    CHK(h->zero.alloc(256));
    HIPCHK(hipMemset(h->zero.p, 0, 256));
    *out = h.release();
    return CBW_OK;
}

int cbw_encoder_destroy(cbw_encoder* h) {
    delete h;
    return CBW_OK;
}

int cbw_encoder_set_param(cbw_encoder* h, const char* name, const float* host, int64_t numel) {
    if (!h) return fail(CBW_ERR_INVALID, "null handle");
    h->finalized = false;
    return h->ps.set(name, host, numel);
}

}  // extern "C"
namespace {
int upload_vec(const ParamStore& ps, const std::string& n, size_t numel, DevBuf& dst) {
    int rc;
    const auto* v = ps.get(n, numel, &rc);
    if (!v) return rc;
    return dst.upload(*v);
}
int upload_linear(const ParamStore& ps, const std::string& n, int cout, int cin, bool has_bias, ConvW& c,
                  float scale = 1.0f) {
    int rc;
    const auto* w = ps.get(n + ".weight", (size_t)cout * cin, &rc);
    if (!w) return rc;
    c.cin = cin; c.cout = cout; c.k = 1; c.stride = 1; c.relu = false;
    std::vector<float> ws(*w);
    for (auto& x : ws) x *= scale;
    CHK(c.w.upload(to_bf16(ws)));
    std::vector<float> b(cout, 0.f);
    if (has_bias) {
        const auto* bv = ps.get(n + ".bias", cout, &rc);
        if (!bv) return rc;
        for (int i = 0; i < cout; ++i) b[i] = (*bv)[i] * scale;
    }
    return c.b.upload(b);
}
int upload_ln(const ParamStore& ps, const std::string& n, int D, LNorm& ln) {
    CHK(upload_vec(ps, n + ".weight", D, ln.g));
    return upload_vec(ps, n + ".bias", D, ln.b);
}
// fused QKV [3D][D] of attention block `p`: q (scaled by hd^-1/2, HF WhisperAttention.scaling) | k (no bias) | v
int pack_qkv(const ParamStore& ps, const std::string& p, int D, ConvW& c) {
    const float qscale = 1.0f / std::sqrt(64.0f);
    int rc;
    const auto* wq = ps.get(p + ".q_proj.weight", (size_t)D * D, &rc); if (!wq) return rc;
    const auto* wk = ps.get(p + ".k_proj.weight", (size_t)D * D, &rc); if (!wk) return rc;
    const auto* wv = ps.get(p + ".v_proj.weight", (size_t)D * D, &rc); if (!wv) return rc;
    const auto* bq = ps.get(p + ".q_proj.bias", D, &rc); if (!bq) return rc;
    const auto* bv = ps.get(p + ".v_proj.bias", D, &rc); if (!bv) return rc;
    std::vector<float> w((size_t)3 * D * D), b((size_t)3 * D, 0.f);
    for (size_t j = 0; j < (size_t)D * D; ++j) {
        w[j] = (*wq)[j] * qscale;
        w[(size_t)D * D + j] = (*wk)[j];
        w[(size_t)2 * D * D + j] = (*wv)[j];
    }
    for (int j = 0; j < D; ++j) { b[j] = (*bq)[j] * qscale; b[2 * D + j] = (*bv)[j]; }
    c.cin = D; c.cout = 3 * D; c.k = 1;
    CHK(c.w.upload(to_bf16(w)));
    return c.b.upload(b);
}
// the fields of layer `p` ("layers.<i>") that the encoder and the decoder share
int load_xf_layer(const ParamStore& ps, const std::string& p, int D, int F, XfLayer& L) {
    CHK(upload_ln(ps, p + ".self_attn_layer_norm", D, L.ln1));
    CHK(pack_qkv(ps, p + ".self_attn", D, L.qkv));
    CHK(upload_linear(ps, p + ".self_attn.out_proj", D, D, true, L.out));
    CHK(upload_ln(ps, p + ".final_layer_norm", D, L.ln_mlp));
    CHK(upload_linear(ps, p + ".fc1", F, D, true, L.fc1));
    return upload_linear(ps, p + ".fc2", D, F, true, L.fc2);
}

// the K/V cache append of a decode step's qkv projection: k / v = the layer's cache at position 0 (row stride ld
// elements), written at position pos, or at the position(s) read on the device from pos_dev (GemvArgs::kv_pos)
struct KvAppend {
    uint16_t *k = nullptr, *v = nullptr;
    int64_t ld = 0;
    int D = 0, pos = 0;
    const int32_t* pos_dev = nullptr;
    int pos_rows = 0;
};
// The one place a GemvArgs is filled: y[M][N] = act(x . w^T + bias (+ res)) over bf16 rows x, or with xf over
// LN(xf) (the LayerNorm prologue); kv_k (optional): the output's K and V thirds also go to the cache rows kv_k / kv_v
GemvArgs gemv_args(const uint16_t* x, const float* xf, int ldx, const float* ln_g, const float* ln_b, float ln_eps,
                   const void* w, const float* bias, const void* res, int res_ld, void* y, int ldy, int M, int N, int K,
                   int flags, uint16_t* kv_k = nullptr, uint16_t* kv_v = nullptr, int64_t kv_ld = 0, int kv_D = 0,
                   const int32_t* kv_pos = nullptr, int kv_pos_rows = 0) {
    GemvArgs a{};
    a.x = xf ? nullptr : (const bf16*)x; a.ldx = ldx; a.w = (const bf16*)w; a.bias = bias;
    a.res = res; a.res_ld = res_ld; a.y = y; a.ldy = ldy;
    a.M = M; a.N = N; a.K = K; a.flags = flags;
    a.xf = xf; a.ln_g = ln_g; a.ln_b = ln_b; a.ln_eps = ln_eps;
    if (kv_k) {
        a.kv_k = (bf16*)kv_k; a.kv_v = (bf16*)kv_v; a.kv_ld = kv_ld; a.kv_D = kv_D;
        a.kv_pos = kv_pos; a.kv_pos_rows = kv_pos_rows;
    }
    return a;
}

// The Linears of one encoder / decoder entry call, all over M rows on stream st: on the skinny GEMV (gemv.hip) where
// gemv is set (<= 16 rows, CBW_DEC_GEMV), else on the implicit-GEMM tiles; with fuse a LayerNorm in front of a Linear
// runs in the GEMV's prologue (and the K/V append in its epilogue), else as launches of their own (LayerNorm into the
// bf16 rows ln_out).  The knobs are read once per entry call, by whoever builds the LinearRun.
struct LinearRun {
    int M;
    hipStream_t st;
    const void* zero;
    bool gemv, fuse;
    uint16_t* ln_out;
    float* splitk = nullptr;   // the encoder's split-K partial sums, for its residual Linears (out-projection, fc2)
    // cbw_decoder_step_wide: the GEMV as row groups of 16 in one launch (cbw_gemv_wide), up to CBW_DEC_WIDE_ROWS rows
    bool wide = false, wide_groups_fast = false;

    int lin(const ConvW& c, const void* x, void* y, const void* res, int flags) const {
        if (!gemv) return launch_conv(c, x, 1, 1, M, y, res, flags, zero, st, nullptr, nullptr, res ? splitk : nullptr);
        return run(c, (const uint16_t*)x, nullptr, nullptr, y, res, flags, KvAppend{});
    }
    int ln_lin(const float* h32, const LNorm& ln, const ConvW& c, void* y, int flags, const KvAppend& kv = {}) const {
        if (fuse) return run(c, nullptr, h32, &ln, y, nullptr, flags, kv);
        HIPCHK(cbw_layernorm(h32, ln.g.as<float>(), ln.b.as<float>(), ln_out, nullptr, M, c.cin, 1e-5f, st));
        CHK(lin(c, ln_out, y, nullptr, flags));
        if (kv.k) HIPCHK(cbw_dec_kv_append((const uint16_t*)y, kv.k, kv.v, M, kv.D, (int)(kv.ld / kv.D), kv.pos, st));
        return CBW_OK;
    }
    int add_lin(const ConvW& c, const void* x, float* h) const {   // residual Linear of the fp32 stream: h += c(x)
        return lin(c, x, h, h, CBW_EPI_RES_F32 | CBW_EPI_OUT_F32);
    }
    int run(const ConvW& c, const uint16_t* x, const float* xf, const LNorm* ln, void* y, const void* res, int flags,
            const KvAppend& kv) const {
        const size_t at = kv.pos_dev ? 0 : (size_t)kv.pos * kv.D;
        const GemvArgs g = gemv_args(x, xf, c.cin, ln ? ln->g.as<float>() : nullptr, ln ? ln->b.as<float>() : nullptr,
                                     ln ? 1e-5f : 0.f, c.w.p, c.b.as<float>(), res, res ? c.cout : 0, y, c.cout, M,
                                     c.cout, c.cin, flags | (c.relu ? CBW_EPI_RELU : 0), kv.k ? kv.k + at : nullptr,
                                     kv.k ? kv.v + at : nullptr, kv.ld, kv.D, kv.pos_dev, kv.pos_rows);
        HIPCHK(wide ? cbw_gemv_wide(g, st, wide_groups_fast) : cbw_gemv(g, st));
        return CBW_OK;
    }
};

// attention sub-block of a pre-LN layer: h += out(attend()), where attend reads q = proj(LN(h)) and writes att
template <class Attend>
int attn_block(const LinearRun& r, const LNorm& ln, const ConvW& proj, const ConvW& out, float* h, uint16_t* q,
               const uint16_t* att, const KvAppend& kv, Attend&& attend) {
    CHK(r.ln_lin(h, ln, proj, q, 0, kv));
    CHK(attend());
    return r.add_lin(out, att, h);
}
// MLP sub-block: h += fc2(gelu(fc1(LN(h)))), f = the fc1 rows
int mlp_block(const LinearRun& r, const XfLayer& L, float* h, uint16_t* f) {
    CHK(r.ln_lin(h, L.ln_mlp, L.fc1, f, CBW_EPI_GELU));
    return r.add_lin(L.fc2, f, h);
}
}  // namespace
extern "C" {

int cbw_encoder_finalize(cbw_encoder* h) {
    if (!h) return fail(CBW_ERR_INVALID, "null handle");
    const int D = h->cfg.d_model, F = h->cfg.ffn_dim, nm = h->cfg.n_mel, cp = h->cpad;
    // the stem's k3 convs, torch [D][cin][3] -> [D][1][3][cpad]: conv1 (n_mel in, padded to cpad), conv2 (D in)
    auto load_k3 = [&](const std::string& n, int cin, int cpad, ConvW& c) -> int {
        int rc;
        const auto* w = h->ps.get(n + ".weight", (size_t)D * cin * 3, &rc); if (!w) return rc;
        std::vector<float> o((size_t)D * 3 * cpad, 0.f);
        for (int co = 0; co < D; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int k = 0; k < 3; ++k) o[((size_t)co * 3 + k) * cpad + ci] = (*w)[((size_t)co * cin + ci) * 3 + k];
        c.cin = cpad; c.cout = D; c.k = 3;
        CHK(c.w.upload(to_bf16(o)));
        return upload_vec(h->ps, n + ".bias", D, c.b);
    };
    CHK(load_k3("conv1", nm, cp, h->conv1));
    CHK(load_k3("conv2", D, D, h->conv2));
    CHK(upload_vec(h->ps, "embed_positions.weight", (size_t)1500 * D, h->pos));
    h->layers.clear();
    h->layers.resize(h->cfg.n_layers);
    for (int i = 0; i < h->cfg.n_layers; ++i)
        CHK(load_xf_layer(h->ps, "layers." + std::to_string(i), D, F, h->layers[i]));
    CHK(upload_ln(h->ps, "layer_norm", D, h->lnf));
    h->finalized = true;
    return CBW_OK;
}

}  // extern "C"
namespace {
bool encoder_splitk_enabled() {   // CBW_ENC_SPLITK=0 runs the out-projection / fc2 GEMMs unsplit (A/B experiments)
    const char* e = getenv("CBW_ENC_SPLITK");
    return !(e && atoi(e) == 0);
}
// K-split of the encoder's few-tile GEMMs (out-projection, fc2: M = B x 1500 rows, N = d_model): the factor
// cbw_conv_splitk_factor picks for each, and the fp32 partial-sum floats it needs
int64_t encoder_splitk_floats(const cbw_encoder* h, int B) {
    if (!encoder_splitk_enabled()) return 0;
    const int D = h->cfg.d_model, F = h->cfg.ffn_dim, M = B * 1500;
    int64_t n = 0;
    for (int K : {D, F}) {
        const int S = cbw_conv_splitk_factor(linear_args(M, K, D));
        if (S > 1) n = std::max<int64_t>(n, (int64_t)S * M * D);
    }
    return n;
}
}  // namespace
extern "C" {

int64_t cbw_encoder_workspace_bytes(cbw_encoder* h, int B) {
    if (!h || B <= 0) return -1;
    const size_t D = h->cfg.d_model, F = h->cfg.ffn_dim, T = 1500;
    return (int64_t)(align_up(B * T * D * 4) + align_up(B * 3000 * D * 2) + align_up(B * T * D * 2) +
                     align_up(B * T * 3 * D * 2) + align_up(B * T * D * 2) + align_up(B * T * F * 2) +
                     align_up((size_t)encoder_splitk_floats(h, B) * 4));
}

int cbw_encoder_hs(cbw_encoder* h, const uint16_t* mel, int B, const int32_t* layer_ids, int n_ids, int normalize,
                   float* hs, void* ws, int64_t ws_bytes, cbw_stream_t stream) {
    if (!h || !mel || !layer_ids || !hs || B <= 0 || n_ids <= 0) return fail(CBW_ERR_INVALID, "bad arguments");
    if (!h->finalized) return fail(CBW_ERR_STATE, "cbw_encoder_finalize not called");
    if (ws_bytes < cbw_encoder_workspace_bytes(h, B)) return fail(CBW_ERR_OOM, "encoder workspace too small");
    const int N = h->cfg.n_layers, D = h->cfg.d_model, T = 1500, M = B * T, H = h->cfg.n_heads;
    int max_id = 0;
    for (int j = 0; j < n_ids; ++j) {
        if (layer_ids[j] < 0 || layer_ids[j] > N) return fail(CBW_ERR_INVALID, "layer id out of range [0, n_layers]");
        max_id = std::max(max_id, (int)layer_ids[j]);
    }
    const int last_layer = (normalize & 2) ? std::min(max_id, N) : N;   // bit 1: stop after the last requested state
    hipStream_t st = (hipStream_t)stream;
    char* p = (char*)ws;
    float* hbuf = (float*)p; p += align_up((size_t)M * D * 4);
    uint16_t* x1 = (uint16_t*)p; p += align_up((size_t)B * 3000 * D * 2);
    uint16_t* a = (uint16_t*)p; p += align_up((size_t)M * D * 2);
    uint16_t* qkv = (uint16_t*)p; p += align_up((size_t)M * 3 * D * 2);
    uint16_t* att = (uint16_t*)p; p += align_up((size_t)M * D * 2);
    uint16_t* f = (uint16_t*)p; p += align_up((size_t)M * h->cfg.ffn_dim * 2);
    float* part = encoder_splitk_floats(h, B) > 0 ? (float*)p : nullptr;   // split-K partial sums
    auto capture = [&](int state) -> int {
        for (int j = 0; j < n_ids; ++j) {
            if (layer_ids[j] != state) continue;
            for (int b = 0; b < B; ++b)
                HIPCHK(hipMemcpyAsync(hs + (((size_t)b * n_ids + j) * T) * D, hbuf + (size_t)b * T * D,
                                      (size_t)T * D * 4, hipMemcpyDeviceToDevice, st));
        }
        return CBW_OK;
    };
    // the stem's k3 convs (p1) over n clips of 3000 frames, + GELU
    auto conv_k3 = [&](const ConvW& c, const void* x, const void* res, void* y, int n, int sw, int flags) {
        ConvArgs a{};
        a.x = x; a.w = c.w.p; a.bias = c.b.as<float>(); a.res = res; a.y = y; a.zero = h->zero.p;
        conv_geometry(a, n, 1, 3000, c.cin, D, 1, 3, 1, sw, 0, 1);
        a.res_ld = a.y_ld = D;
        a.flags = CBW_EPI_GELU | flags;
        return cbw_conv_igemm(a, st);
    };
    // conv1: [B][1][3000][cpad] -> [B][1][3000][D]; conv2 (s2) + positions (per clip: the position table is [1500][D])
    HIPCHK(conv_k3(h->conv1, mel, nullptr, x1, B, 1, 0));
    for (int b = 0; b < B; ++b)
        HIPCHK(conv_k3(h->conv2, x1 + (size_t)b * 3000 * D, h->pos.p, hbuf + (size_t)b * T * D, 1, 2,
                       CBW_EPI_RES_F32 | CBW_EPI_OUT_F32 | CBW_EPI_RES_AFTER_ACT));
    CHK(capture(0));
    const LinearRun run{M, st, h->zero.p, false, false, a, part};
    for (int i = 0; i < last_layer && i < N; ++i) {
        const XfLayer& L = h->layers[i];
        CHK(attn_block(run, L.ln1, L.qkv, L.out, hbuf, qkv, att, {}, [&]() -> int {
            HIPCHK(cbw_attention(qkv, att, B, T, H, 64, st));
            return CBW_OK;
        }));
        CHK(mlp_block(run, L, hbuf, f));
        if (i + 1 < N) CHK(capture(i + 1));
    }
    if (last_layer >= N) {
        for (int j = 0; j < n_ids; ++j) {
            if (layer_ids[j] != N) continue;
            for (int b = 0; b < B; ++b)
                HIPCHK(cbw_layernorm(hbuf + (size_t)b * T * D, h->lnf.g.as<float>(), h->lnf.b.as<float>(), nullptr,
                                     hs + (((size_t)b * n_ids + j) * T) * D, T, D, 1e-5f, st));
        }
    }
    if (normalize & 1) HIPCHK(cbw_l2norm_rows_f32(hs, (int64_t)B * n_ids * T, D, st));
    return CBW_OK;
}

// ------------------------------------------------------------------ decoder
}  // extern "C"

struct cbw_decoder {
    cbw_decoder_config cfg{};
    ParamStore ps;
    bool finalized = false;
    int Vpad = 0;
    DevBuf zero;
    ConvW emb;   // the padded token embedding [Vpad][D], also the tied vocabulary projection (a Linear without bias)
    DevBuf pos;
    struct Layer : XfLayer {   // + the cross-attention block
        LNorm ln_x;
        ConvW cq, ck, cv, co;
    };
    std::vector<Layer> layers;
    LNorm lnf;
};

namespace {
struct DecState {
    uint16_t *ks, *vs, *kc, *vc, *a, *qkv, *att, *qc, *f, *scratch, *enc;
    float* h;
    // prefill activations (max_len rows): residual stream, LN out, qkv, attention out, cross q, fc1 out
    float* ph;
    uint16_t *pa, *pqkv, *patt, *pqc, *pf;
    float* apart;   // split-key attention partials
    char* end;
};
bool dec_fuse_enabled() {   // CBW_DEC_FUSE=0 keeps the step's LayerNorms and K/V append as separate launches (A/B)
    const char* e = getenv("CBW_DEC_FUSE");
    return !(e && atoi(e) == 0);
}
bool dec_split_enabled() {   // CBW_DEC_SPLIT=0 runs the step's attention on the one-workgroup-per-row kernel (A/B)
    const char* e = getenv("CBW_DEC_SPLIT");
    return !(e && atoi(e) == 0);
}
// CBW_DEC_GEMV=0 runs the decode-step Linears on the tile kernels (A/B); max_rows: 16, or CBW_DEC_WIDE_ROWS where the
// rows run as groups of 16 (cbw_gemv_wide)
bool dec_gemv_enabled(int B, int max_rows = 16) {
    const char* e = getenv("CBW_DEC_GEMV");
    return B <= max_rows && !(e && atoi(e) == 0);
}
// CBW_GEMV_WIDE_ORDER=groups makes the row groups of a wide launch the fast grid coordinate (A/B; default: the
// column blocks, docs/MEASUREMENT_LOG.md)
static_assert(GV_WIDE_ROWS == CBW_DEC_WIDE_ROWS, "gemv_route.h / cbw.h");
bool gemv_wide_groups_fast() {
    const char* e = getenv("CBW_GEMV_WIDE_ORDER");
    return e && !strcmp(e, "groups");
}

DecState dec_carve(const cbw_decoder* h, void* state, int B, int Benc) {
    const size_t L = h->cfg.n_layers, D = h->cfg.d_model, F = h->cfg.ffn_dim, ML = h->cfg.max_len;
    char* p = (char*)state;
    DecState s;
    s.ks = (uint16_t*)p; p += align_up(L * B * ML * D * 2);
    s.vs = (uint16_t*)p; p += align_up(L * B * ML * D * 2);
    s.kc = (uint16_t*)p; p += align_up(L * Benc * 1500 * D * 2);
    s.vc = (uint16_t*)p; p += align_up(L * Benc * 1500 * D * 2);
    s.h = (float*)p; p += align_up((size_t)B * D * 4);
    s.a = (uint16_t*)p; p += align_up((size_t)B * D * 2);
    s.qkv = (uint16_t*)p; p += align_up((size_t)B * 3 * D * 2);
    s.att = (uint16_t*)p; p += align_up((size_t)B * D * 2);
    s.qc = (uint16_t*)p; p += align_up((size_t)B * D * 2);
    s.f = (uint16_t*)p; p += align_up((size_t)B * F * 2);
    s.scratch = (uint16_t*)p; p += align_up((size_t)B * ML * D * 2);
    s.enc = (uint16_t*)p; p += align_up((size_t)Benc * 1500 * D * 2);
    s.ph = (float*)p; p += align_up(ML * D * 4);
    s.pa = (uint16_t*)p; p += align_up(ML * D * 2);
    s.pqkv = (uint16_t*)p; p += align_up(ML * 3 * D * 2);
    s.patt = (uint16_t*)p; p += align_up(ML * D * 2);
    s.pqc = (uint16_t*)p; p += align_up(ML * D * 2);
    s.pf = (uint16_t*)p; p += align_up(ML * F * 2);
    s.apart = (float*)p; p += align_up((size_t)cbw_dec_attn_split_floats(B, h->cfg.n_heads) * 4);
    s.end = p;
    return s;
}
int64_t dec_state_bytes(const cbw_decoder* h, int B, int Benc) {   // the carve of a state at address 0
    return (int64_t)(dec_carve(h, nullptr, B, Benc).end - (char*)nullptr);
}
// What every decoder compute entry checks first (ptrs_ok: its own pointer arguments): a finalized handle and B rows
// that are a positive multiple of the Benc encoder slots.  The entry's own range checks come next, then dec_state.
int dec_check(const cbw_decoder* h, bool ptrs_ok, int B, int Benc) {
    if (!h || !ptrs_ok) return fail(CBW_ERR_INVALID, "null argument");
    if (!h->finalized) return fail(CBW_ERR_STATE, "cbw_decoder_finalize not called");
    if (B <= 0 || Benc <= 0 || B % Benc) return fail(CBW_ERR_INVALID, "B must be a positive multiple of Benc");
    return CBW_OK;
}
// ... and last: the state's size, and its carve
int dec_state(const cbw_decoder* h, void* state, int64_t state_bytes, int B, int Benc, DecState* s) {
    if (state_bytes < dec_state_bytes(h, B, Benc)) return fail(CBW_ERR_OOM, "decoder state too small");
    *s = dec_carve(h, state, B, Benc);
    return CBW_OK;
}
// the step's attention: split-key kernel (K/V read once per kv batch) when it applies, else one workgroup per row
int dec_self_split_keys() {   // CBW_DEC_SELF_SPLIT=N: self-attention over more than N keys on the split kernel
    const char* e = getenv("CBW_DEC_SELF_SPLIT");
    return e ? atoi(e) : 0;
}
bool dec_self_one_launch() {   // CBW_DEC_SELF_ONE=0: self-attention on the split kernel + combine (A/B)
    const char* e = getenv("CBW_DEC_SELF_ONE");
    return !(e && atoi(e) == 0);
}
// the kernel a step's attention runs on (the only statement of the routing: dec_attend launches what this names,
// cbw_decode_attention asks it which operands a call needs)
enum class DecAttn { SelfOne, Row, Split };
DecAttn dec_attend_route(int n_keys, int rows_per_kv, bool has_pos, bool self) {
    if (self && rows_per_kv == 1 && n_keys <= 448 && dec_split_enabled() && dec_self_one_launch())
        return DecAttn::SelfOne;
    if (self && !has_pos && n_keys <= dec_self_split_keys()) return DecAttn::Row;
    if (has_pos || (dec_split_enabled() && rows_per_kv <= 8)) return DecAttn::Split;
    return DecAttn::Row;
}
// part: cbw_dec_attn_split_floats(B, H) floats, the split kernel's partials (the state's apart)
hipError_t dec_attend(float* part, const uint16_t* q, int ldq, const uint16_t* kc, const uint16_t* vc,
                      int64_t kv_bstride, int n_keys, int rows_per_kv, uint16_t* out, int B, int H, int D,
                      hipStream_t st, const int* n_keys_pos = nullptr, bool self = false, int nk_rows = 0) {
    switch (dec_attend_route(n_keys, rows_per_kv, n_keys_pos != nullptr, self)) {
    case DecAttn::SelfOne:
        return cbw_dec_self_attn(q, ldq, kc, vc, kv_bstride, n_keys, out, B, H, D, st, n_keys_pos, nk_rows);
    case DecAttn::Split:
        return cbw_dec_attn_split(q, ldq, kc, vc, kv_bstride, n_keys, rows_per_kv, out, B, H, D, part, st, n_keys_pos,
                                  nk_rows);
    default:
        return cbw_dec_attention(q, ldq, kc, vc, kv_bstride, n_keys, rows_per_kv, out, B, H, D, st);
    }
}
}  // namespace

extern "C" {

int cbw_decoder_create(const cbw_decoder_config* cfg, cbw_decoder** out) {
    if (!cfg || !out) return fail(CBW_ERR_INVALID, "null argument");
    if (cfg->n_heads < 1 || cfg->d_model % 128 || cfg->d_model / cfg->n_heads != 64 || cfg->ffn_dim % 128 ||
        cfg->n_layers < 1 || cfg->vocab < 2 || cfg->max_len < 1 || cfg->max_len > 448)
        return fail(CBW_ERR_INVALID, "decoder needs d_model % 128 == 0, head_dim 64, ffn_dim % 128 == 0, max_len <= 448");
    auto h = std::make_unique<cbw_decoder>();
    h->cfg = *cfg;
    h->Vpad = (cfg->vocab + 127) / 128 * 128;
    CHK(h->zero.alloc(256));
    HIPCHK(hipMemset(h->zero.p, 0, 256));
    *out = h.release();
    return CBW_OK;
}

int cbw_decoder_destroy(cbw_decoder* h) {
    delete h;
    return CBW_OK;
}

int cbw_decoder_set_param(cbw_decoder* h, const char* name, const float* host, int64_t numel) {
    if (!h) return fail(CBW_ERR_INVALID, "null handle");
    h->finalized = false;
    return h->ps.set(name, host, numel);
}

int cbw_decoder_vocab_padded(cbw_decoder* h) { return h ? h->Vpad : -1; }

int cbw_decoder_finalize(cbw_decoder* h) {
    if (!h) return fail(CBW_ERR_INVALID, "null handle");
    const int D = h->cfg.d_model, F = h->cfg.ffn_dim, V = h->cfg.vocab;
    int rc;
    {
        const auto* e = h->ps.get("embed_tokens.weight", (size_t)V * D, &rc);
        if (!e) return rc;
        std::vector<float> ep((size_t)h->Vpad * D, 0.f);
        std::copy(e->begin(), e->end(), ep.begin());
        h->emb.cin = D; h->emb.cout = h->Vpad; h->emb.k = 1;
        CHK(h->emb.w.upload(to_bf16(ep)));
        const auto* p = h->ps.get("embed_positions.weight", (size_t)448 * D, &rc);
        if (!p) return rc;
        CHK(h->pos.upload(*p));
    }
    const float qscale = 1.0f / std::sqrt(64.0f);
    h->layers.clear();
    h->layers.resize(h->cfg.n_layers);
    for (int i = 0; i < h->cfg.n_layers; ++i) {
        auto& L = h->layers[i];
        const std::string p = "layers." + std::to_string(i);
        CHK(load_xf_layer(h->ps, p, D, F, L));
        CHK(upload_ln(h->ps, p + ".encoder_attn_layer_norm", D, L.ln_x));
        CHK(upload_linear(h->ps, p + ".encoder_attn.q_proj", D, D, true, L.cq, qscale));
        CHK(upload_linear(h->ps, p + ".encoder_attn.k_proj", D, D, false, L.ck));
        CHK(upload_linear(h->ps, p + ".encoder_attn.v_proj", D, D, true, L.cv));
        CHK(upload_linear(h->ps, p + ".encoder_attn.out_proj", D, D, true, L.co));
    }
    CHK(upload_ln(h->ps, "layer_norm", D, h->lnf));
    h->finalized = true;
    return CBW_OK;
}

int64_t cbw_decoder_state_bytes(cbw_decoder* h, int B, int Benc) {
    if (!h || B <= 0 || Benc <= 0 || B % Benc) return -1;
    return dec_state_bytes(h, B, Benc);
}

}  // extern "C"
namespace {
// cross-attention K/V of `rows` encoder rows (enc_out f32 [rows][D]) into every layer's cross cache, at element
// offset `at` of the state's bf16 encoder copy and of each layer's [Benc x 1500][D] cache
int dec_cross_kv(cbw_decoder* h, const float* enc_out, size_t at, int rows, int Benc, const DecState& s,
                 hipStream_t st) {
    const int D = h->cfg.d_model;
    HIPCHK(cbw_cast_permute_lbtd(enc_out, s.enc + at, 1, 1, rows, D, st));
    const size_t per = (size_t)Benc * 1500 * D;
    const LinearRun run{rows, st, h->zero.p, false, false, nullptr};
    for (int l = 0; l < h->cfg.n_layers; ++l) {
        CHK(run.lin(h->layers[l].ck, s.enc + at, s.kc + l * per + at, nullptr, 0));
        CHK(run.lin(h->layers[l].cv, s.enc + at, s.vc + l * per + at, nullptr, 0));
    }
    return CBW_OK;
}
}  // namespace
extern "C" {

int cbw_decoder_cross_kv(cbw_decoder* h, const float* enc_out, int Benc, void* state, int64_t state_bytes, int B,
                         cbw_stream_t stream) {
    CHK(dec_check(h, enc_out && state, B, Benc));
    DecState s;
    CHK(dec_state(h, state, state_bytes, B, Benc, &s));
    return dec_cross_kv(h, enc_out, 0, Benc * 1500, Benc, s, (hipStream_t)stream);
}

int cbw_decoder_cross_kv_slot(cbw_decoder* h, const float* enc_out, int slot, int Benc, void* state,
                              int64_t state_bytes, int B, cbw_stream_t stream) {
    CHK(dec_check(h, enc_out && state, B, Benc));
    if (slot < 0 || slot >= Benc) return fail(CBW_ERR_INVALID, "cross_kv_slot needs 0 <= slot < Benc");
    DecState s;
    CHK(dec_state(h, state, state_bytes, B, Benc, &s));
    return dec_cross_kv(h, enc_out, (size_t)slot * 1500 * h->cfg.d_model, 1500, Benc, s, (hipStream_t)stream);
}

}  // extern "C"
namespace {
// one decode step; pos_dev (optional) = the position read on the device (pos is then unused): every launch
// argument is then independent of the position, so the step can be captured once and replayed.  pos_rows: pos_dev
// holds one position per row (the rows of several windows, each at its own position, in one step)
// wide (cbw_decoder_step_wide): up to CBW_DEC_WIDE_ROWS rows, the Linears as row groups of 16 on the fused GEMV
int dec_step(cbw_decoder* h, const int32_t* tokens, int pos, const int32_t* pos_dev, int B, int Benc, void* state,
             int64_t state_bytes, float* logits, cbw_stream_t stream, int pos_rows = 0, bool wide = false) {
    CHK(dec_check(h, tokens && state && logits, B, Benc));
    if (!pos_dev && (pos < 0 || pos >= h->cfg.max_len)) return fail(CBW_ERR_INVALID, "step needs 0 <= pos < max_len");
    DecState s;
    CHK(dec_state(h, state, state_bytes, B, Benc, &s));
    hipStream_t st = (hipStream_t)stream;
    const int D = h->cfg.d_model, H = h->cfg.n_heads, ML = h->cfg.max_len;
    // the step's Linears: skinny GEMV (gemv.hip) for <= 16 rows, else the implicit-GEMM tiles; LayerNorm -> Linear
    // pairs: on the GEMV the LayerNorm runs in its prologue (and the qkv projection appends K/V to the cache in its
    // epilogue), else as separate launches
    const bool gemv = dec_gemv_enabled(B, wide ? CBW_DEC_WIDE_ROWS : 16);
    LinearRun run{B, st, h->zero.p, gemv, gemv && dec_fuse_enabled() && cbw_gemv_ln_ok(wide ? 16 : B, D), s.a};
    run.wide = wide;
    run.wide_groups_fast = wide && gemv_wide_groups_fast();
    if (pos_dev && !run.fuse)
        return fail(CBW_ERR_INVALID, "device-position steps need the fused GEMV path (<= 16 rows, CBW_DEC_GEMV / "
                                     "CBW_DEC_FUSE on)");
    HIPCHK(cbw_dec_embed(tokens, h->emb.w.as<uint16_t>(), h->pos.as<float>(), pos, s.h, B, D, st, 0, pos_dev, pos_rows));
    const size_t self_per = (size_t)B * ML * D, cross_per = (size_t)Benc * 1500 * D;
    for (int l = 0; l < h->cfg.n_layers; ++l) {
        auto& L = h->layers[l];
        uint16_t* kl = s.ks + l * self_per;
        uint16_t* vl = s.vs + l * self_per;
        const KvAppend kv{kl, vl, (int64_t)ML * D, D, pos, pos_dev, pos_rows};
        CHK(attn_block(run, L.ln1, L.qkv, L.out, s.h, s.qkv, s.att, kv, [&]() -> int {
            HIPCHK(dec_attend(s.apart, s.qkv, 3 * D, kl, vl, (int64_t)ML * D, pos_dev ? ML : pos + 1, 1, s.att, B, H, D,
                              st, pos_dev, true, pos_rows));
            return CBW_OK;
        }));
        CHK(attn_block(run, L.ln_x, L.cq, L.co, s.h, s.qc, s.att, {}, [&]() -> int {
            HIPCHK(dec_attend(s.apart, s.qc, D, s.kc + l * cross_per, s.vc + l * cross_per, (int64_t)1500 * D,
                              1500, B / Benc, s.att, B, H, D, st));
            return CBW_OK;
        }));
        CHK(mlp_block(run, L, s.h, s.f));
    }
    // the final LayerNorm and the tied vocabulary projection
    return run.ln_lin(s.h, h->lnf, h->emb, logits, CBW_EPI_OUT_F32);
}

}  // namespace
extern "C" {

int cbw_decoder_step(cbw_decoder* h, const int32_t* tokens, int pos, int B, int Benc, void* state, int64_t state_bytes,
                     float* logits, cbw_stream_t stream) {
    return dec_step(h, tokens, pos, nullptr, B, Benc, state, state_bytes, logits, stream);
}

int cbw_decoder_step_dev(cbw_decoder* h, const int32_t* tokens, const int32_t* pos_dev, int B, int Benc, void* state,
                         int64_t state_bytes, float* logits, cbw_stream_t stream) {
    if (!pos_dev) return fail(CBW_ERR_INVALID, "null pos_dev");
    return dec_step(h, tokens, 0, pos_dev, B, Benc, state, state_bytes, logits, stream);
}

int cbw_decoder_step_rows(cbw_decoder* h, const int32_t* tokens, const int32_t* pos_rows, int B, int Benc, void* state,
                          int64_t state_bytes, float* logits, cbw_stream_t stream) {
    if (!pos_rows) return fail(CBW_ERR_INVALID, "null pos_rows");
    return dec_step(h, tokens, 0, pos_rows, B, Benc, state, state_bytes, logits, stream, 1);
}

int cbw_decoder_step_wide(cbw_decoder* h, const int32_t* tokens, const int32_t* pos_rows, int B, int Benc, void* state,
                          int64_t state_bytes, float* logits, cbw_stream_t stream) {
    if (!pos_rows) return fail(CBW_ERR_INVALID, "null pos_rows");
    if (B > CBW_DEC_WIDE_ROWS) return fail(CBW_ERR_INVALID, "cbw_decoder_step_wide: at most 80 rows");
    // the split cross-attention reads a window's K/V once for its rows: at most 8 rows per encoder slot
    if (B > 0 && Benc > 0 && B % Benc == 0 && B / Benc > 8)
        return fail(CBW_ERR_INVALID, "cbw_decoder_step_wide: at most 8 rows per encoder slot");
    return dec_step(h, tokens, 0, pos_rows, B, Benc, state, state_bytes, logits, stream, 1, true);
}

int cbw_decoder_prefill(cbw_decoder* h, const int32_t* tokens, int T, int B, int Benc, void* state,
                        int64_t state_bytes, float* logits, cbw_stream_t stream) {
    if (Benc != 1) return fail(CBW_ERR_INVALID, "prefill needs Benc == 1 (cbw_decoder_prefill_rows: one window of several)");
    return cbw_decoder_prefill_rows(h, tokens, T, 0, 0, B, B, Benc, state, state_bytes, logits, stream);
}

}  // extern "C"

namespace {
// The prefill layers: the T prefix tokens as T rows at positions 0..T-1 (the beams are identical through a forced
// prefix: one row set), their K/V replicated into cache rows [r0, r0 + nb), which attend to encoder slot `slot`; s.ph
// ends as the last layer's residual stream.  probes (n_probe > 0): right after layer l's cross-attention query, the
// probabilities of each listed (layer, head) pair of that layer -> probs[i] [T][1500].
int dec_prefill_layers(cbw_decoder* h, const int32_t* tokens, int T, int slot, int r0, int nb, int B, int Benc,
                       const DecState& s, hipStream_t st, const int32_t* probe = nullptr, int n_probe = 0,
                       float* probs = nullptr) {
    const int D = h->cfg.d_model, H = h->cfg.n_heads, ML = h->cfg.max_len;
    const LinearRun run{T, st, h->zero.p, false, false, s.pa};
    HIPCHK(cbw_dec_embed(tokens, h->emb.w.as<uint16_t>(), h->pos.as<float>(), 0, s.ph, T, D, st, 1));
    const size_t self_per = (size_t)B * ML * D, cross_per = (size_t)Benc * 1500 * D;
    for (int l = 0; l < h->cfg.n_layers; ++l) {
        auto& L = h->layers[l];
        uint16_t* kl = s.ks + l * self_per + (size_t)r0 * ML * D;
        uint16_t* vl = s.vs + l * self_per + (size_t)r0 * ML * D;
        const uint16_t* kx = s.kc + l * cross_per + (size_t)slot * 1500 * D;
        const uint16_t* vx = s.vc + l * cross_per + (size_t)slot * 1500 * D;
        CHK(attn_block(run, L.ln1, L.qkv, L.out, s.ph, s.pqkv, s.patt, {}, [&]() -> int {
            HIPCHK(cbw_dec_kv_prefill(s.pqkv, kl, vl, T, nb, D, ML, st));
            HIPCHK(cbw_dec_attention(s.pqkv, 3 * D, kl, vl, (int64_t)ML * D, T, T, s.patt, T, H, D, st, 1));
            return CBW_OK;
        }));
        CHK(attn_block(run, L.ln_x, L.cq, L.co, s.ph, s.pqc, s.patt, {}, [&]() -> int {
            for (int i = 0; i < n_probe; ++i)
                if (probe[2 * i] == l)
                    HIPCHK(cbw_dec_cross_probs(s.pqc, D, kx, 1500, T, D, probe[2 * i + 1], probs + (size_t)i * T * 1500,
                                               st));
            HIPCHK(cbw_dec_attention(s.pqc, D, kx, vx, (int64_t)1500 * D, 1500, T, s.patt, T, H, D, st));
            return CBW_OK;
        }));
        CHK(mlp_block(run, L, s.ph, s.pf));
    }
    return CBW_OK;
}
}  // namespace

extern "C" {

int cbw_decoder_prefill_rows(cbw_decoder* h, const int32_t* tokens, int T, int slot, int r0, int nb, int B, int Benc,
                             void* state, int64_t state_bytes, float* logits, cbw_stream_t stream) {
    CHK(dec_check(h, tokens && state && logits, B, Benc));
    if (T < 1 || T > h->cfg.max_len || slot < 0 || slot >= Benc || nb < 1 || r0 < 0 || r0 + nb > B)
        return fail(CBW_ERR_INVALID, "prefill needs 1 <= T <= max_len, 0 <= slot < Benc, rows [r0, r0 + nb) within B");
    DecState s;
    CHK(dec_state(h, state, state_bytes, B, Benc, &s));
    hipStream_t st = (hipStream_t)stream;
    CHK(dec_prefill_layers(h, tokens, T, slot, r0, nb, B, Benc, s, st));
    // logits of the last prefix token only: one row, its vocabulary projection on the same kernel as the step's
    // (a state of more than 16 rows is stepped by cbw_decoder_step_wide, on the GEMV as well)
    const LinearRun last{1, st, h->zero.p, dec_gemv_enabled(B, CBW_DEC_WIDE_ROWS), false, s.pa};
    return last.ln_lin(s.ph + (size_t)(T - 1) * h->cfg.d_model, h->lnf, h->emb, logits, CBW_EPI_OUT_F32);
}

}  // extern "C"
namespace {
// cbw_decoder_cross_attn_probs and its slot-taking form: the checks, then the probed prefill of slot `slot`, row r0
int dec_cross_attn_probs(const std::string& who, cbw_decoder* h, const int32_t* tokens, int T, const int32_t* heads,
                         int n, int slot, int r0, int B, int Benc, void* state, int64_t state_bytes, float* probs,
                         cbw_stream_t stream) {
    CHK(dec_check(h, tokens && heads && state && probs, B, Benc));
    if (T < 1 || T > h->cfg.max_len || n < 1) return fail(CBW_ERR_INVALID, who + " needs 1 <= T <= max_len, n >= 1");
    if (h->cfg.d_model != 64 * h->cfg.n_heads) return fail(CBW_ERR_INVALID, who + ": head dim must be 64");
    for (int i = 0; i < n; ++i)
        if (heads[2 * i] < 0 || heads[2 * i] >= h->cfg.n_layers || heads[2 * i + 1] < 0 ||
            heads[2 * i + 1] >= h->cfg.n_heads)
            return fail(CBW_ERR_INVALID, who + ": (layer, head) out of range");
    if (slot < 0 || slot >= Benc || r0 < 0 || r0 >= B)
        return fail(CBW_ERR_INVALID, who + " needs 0 <= slot < Benc, 0 <= r0 < B");
    DecState s;
    CHK(dec_state(h, state, state_bytes, B, Benc, &s));
    return dec_prefill_layers(h, tokens, T, slot, r0, 1, B, Benc, s, (hipStream_t)stream, heads, n, probs);
}
}  // namespace
extern "C" {

int cbw_decoder_cross_attn_probs(cbw_decoder* h, const int32_t* tokens, int T, const int32_t* heads, int n, int B,
                                 int Benc, void* state, int64_t state_bytes, float* probs, cbw_stream_t stream) {
    return dec_cross_attn_probs("cross_attn_probs", h, tokens, T, heads, n, 0, 0, B, Benc, state, state_bytes, probs,
                                stream);
}

int cbw_decoder_cross_attn_probs_slot(cbw_decoder* h, const int32_t* tokens, int T, const int32_t* heads, int n,
                                      int slot, int r0, int B, int Benc, void* state, int64_t state_bytes,
                                      float* probs, cbw_stream_t stream) {
    if (!h || !tokens || !heads || !state || !probs)
        return fail(CBW_ERR_INVALID, "cbw_decoder_cross_attn_probs_slot: null argument");
    return dec_cross_attn_probs("cbw_decoder_cross_attn_probs_slot", h, tokens, T, heads, n, slot, r0, B, Benc, state,
                                state_bytes, probs, stream);
}

int cbw_dtw(const double* matrix, int rows, int cols, int32_t* text_idx, int32_t* time_idx, int* len) {
    if (!matrix || !text_idx || !time_idx || !len || rows < 1 || cols < 1) return fail(CBW_ERR_INVALID, "cbw_dtw: bad arguments");
    // transformers' _dynamic_time_warping, step for step: float32 cost and trace tables, each cost the f64 matrix entry
    // plus the chosen f32 predecessor rounded to f32 (numpy's float64 + float32 stored into a float32 array); strict
    // comparisons pick the diagonal, then the row above, else the column to the left
    const int R = rows + 1, C = cols + 1;
    std::vector<float> cost((size_t)R * C, std::numeric_limits<float>::infinity()), trace((size_t)R * C, -1.f);
    cost[0] = 0.f;
    for (int j = 1; j < C; ++j)
        for (int i = 1; i < R; ++i) {
            const float c0 = cost[(size_t)(i - 1) * C + j - 1], c1 = cost[(size_t)(i - 1) * C + j],
                        c2 = cost[(size_t)i * C + j - 1];
            float c, t;
            if (c0 < c1 && c0 < c2) c = c0, t = 0.f;
            else if (c1 < c0 && c1 < c2) c = c1, t = 1.f;
            else c = c2, t = 2.f;
            cost[(size_t)i * C + j] = (float)(matrix[(size_t)(i - 1) * cols + j - 1] + (double)c);
            trace[(size_t)i * C + j] = t;
        }
    for (int j = 0; j < C; ++j) trace[j] = 2.f;
    for (int i = 0; i < R; ++i) trace[(size_t)i * C] = 1.f;
    int i = rows, j = cols, n = 0;
    while (i > 0 || j > 0) {
        text_idx[n] = i - 1;
        time_idx[n] = j - 1;
        ++n;
        const float t = trace[(size_t)i * C + j];
        if (t == 0.f) --i, --j;
        else if (t == 1.f) --i;
        else if (t == 2.f) --j;
        else return fail(CBW_ERR_STATE, "cbw_dtw: unexpected trace entry");
    }
    std::reverse(text_idx, text_idx + n);
    std::reverse(time_idx, time_idx + n);
    *len = n;
    return CBW_OK;
}

// The device statement of what follows the weights in _extract_token_timestamps: no allocation, no synchronisation.
int64_t cbw_token_ts_ws_bytes(int T, int F) {
    if (T < 1 || T > 1024 || F < 1 || F > CBW_DTW_MAX_F)
        return fail(CBW_ERR_INVALID, "cbw_token_ts_ws_bytes needs 1 <= T <= 1024, 1 <= F <= 1500");
    return cbw_dtw_trace_words(T, F) * (int64_t)sizeof(uint32_t);
}

namespace {
static int token_ts_ws_check(const char* who, int T, int F, const void* ws, int64_t ws_bytes) {
    if (!ws || ((uintptr_t)ws & 3) || ws_bytes < cbw_dtw_trace_words(T, F) * (int64_t)sizeof(uint32_t))
        return fail(CBW_ERR_INVALID, std::string(who) + ": ws null, misaligned or smaller than cbw_token_ts_ws_bytes");
    return CBW_OK;
}
}  // namespace

int cbw_align_matrix(const float* probs, int n, int T_all, int t0, int T, int F, int width, float* matrix,
                     int32_t* degenerate, void* ws, int64_t ws_bytes, cbw_stream_t stream) {
    if (!probs || !matrix || !degenerate) return fail(CBW_ERR_INVALID, "cbw_align_matrix: null probs, matrix or degenerate");
    if (n < 1) return fail(CBW_ERR_INVALID, "cbw_align_matrix: n < 1");
    if (T < 2 || T > 1024) return fail(CBW_ERR_INVALID, "cbw_align_matrix needs 2 <= T <= 1024");
    if (t0 < 0 || T_all < T || t0 > T_all - T) return fail(CBW_ERR_INVALID, "cbw_align_matrix: [t0, t0 + T) outside [0, T_all)");
    if (F < 1 || F > 1500) return fail(CBW_ERR_INVALID, "cbw_align_matrix needs 1 <= F <= 1500");
    if (width < 1 || width > 7 || !(width & 1)) return fail(CBW_ERR_INVALID, "cbw_align_matrix: width must be 1, 3, 5 or 7");
    CHK(token_ts_ws_check("cbw_align_matrix", T, F, ws, ws_bytes));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(degenerate, 0, sizeof(int32_t), st));
    HIPCHK(cbw_align_matrix_launch(probs, n, T_all, t0, T, F, width, matrix, degenerate, st));
    return CBW_OK;
}

int cbw_dtw_dev(const float* matrix, int T, int F, int32_t* first_frame, int32_t* text_idx, int32_t* time_idx,
                int32_t* len, void* ws, int64_t ws_bytes, cbw_stream_t stream) {
    if (!matrix || !first_frame) return fail(CBW_ERR_INVALID, "cbw_dtw_dev: null matrix or first_frame");
    if (!!text_idx != !!time_idx || !!text_idx != !!len)
        return fail(CBW_ERR_INVALID, "cbw_dtw_dev: text_idx, time_idx and len are all null or all set");
    if (T < 1 || T > 1024) return fail(CBW_ERR_INVALID, "cbw_dtw_dev needs 1 <= T <= 1024");
    if (F < 1 || F > CBW_DTW_MAX_F) return fail(CBW_ERR_INVALID, "cbw_dtw_dev needs 1 <= F <= 1500");
    CHK(token_ts_ws_check("cbw_dtw_dev", T, F, ws, ws_bytes));
    HIPCHK(cbw_dtw_launch(matrix, T, F, first_frame, text_idx, time_idx, len, (uint32_t*)ws, (hipStream_t)stream));
    return CBW_OK;
}

}  // extern "C"
namespace {
// the checks of the batched entries, per window, and the table the kernels take: base pointers plus offsets
int token_ts_batch(const std::string& who, const cbw_token_ts_window* win, int N, int min_T, const float* probs,
                   float* matrix, void* ws, int64_t ws_bytes, cbw_ts_batch* out) {
    if (!win) return fail(CBW_ERR_INVALID, who + ": null win");
    if (N < 1 || N > CBW_TOKEN_TS_MAX_WINDOWS) return fail(CBW_ERR_INVALID, who + " needs 1 <= N <= 16 windows");
    if (ws_bytes >= 0 && (!ws || ((uintptr_t)ws & 3))) return fail(CBW_ERR_INVALID, who + ": ws null or misaligned");
    for (int i = 0; i < N; ++i) {
        const cbw_token_ts_window& w = win[i];
        const std::string at = who + ": window " + std::to_string(i);
        if (w.T < min_T || w.T > 1024) return fail(CBW_ERR_INVALID, at + " needs " + std::to_string(min_T) + " <= T <= 1024");
        if (w.t0 < 0 || w.T_all < w.T || w.t0 > w.T_all - w.T)
            return fail(CBW_ERR_INVALID, at + ": [t0, t0 + T) outside [0, T_all)");
        if (w.F < 1 || w.F > CBW_DTW_MAX_F) return fail(CBW_ERR_INVALID, at + " needs 1 <= F <= 1500");
        if (w.probs_off < 0 || w.matrix_off < 0 || w.ws_off < 0 || (w.ws_off & 3))
            return fail(CBW_ERR_INVALID, at + ": an offset is negative, or ws_off no multiple of 4");
        const int64_t need = cbw_dtw_trace_words(w.T, w.F) * (int64_t)sizeof(uint32_t);
        if (ws_bytes >= 0 && (need > ws_bytes || w.ws_off > ws_bytes - need))
            return fail(CBW_ERR_INVALID, at + ": ws smaller than ws_off + cbw_token_ts_ws_bytes");
        if (out) out->w[i] = {probs + w.probs_off, matrix + w.matrix_off, (uint32_t*)((char*)ws + w.ws_off), w.T_all,
                              w.t0, w.T, w.F};
    }
    return CBW_OK;
}
}  // namespace
extern "C" {

int64_t cbw_token_ts_ws_bytes_batch(const cbw_token_ts_window* win, int N) {
    CHK(token_ts_batch("cbw_token_ts_ws_bytes_batch", win, N, 1, nullptr, nullptr, nullptr, -1, nullptr));
    int64_t sum = 0;
    for (int i = 0; i < N; ++i) sum += cbw_dtw_trace_words(win[i].T, win[i].F) * (int64_t)sizeof(uint32_t);
    return sum;
}

int cbw_align_matrix_batch(const float* probs, int n, const cbw_token_ts_window* win, int N, int width, float* matrix,
                           int32_t* degenerate, void* ws, int64_t ws_bytes, cbw_stream_t stream) {
    const char* who = "cbw_align_matrix_batch";
    if (!probs || !matrix || !degenerate) return fail(CBW_ERR_INVALID, std::string(who) + ": null probs, matrix or degenerate");
    if (n < 1) return fail(CBW_ERR_INVALID, std::string(who) + ": n < 1");
    if (width < 1 || width > 7 || !(width & 1)) return fail(CBW_ERR_INVALID, std::string(who) + ": width must be 1, 3, 5 or 7");
    cbw_ts_batch b{};
    CHK(token_ts_batch(who, win, N, 2, probs, matrix, ws, ws_bytes < 0 ? 0 : ws_bytes, &b));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(degenerate, 0, N * sizeof(int32_t), st));
    HIPCHK(cbw_align_matrix_batch_launch(b, N, n, width, degenerate, st));
    return CBW_OK;
}

int cbw_dtw_dev_batch(const float* matrix, const cbw_token_ts_window* win, int N, int32_t* first_frame, int ld,
                      void* ws, int64_t ws_bytes, cbw_stream_t stream) {
    const char* who = "cbw_dtw_dev_batch";
    if (!matrix || !first_frame) return fail(CBW_ERR_INVALID, std::string(who) + ": null matrix or first_frame");
    cbw_ts_batch b{};
    // the matrices are read here; the table's probs entries are not used by the DTW
    CHK(token_ts_batch(who, win, N, 1, nullptr, const_cast<float*>(matrix), ws, ws_bytes < 0 ? 0 : ws_bytes, &b));
    for (int i = 0; i < N; ++i)
        if (ld < win[i].T) return fail(CBW_ERR_INVALID, std::string(who) + ": ld below the largest T");
    HIPCHK(cbw_dtw_batch_launch(b, N, first_frame, ld, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_decoder_reorder(cbw_decoder* h, const int32_t* src_rows, int B, int Benc, int len, void* state,
                        int64_t state_bytes, cbw_stream_t stream) {
    if (!h || !src_rows || !state) return fail(CBW_ERR_INVALID, "null argument");
    if (B <= 0 || Benc <= 0 || B % Benc || len < 0 || len > h->cfg.max_len) return fail(CBW_ERR_INVALID, "bad arguments");
    DecState s;
    CHK(dec_state(h, state, state_bytes, B, Benc, &s));
    if (len == 0) return CBW_OK;
    hipStream_t st = (hipStream_t)stream;
    const int D = h->cfg.d_model, ML = h->cfg.max_len;
    const size_t self_per = (size_t)B * ML * D;
    if (B <= 16) {   // every layer's K and V in one in-place launch
        HIPCHK(cbw_dec_reorder_kv(s.ks, s.vs, src_rows, B, h->cfg.n_layers, (int64_t)self_per, (int64_t)ML * D,
                                  (int64_t)len * D, st));
        return CBW_OK;
    }
    for (int l = 0; l < h->cfg.n_layers; ++l) {
        for (uint16_t* cache : {s.ks + l * self_per, s.vs + l * self_per}) {
            HIPCHK(cbw_dec_gather_rows(cache, s.scratch, src_rows, B, (int64_t)ML * D, (int64_t)len * D, st));
            HIPCHK(hipMemcpy2DAsync(cache, (size_t)ML * D * 2, s.scratch, (size_t)ML * D * 2, (size_t)len * D * 2, B,
                                    hipMemcpyDeviceToDevice, st));
        }
    }
    return CBW_OK;
}

int cbw_logprob_topk(const float* logits, int B, int V, int ld, const float* bias, int64_t bias_ld, int k, float* lp,
                     int32_t* idx, cbw_stream_t stream) {
    if (!logits || !lp || !idx || B <= 0 || V <= 0 || ld < V || k < 1 || k > 16 || bias_ld < 0)
        return fail(CBW_ERR_INVALID, "bad arguments (k must be in [1, 16])");
    HIPCHK(cbw_logprob_topk_launch(logits, B, V, ld, bias, bias_ld, k, lp, idx, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_beam_select(const float* lp, const int32_t* idx, int B, int k, int eos, double* beam_scores,
                    double* cand_score, int32_t* cand_row, int32_t* cand_tok, int32_t* tokens, int32_t* parents,
                    int32_t* ok, int32_t* ts_state, int32_t* st_out, int timestamp_begin, int count,
                    cbw_stream_t stream) {
    if (!lp || !idx || !beam_scores || !cand_score || !cand_row || !cand_tok || !tokens || !parents || !ok || !ts_state ||
        !st_out || B < 1 || B > 16 || k < 1 || k > 16)
        return fail(CBW_ERR_INVALID, "bad arguments (B and k in [1, 16])");
    HIPCHK(cbw_beam_select_launch(lp, idx, B, k, eos, beam_scores, cand_score, cand_row, cand_tok, tokens, parents, ok,
                                  ts_state, st_out, timestamp_begin, count, (hipStream_t)stream));
    return CBW_OK;
}
int cbw_timestamp_rules(const float* logits, int B, int V, int ld, const float* bias, const int32_t* state,
                        int timestamp_begin, int no_timestamps, int eos, int max_initial, float* bias_out,
                        cbw_stream_t stream) {
    if (!logits || !state || !bias_out || B <= 0 || V <= 0 || ld < V || timestamp_begin <= 0 ||
        timestamp_begin >= V || eos < 0 || eos >= V || no_timestamps < 0 || no_timestamps >= V)
        return fail(CBW_ERR_INVALID, "bad arguments");
    HIPCHK(cbw_timestamp_rules_launch(logits, B, V, ld, bias, state, timestamp_begin, no_timestamps, eos, max_initial,
                                      bias_out, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_greedy_select(const float* logits, int B, int V, int ld, const float* bias, const float* bias_begin,
                      int timestamp_begin, int no_timestamps, int eos, int max_initial, int32_t* ts_state,
                      const int32_t* pos_rows, const int32_t* limit, int32_t* active, int32_t* tokens, float* logprob,
                      cbw_stream_t stream) {
    if (!logits || !ts_state || !pos_rows || !limit || !active || !tokens || !logprob || B < 1 || B > 16 || V < 1 ||
        ld < V)
        return fail(CBW_ERR_INVALID, "bad arguments (B in [1, 16], ld >= V >= 1)");
    HIPCHK(cbw_greedy_select_launch(logits, B, V, ld, bias, bias_begin, timestamp_begin, no_timestamps, eos,
                                    max_initial, ts_state, pos_rows, limit, active, tokens, logprob,
                                    (hipStream_t)stream));
    return CBW_OK;
}

int cbw_sample_select(const float* logits, int B, int V, int ld, const float* bias, const float* bias_begin,
                      int timestamp_begin, int no_timestamps, int eos, int max_initial, int32_t* ts_state,
                      const int32_t* pos_rows, const int32_t* limit, int32_t* active, int32_t* tokens, float* logprob,
                      float temperature, int top_k, const float* noise, int64_t noise_ld, cbw_stream_t stream) {
    if (!logits || !ts_state || !pos_rows || !limit || !active || !tokens || !logprob || !noise || B < 1 || B > 16 ||
        V < 1 || V > CBW_SAMPLE_MAX_V || ld < V || noise_ld < V)
        return fail(CBW_ERR_INVALID, "bad arguments (B in [1, 16], V in [1, 52224], ld >= V, noise_ld >= V)");
    if (!(temperature > 0.f) || !std::isfinite(temperature) || top_k < 1)
        return fail(CBW_ERR_INVALID, "bad arguments (temperature > 0 and finite, top_k >= 1)");
    HIPCHK(cbw_sample_select_launch(logits, B, V, ld, bias, bias_begin, timestamp_begin, no_timestamps, eos,
                                    max_initial, ts_state, pos_rows, limit, active, tokens, logprob, temperature, top_k,
                                    noise, noise_ld, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_history_rules(float* logits, int B, int V, int ld, int32_t* hist, int hist_ld, int32_t* hist_len,
                      const int32_t* last_tokens, const int32_t* pos_rows, const int32_t* active,
                      float repetition_penalty, int no_repeat_ngram_size, cbw_stream_t stream) {
    if (!logits || !hist || !hist_len || !pos_rows || !active || B < 1 || B > 16 || V < 1 || ld < V || hist_ld < 1 ||
        hist_ld > CBW_HISTORY_MAX_LD)
        return fail(CBW_ERR_INVALID, "bad arguments (B in [1, 16], ld >= V >= 1, hist_ld in [1, 2048])");
    if (!(repetition_penalty > 0.f) || !std::isfinite(repetition_penalty) || no_repeat_ngram_size < 0)
        return fail(CBW_ERR_INVALID, "bad arguments (repetition_penalty > 0 and finite, no_repeat_ngram_size >= 0)");
    HIPCHK(cbw_history_rules_launch(logits, B, V, ld, hist, hist_ld, hist_len, last_tokens, pos_rows, active,
                                    repetition_penalty, no_repeat_ngram_size, (hipStream_t)stream));
    return CBW_OK;
}

// ------------------------------------------------------------------ building block
}  // extern "C"
namespace {
// 256 zero bytes per device (padding taps / rows past M of the building-block convs)
int block_zero_page(const void** out) {
    static thread_local std::map<int, std::shared_ptr<DevBuf>> zeros;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    auto it = zeros.find(dev);
    if (it == zeros.end()) {
        auto z = std::make_shared<DevBuf>();
        CHK(z->alloc(256));
        HIPCHK(hipMemset(z->p, 0, 256));
        it = zeros.emplace(dev, z).first;
    }
    *out = it->second->p;
    return CBW_OK;
}
}  // namespace
extern "C" {
int cbw_conv2d(const uint16_t* x, const uint16_t* w, const float* bias, const void* res, void* y, int N, int H, int W,
               int Cin, int Cout, int KH, int KW, int sh, int sw, int ph, int pw, int flags, cbw_stream_t stream) {
    if (!x || !w || !y || Cin % 64 || Cout % 64) return fail(CBW_ERR_INVALID, "cbw_conv2d: Cin and Cout must be multiples of 64");
    if (!((KH == 1 && KW == 1) || (KH == 3 && KW == 3) || (KH == 1 && KW == 3)))
        return fail(CBW_ERR_INVALID, "cbw_conv2d: kernel must be 1x1, 3x3 or 1x3");
    const void* zp = nullptr;
    CHK(block_zero_page(&zp));
    ConvArgs a{};
    a.x = x; a.w = w; a.bias = bias; a.res = res; a.y = y; a.zero = zp;
    conv_geometry(a, N, H, W, Cin, Cout, KH, KW, sh, sw, ph, pw);
    a.res_ld = a.y_ld = Cout;
    a.flags = flags;
    HIPCHK(cbw_conv_igemm(a, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_conv1x1_chain(const uint16_t* x, const uint16_t* we, const float* be, const uint16_t* res, const uint16_t* wr,
                      const float* br, uint16_t* y, uint16_t* t1, int N, int H, int W, cbw_stream_t stream) {
    if (!x || !we || !be || !res || !wr || !br || !y || !t1 || N <= 0 || H <= 0 || W <= 0)
        return fail(CBW_ERR_INVALID, "cbw_conv1x1_chain: bad argument");
    const void* zp = nullptr;
    CHK(block_zero_page(&zp));
    ConvArgs a{};
    a.x = x; a.w = we; a.bias = be; a.res = res; a.y = y; a.zero = zp;
    conv_geometry(a, N, H, W, 128, 512, 1, 1, 1, 1, 0, 0);
    a.res_ld = a.y_ld = 512;
    a.flags = CBW_EPI_RELU;
    if (!cbw_conv_chain_supported(a, 128)) return fail(CBW_ERR_INVALID, "cbw_conv1x1_chain: shape not supported");
    DevBuf packed;   // a handle packs once at finalize; here per call, freed after the launch has finished
    CHK(packed.alloc((size_t)128 * 512 * 2));
    HIPCHK(cbw_conv_chain_pack(wr, packed.as<uint16_t>(), (hipStream_t)stream));
    HIPCHK(cbw_conv_chain(a, packed.as<uint16_t>(), br, t1, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return CBW_OK;
}

int cbw_gemm_splitk_factor(int M, int K, int N) {
    if (M <= 0 || K <= 0 || N <= 0) return fail(CBW_ERR_INVALID, "cbw_gemm_splitk_factor: bad shape");
    return cbw_conv_splitk_factor(linear_args(M, K, N));
}

int cbw_encoder_attention(const uint16_t* qkv, uint16_t* out, int B, int T, int H, cbw_stream_t stream) {
    if (!qkv || !out || B <= 0 || T <= 0 || H <= 0) return fail(CBW_ERR_INVALID, "cbw_encoder_attention: bad argument");
    HIPCHK(cbw_attention(qkv, out, B, T, H, 64, (hipStream_t)stream));
    return CBW_OK;
}

int64_t cbw_decode_attention_ws_floats(int B, int H) {
    if (B <= 0 || H <= 0 || (int64_t)B * H > INT32_MAX / cbw_dec_attn_split_floats(1, 1))
        return fail(CBW_ERR_INVALID, "cbw_decode_attention_ws_floats: bad shape");
    return cbw_dec_attn_split_floats(B, H);
}

int cbw_decode_attention(const uint16_t* q, int ldq, const uint16_t* k, const uint16_t* v, int64_t kv_bstride,
                         int n_keys, int rows_per_kv, const int32_t* n_keys_pos, int nk_rows, int causal, int path,
                         uint16_t* out, int B, int H, int D, float* ws, int64_t ws_floats, cbw_stream_t stream) {
    auto bad = [](const char* why) { return fail(CBW_ERR_INVALID, std::string("cbw_decode_attention: ") + why); };
    if (!q || !k || !v || !out) return bad("null operand");
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) return bad("q, k, v must be 16-byte aligned");
    if (path < 0 || path > 4) return bad("path must be 0..4");
    if (B <= 0 || H <= 0) return bad("B, H must be positive");
    if ((int64_t)H * 64 > D || D % 8) return bad("D must be a multiple of 8 and at least 64 H");
    if (ldq % 8 || ldq < H * 64) return bad("ldq must be a multiple of 8 and at least 64 H");
    if (n_keys < 1 || n_keys > (path == 4 ? 448 : 1536)) return bad("n_keys must be 1..1536 (1..448 on path 4)");
    if (kv_bstride % 8 || kv_bstride < (int64_t)n_keys * D)
        return bad("kv_bstride must be a multiple of 8 and at least n_keys D");
    if (rows_per_kv < 1 || B % rows_per_kv) return bad("rows_per_kv must be positive and divide B");
    if (path == 4 && rows_per_kv != 1) return bad("path 4 needs rows_per_kv == 1");
    if (causal && path != 2) return bad("causal needs path 2");
    if (n_keys_pos && path == 2) return bad("path 2 takes no device key counts");
    const bool routed = path < 2;   // paths 0 and 1: the step's routing decides, self-attention on path 0
    const bool split = path == 3 || (routed && dec_attend_route(n_keys, rows_per_kv, n_keys_pos != nullptr, path == 0) ==
                                                   DecAttn::Split);
    if (split && rows_per_kv > 8) return bad("the split kernel serves at most 8 rows per K/V batch");
    if (split) {
        const int64_t need = cbw_decode_attention_ws_floats(B, H);
        if (need < 0) return bad("B H too large for the split kernel's partials");
        if (!ws || ws_floats < need) return bad("ws null or too small");
    }
    hipStream_t st = (hipStream_t)stream;
    switch (path) {
    case 2:
        HIPCHK(cbw_dec_attention(q, ldq, k, v, kv_bstride, n_keys, rows_per_kv, out, B, H, D, st, causal != 0));
        break;
    case 3:
        HIPCHK(cbw_dec_attn_split(q, ldq, k, v, kv_bstride, n_keys, rows_per_kv, out, B, H, D, ws, st, n_keys_pos,
                                  nk_rows != 0));
        break;
    case 4:
        HIPCHK(cbw_dec_self_attn(q, ldq, k, v, kv_bstride, n_keys, out, B, H, D, st, n_keys_pos, nk_rows != 0));
        break;
    default:
        HIPCHK(dec_attend(ws, q, ldq, k, v, kv_bstride, n_keys, rows_per_kv, out, B, H, D, st, n_keys_pos, path == 0,
                          nk_rows != 0));
    }
    return CBW_OK;
}

int cbw_decode_cross_probs(const uint16_t* q, int ldq, const uint16_t* k, int n_keys, int T, int D, int head,
                           float* out, cbw_stream_t stream) {
    if (!q || !k || !out || ((uintptr_t)k & 15))
        return fail(CBW_ERR_INVALID, "cbw_decode_cross_probs: null operand or k not 16-byte aligned");
    if (n_keys < 1 || n_keys > 1536 || T <= 0 || head < 0 || D % 8 || (int64_t)(head + 1) * 64 > D ||
        (int64_t)(head + 1) * 64 > ldq)
        return fail(CBW_ERR_INVALID,
                    "cbw_decode_cross_probs: 1 <= n_keys <= 1536, T >= 1, D % 8, 64 (head + 1) <= D, ldq");
    HIPCHK(cbw_dec_cross_probs(q, ldq, k, n_keys, T, D, head, out, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_gemm(const uint16_t* x, const uint16_t* w, const float* bias, const void* res, void* y, int M, int K, int N,
             int flags, int ksplit, float* partial, int64_t partial_floats, cbw_stream_t stream) {
    if (!x || !w || !y || M <= 0 || K % 64 || N % 64 || ksplit < 0)
        return fail(CBW_ERR_INVALID, "cbw_gemm: K and N must be multiples of 64");
    const void* zp = nullptr;
    CHK(block_zero_page(&zp));
    ConvArgs a = linear_args(M, K, N);
    a.x = x; a.w = w; a.bias = bias; a.res = res; a.y = y; a.zero = zp;
    a.flags = flags;
    const int S = ksplit == 0 ? cbw_conv_splitk_factor(a) : ksplit;
    if (S > 1) {
        if (!partial || partial_floats < (int64_t)S * M * N) return fail(CBW_ERR_OOM, "cbw_gemm: partial buffer too small");
        if (N % 128 || S > K / 64) return fail(CBW_ERR_INVALID, "cbw_gemm: split-K needs N % 128 == 0 and S <= K / 64");
    }
    HIPCHK(cbw_conv_igemm_splitk(a, S, partial, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_linear_rows(const uint16_t* x, const float* xf, int ldx, const float* ln_g, const float* ln_b, float ln_eps,
                    const uint16_t* w, const float* bias, const void* res, int res_ld, void* y, int ldy, int M, int N,
                    int K, int flags, uint16_t* kv_k, uint16_t* kv_v, int64_t kv_ld, int kv_D, const int32_t* kv_pos,
                    int kv_pos_rows, cbw_stream_t stream) {
    if ((!x && !xf) || !w || !y) return fail(CBW_ERR_INVALID, "cbw_linear_rows: null operand");
    if (M < 1 || M > 16 || N < 4 || N % 4 || K < 32 || K % 32 || ldx % 8 || ldy % 4 || ldx < K || ldy < N ||
        (res && (res_ld % 4 || res_ld < N)))
        return fail(CBW_ERR_INVALID, "cbw_linear_rows: 1 <= M <= 16, K % 32, N % 4, ldx % 8, ldy % 4, res_ld % 4");
    if (flags & ~(CBW_EPI_RELU | CBW_EPI_GELU | CBW_EPI_RES_F32 | CBW_EPI_OUT_F32 | CBW_EPI_RES_AFTER_ACT))
        return fail(CBW_ERR_INVALID, "cbw_linear_rows: unknown flag");
    if (xf && (!ln_g || !ln_b || !cbw_gemv_ln_ok(M, K)))
        return fail(CBW_ERR_INVALID, "cbw_linear_rows: the LayerNorm prologue needs gamma, beta and K <= 1280");
    if (kv_k && (!kv_v || kv_D <= 0 || kv_D % 4 || N != 3 * kv_D || kv_ld % 4 || kv_ld < kv_D || (flags & CBW_EPI_OUT_F32)))
        return fail(CBW_ERR_INVALID, "cbw_linear_rows: K/V append needs kv_v, N == 3 kv_D, kv_D % 4, kv_ld % 4, bf16 output");
    if (gemv_route(M, N, K, xf != nullptr).kernel == GemvKernel::Invalid)
        return fail(CBW_ERR_INVALID, "cbw_linear_rows: no kernel for this shape");
    HIPCHK(cbw_gemv(gemv_args(x, xf, ldx, ln_g, ln_b, ln_eps, w, bias, res, res_ld, y, ldy, M, N, K, flags, kv_k, kv_v,
                              kv_ld, kv_D, kv_pos, kv_pos_rows),
                    (hipStream_t)stream));
    return CBW_OK;
}

const char* cbw_linear_rows_kernel(int M, int N, int K, int ln) { return gemv_route(M, N, K, ln != 0).name; }

int cbw_linear_rows_wide(const uint16_t* x, const float* xf, int ldx, const float* ln_g, const float* ln_b, float ln_eps,
                         const uint16_t* w, const float* bias, const void* res, int res_ld, void* y, int ldy, int M,
                         int N, int K, int flags, uint16_t* kv_k, uint16_t* kv_v, int64_t kv_ld, int kv_D,
                         const int32_t* kv_pos, int kv_pos_rows, cbw_stream_t stream) {
    if ((!x && !xf) || !w || !y) return fail(CBW_ERR_INVALID, "cbw_linear_rows_wide: null operand");
    if (M < 1 || M > CBW_DEC_WIDE_ROWS || N < 4 || N % 4 || K < 32 || K % 32 || ldx % 8 || ldy % 4 || ldx < K ||
        ldy < N || (res && (res_ld % 4 || res_ld < N)))
        return fail(CBW_ERR_INVALID, "cbw_linear_rows_wide: 1 <= M <= 80, K % 32, N % 4, ldx % 8, ldy % 4, res_ld % 4");
    if (flags & ~(CBW_EPI_RELU | CBW_EPI_GELU | CBW_EPI_RES_F32 | CBW_EPI_OUT_F32 | CBW_EPI_RES_AFTER_ACT))
        return fail(CBW_ERR_INVALID, "cbw_linear_rows_wide: unknown flag");
    if (xf && (!ln_g || !ln_b || !cbw_gemv_ln_ok(16, K)))
        return fail(CBW_ERR_INVALID, "cbw_linear_rows_wide: the LayerNorm prologue needs gamma, beta and K <= 1280");
    if (kv_k && (!kv_v || kv_D <= 0 || kv_D % 4 || N != 3 * kv_D || kv_ld % 4 || kv_ld < kv_D || (flags & CBW_EPI_OUT_F32)))
        return fail(CBW_ERR_INVALID, "cbw_linear_rows_wide: K/V append needs kv_v, N == 3 kv_D, kv_D % 4, kv_ld % 4, bf16 output");
    if (gemv_wide_route(M, N, K, xf != nullptr).groups < 1)
        return fail(CBW_ERR_INVALID, "cbw_linear_rows_wide: no kernel for this shape");
    HIPCHK(cbw_gemv_wide(gemv_args(x, xf, ldx, ln_g, ln_b, ln_eps, w, bias, res, res_ld, y, ldy, M, N, K, flags, kv_k,
                                   kv_v, kv_ld, kv_D, kv_pos, kv_pos_rows),
                         (hipStream_t)stream, gemv_wide_groups_fast()));
    return CBW_OK;
}

const char* cbw_linear_rows_wide_kernel(int M, int N, int K, int ln) { return gemv_wide_route(M, N, K, ln != 0).name; }

int cbw_layernorm_rows(const float* x, const float* g, const float* b, uint16_t* y, float* y32, int rows, int D,
                       float eps, cbw_stream_t stream) {
    if (!x || !g || !b || (!y && !y32) || rows <= 0 || D <= 0 || D % 4)
        return fail(CBW_ERR_INVALID, "cbw_layernorm_rows: null operand, empty shape or D % 4 != 0");
    HIPCHK(cbw_layernorm(x, g, b, y, y32, rows, D, eps, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_conv1x1_dual(const uint16_t* x, const uint16_t* x2, const uint16_t* w, const float* bias, const void* res,
                     void* y, int N, int H, int W, int Cin, int H2, int W2, int Cin2, int s2, int Cout, int flags,
                     cbw_stream_t stream) {
    if (!x || !x2 || !w || !y || N <= 0 || H <= 0 || W <= 0 || Cin % 64 || Cin2 % 64 || Cout % 128 || s2 < 1 ||
        (H - 1) * s2 >= H2 || (W - 1) * s2 >= W2 || (flags & ~1))
        return fail(CBW_ERR_INVALID, "cbw_conv1x1_dual: bad shapes");
    const void* zp = nullptr;
    CHK(block_zero_page(&zp));
    ConvArgs a{};
    a.x = x; a.w = w; a.bias = bias; a.res = res; a.y = y; a.zero = zp;
    a.x2 = x2; a.Cin2 = Cin2; a.H2 = H2; a.W2 = W2; a.s2 = s2;
    conv_geometry(a, N, H, W, Cin, Cout, 1, 1, 1, 1, 0, 0);
    a.res_ld = a.y_ld = Cout;
    a.flags = flags;
    HIPCHK(cbw_conv_igemm(a, (hipStream_t)stream));
    return CBW_OK;
}

// ---- the exact-decision tiers' kernels one by one (tests): argument checks, then the launcher the tier calls
int cbw_conv2d_f32(const float* x, const float* w, const float* bias, const float* res, float* y, int N, int H, int W,
                   int Cin, int Cout, int KH, int KW, int sh, int sw, int ph, int pw, int relu, cbw_stream_t stream) {
    if (!x || !w || !y || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cout % 64 || KH <= 0 || KW <= 0 ||
        sh <= 0 || sw <= 0 || ph < 0 || pw < 0 || H + 2 * ph < KH || W + 2 * pw < KW)
        return fail(CBW_ERR_INVALID, "cbw_conv2d_f32: null operand, empty shape or Cout % 64 != 0");
    if (Cin % 16 == 0 && (((uintptr_t)x | (uintptr_t)w) & 15))
        return fail(CBW_ERR_INVALID, "cbw_conv2d_f32: x and w must be 16-byte aligned when Cin % 16 == 0");
    F32ConvArgs a{};
    a.x = x; a.w = w; a.bias = bias; a.res = res; a.y = y;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.KH = KH; a.KW = KW;
    a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw;
    a.Ho = (H + 2 * ph - KH) / sh + 1;
    a.Wo = (W + 2 * pw - KW) / sw + 1;
    if ((int64_t)N * a.Ho * a.Wo > INT32_MAX / 64 || (int64_t)KH * KW * Cin > INT32_MAX / 64)
        return fail(CBW_ERR_INVALID, "cbw_conv2d_f32: shape too large");
    a.M = N * a.Ho * a.Wo;
    a.relu = relu ? 1 : 0;
    HIPCHK(cbw_conv_f32(a, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_sim_maps_f32(const float* utt, const float* utt_mask, int B, const float* kwd, const float* kwd_mask, int K,
                     int L, int Tk, int Tu, int E, const int32_t* pair_utt, const int32_t* pair_kwd, int n_pairs,
                     const int32_t* sel, int p0, int P, float* out, cbw_stream_t stream) {
    if (!utt || !utt_mask || !kwd || !kwd_mask || !sel || !out || B < 0 || K < 1 || L < 1 || Tk < 1 || Tu < 1 || E < 4 ||
        E % 4 || p0 < 0 || P < 1 || P > 65535 || (int64_t)L * E * 4 > 64 * 1024)
        return fail(CBW_ERR_INVALID, "cbw_sim_maps_f32: null operand or bad shape (E % 4 == 0, 1 <= P <= 65535)");
    if ((((uintptr_t)utt | (uintptr_t)kwd) & 15))
        return fail(CBW_ERR_INVALID, "cbw_sim_maps_f32: utt and kwd must be 16-byte aligned");
    if (B == 0) {
        if (pair_utt || pair_kwd) return fail(CBW_ERR_INVALID, "cbw_sim_maps_f32: pair indices need B >= 1");
        HIPCHK(cbw_sim_f32(kwd, kwd_mask, utt, utt_mask, sel, p0, P, out, L, Tk, Tu, E, (hipStream_t)stream));
        return CBW_OK;
    }
    if ((pair_utt == nullptr) != (pair_kwd == nullptr) || n_pairs < 1 ||
        (!pair_utt && (int64_t)n_pairs != (int64_t)B * K))
        return fail(CBW_ERR_INVALID, "cbw_sim_maps_f32: both index arrays or neither, and then n_pairs == B * K");
    HIPCHK(cbw_sim_f32_pairs(kwd, kwd_mask, K, utt, utt_mask, B, pair_utt, pair_kwd, n_pairs, sel, p0, P, out, L, Tk, Tu,
                             E, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_maxpool_f32(const float* x, float* y, int N, int H, int W, int C, cbw_stream_t stream) {
    if (!x || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(CBW_ERR_INVALID, "cbw_maxpool_f32: bad argument");
    HIPCHK(cbw_maxpool_f32(x, y, N, H, W, C, out_dim(H, 3, 2), out_dim(W, 3, 2), (hipStream_t)stream));
    return CBW_OK;
}

int cbw_pool_fc_f32(const float* x, const float* w, const float* b, const int32_t* sel, int p0, int P, float* logits,
                    int HW, int C, cbw_stream_t stream) {
    if (!x || !w || !b || !sel || !logits || p0 < 0 || P <= 0 || HW <= 0 || C <= 0)
        return fail(CBW_ERR_INVALID, "cbw_pool_fc_f32: bad argument");
    HIPCHK(cbw_pool_fc_f32(x, w, b, sel, p0, P, logits, HW, C, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_split3_f32(const float* x, uint16_t* y, int64_t M, int C, cbw_stream_t stream) {
    if (!x || !y || M <= 0 || C <= 0 || C % 4 || (((uintptr_t)x | (uintptr_t)y) & 15))
        return fail(CBW_ERR_INVALID, "cbw_split3_f32: null or misaligned operand, or C % 4 != 0");
    HIPCHK(cbw_split3(x, y, M, C, (hipStream_t)stream));
    return CBW_OK;
}

int64_t cbw_channel_sum_workspace_bytes(int C) {
    if (C <= 0) return fail(CBW_ERR_INVALID, "cbw_channel_sum_workspace_bytes: bad argument");
    return (int64_t)cbw_channel_sum_groups() * C * (int64_t)sizeof(float);
}

int cbw_channel_sum_f32(const float* x, int64_t M, int C, float* part, int64_t part_bytes, cbw_stream_t stream) {
    if (!x || !part || M <= 0 || C <= 0) return fail(CBW_ERR_INVALID, "cbw_channel_sum_f32: bad argument");
    if (part_bytes < cbw_channel_sum_workspace_bytes(C)) return fail(CBW_ERR_OOM, "cbw_channel_sum_f32: part too small");
    HIPCHK(cbw_channel_sum_f32(x, M, C, part, (hipStream_t)stream));
    return CBW_OK;
}

int cbw_conv2d_x3(const uint16_t* x, const uint16_t* w, const float* bias, const void* res, int res_split, void* y,
                  float* y32, int out_split, int N, int H, int W, int C, int Cout, int k, int stride, int relu,
                  cbw_stream_t stream) {
    if (!x || !w || !bias || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 64 || Cout <= 0 || Cout % 64 ||
        (k != 1 && k != 3) || (stride != 1 && stride != 2) || (y32 && !out_split))
        return fail(CBW_ERR_INVALID, "cbw_conv2d_x3: null operand, C or Cout not a multiple of 64, k not 1 / 3, stride "
                                     "not 1 / 2, or y32 without the split output");
    const void* zp = nullptr;
    CHK(block_zero_page(&zp));
    const ConvShape c{3 * C, Cout, k, stride, relu != 0};
    return launch_conv_x3(c, w, bias, x, N, H, W, y, y32, res, res_split != 0,
                          out_split ? CBW_EPI_SPLIT3 : CBW_EPI_OUT_F32, zp, (hipStream_t)stream, nullptr);
}

}  // extern "C"
