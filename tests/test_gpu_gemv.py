"""The decode-step GEMV (csrc/gemv.hip: every Linear of cbw_decoder_step* and the vocabulary projection) through its
building-block entry points cbw_linear_rows / cbw_layernorm_rows, at every row count 1..16 and every width.

K covers the dot kernel's six widths (768, 1024, 1280, 3072, 4096, 5120: NJ = 3, 4, 5, 12, 16, 20, each with its
8-row / 4-wave and 16-row / 8-wave instantiation, K 5120 with one column per wave and two K stages above 8 rows)
and the MFMA kernel at K 128 (1 wave), 384 (2), 1536 (8) and 2048 (8: a K no dot kernel takes).  N = 100: a multiple of
4 but not of 8 or 16, so every instantiation (4, 8 or 16 columns per workgroup) has a column tail and several
workgroups.  Every test asserts cbw_linear_rows_kernel for its (M, K, prologue) against the name written out here
(want_kernel), so no case passes on another kernel than the one it was written for.

  a. exact integers: small-integer operands, every partial sum an integer below 2^24, so any summation order gives the
     int64 result exactly; packed and padded (ldx = K + 8, ldy = N + 4) rows; rows >= M and columns >= N keep a sentinel.
  b. row independence, bit for bit: row r of an M-row call = the 1-row call on row r alone (the sentence of
     cbw_decoder_step_rows in cbw.h), f32 and bf16 outputs, with and without the LayerNorm prologue.
  c. float64 numerics of every epilogue the step uses or admits, at a derived tolerance (see _tolerance).
  d. the LayerNorm prologue = cbw_layernorm_rows then the plain call, bit for bit; cbw_layernorm_rows against float64.
  e. the K/V append of the qkv projection's epilogue, all three position forms, sentinel-checked caches.
  f. every argument rejection returns CBW_ERR_INVALID and writes nothing.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RELU, GELU, RES_F32, OUT_F32, RES_AFTER_ACT = 1, 2, 4, 8, 16
N = 100
DOT_KS = (768, 1024, 1280, 3072, 4096, 5120)
MFMA_KS = (128, 384, 1536, 2048)
ALL_KS = MFMA_KS + DOT_KS
LN_KS = (128, 384, 768, 1024, 1280)
SENTINEL = -768.0   # exact in bf16 and f32, and no output of these operands
U = 2.0 ** -24   # unit roundoff of fp32


def want_kernel(M, K, ln):
    """The kernel cbw_gemv is meant to run, written out from gemv.hip's instantiation list (not from gemv_route.h)."""
    b = "true" if ln else "false"
    if K not in DOT_KS:
        return f"gemv_kernel<{b}>"
    rows = "8, 1, 4" if M <= 8 else "16, 1, 8"
    if K == 5120:
        rows = "8, 1, 4" if M <= 8 else "16, 2, 8"
        return f"gemv_dot_kernel<false, 20, 1, {rows}>"
    return f"gemv_dot_kernel<{b}, {K // 256}, 2, {rows}>"


def mfma_waves(K):
    W = 1
    while W < 16 and -(-(K // 32) // W) > 10:
        W *= 2
    return W


def chain_depth(K):
    """D, the longest chain of fp32 additions a product passes through before the epilogue, read from gemv.hip.
    gemv_dot_kernel: a lane runs NL loads x 4 v_dot2_f32_bf16, each adding two products to the accumulator (2
    additions), then at most 6 lane-exchange additions (wave_sum_x; half_wave_sum has 5): 8 NL + 6, NL = K / 256 with
    two columns per wave and K / 512 = 10 at K 5120.  gemv_kernel: a wave owns ceil(K / 32 / W) <= 10 MFMA steps of 32
    products each (at most 32 additions per step), then wave 0 adds the other W - 1 <= 15 partial sums: at most
    32 steps + 16."""
    if K in DOT_KS:
        nl = 10 if K == 5120 else K // 256
        return 8 * nl + 6
    return 32 * -(-(K // 32) // mfma_waves(K)) + 16


def _lib():
    from cbw import _lib as L
    return L, L.load()


def assert_kernel(M, K, ln, n=N):
    L, lib = _lib()
    got = lib.cbw_linear_rows_kernel(M, n, K, int(ln)).decode()
    assert got == want_kernel(M, K, ln), f"M {M} K {K} ln {ln}: runs {got}, the test was written for {want_kernel(M, K, ln)}"


def linear(w, y, M, n, K, flags=0, x=None, xf=None, ldx=None, ln=None, bias=None, res=None, res_ld=0, ldy=None,
           kv=None, check=True):
    """cbw_linear_rows on device tensors; ln = (gamma, beta, eps); kv = (k, v, kv_ld, kv_D, pos tensor or None, rows)."""
    L, lib = _lib()
    g, b, eps = ln if ln else (None, None, 0.0)
    kk, vv, kv_ld, kv_D, pos, pos_rows = kv if kv else (None, None, 0, 0, None, 0)
    rc = lib.cbw_linear_rows(L.ptr(x), L.ptr(xf), K if ldx is None else ldx, L.ptr(g), L.ptr(b), eps, L.ptr(w),
                             L.ptr(bias), L.ptr(res), res_ld, L.ptr(y), n if ldy is None else ldy, M, n, K, flags,
                             L.ptr(kk), L.ptr(vv), kv_ld, kv_D, L.ptr(pos), pos_rows, L.stream_handle())
    if check:
        L.check(rc, "cbw_linear_rows")
    return rc


def _bf(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def operands(K):
    """Random operands of one width, made once and never changed: 16 rows x ~ N(0, 1) (bf16), w ~ N(0, 1 / K) (bf16),
    bias and residual ~ N(0, 1), and their float64 products."""
    rng = np.random.default_rng(1000 + K)
    x = _bf(rng.standard_normal((16, K)))
    w = _bf(rng.standard_normal((N, K)) / np.sqrt(K))
    bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
    res32 = torch.from_numpy(rng.standard_normal((16, N)).astype(np.float32))
    res16 = res32.to(torch.bfloat16)
    acc = x.double() @ w.double().T
    absacc = x.double().abs() @ w.double().abs().T
    d = "cuda"
    return dict(x=x, w=w, bias=bias, res32=res32, res16=res16, acc=acc, absacc=absacc, xd=x.to(d), wd=w.to(d),
                biasd=bias.to(d), res32d=res32.to(d), res16d=res16.to(d))


# ---------------------------------------------------------------- a. exact integers
@functools.lru_cache(maxsize=None)
def int_operands(K):
    m, n, k = np.arange(16)[:, None], np.arange(N)[:, None], np.arange(K)[None, :]
    x = ((17 * m + 3 * k) % 7) - 3
    w = ((131 * n + 7 * k) % 9) - 4
    bias = (np.arange(N) * 5) % 23 - 11
    ref = x.astype(np.int64) @ w.astype(np.int64).T + bias[None, :]
    assert (np.abs(x).astype(np.int64) @ np.abs(w).astype(np.int64).T).max() + 11 < 2 ** 24
    return (_bf(x).to("cuda"), _bf(w).to("cuda"), torch.from_numpy(bias.astype(np.float32)).to("cuda"),
            torch.from_numpy(ref))


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("K", ALL_KS)
def test_exact_integers(K, padded):
    """Indexing: with integer operands exact in bf16 and every partial sum below 2^24, the f32 output equals the int64
    reference whatever the order of the sums -- every element, every M in 1..16, rows packed and with ldx = K + 8,
    ldy = N + 4; the row after the last and the columns past N keep the sentinel."""
    x, w, bias, ref = int_operands(K)
    ldx, ldy = (K + 8, N + 4) if padded else (K, N)
    xs = torch.zeros((16, ldx), dtype=torch.bfloat16, device="cuda")
    xs[:, :K] = x
    if padded:
        xs[:, K:] = 3.0   # read by no one
    for M in range(1, 17):
        assert_kernel(M, K, False)
        y = torch.full((M + 1, ldy), SENTINEL, dtype=torch.float32, device="cuda")
        linear(w, y, M, N, K, OUT_F32, x=xs, ldx=ldx, bias=bias, ldy=ldy)
        got = y.cpu()
        assert torch.equal(got[:M, :N].to(torch.int64), ref[:M]) and torch.equal(got[:M, :N], ref[:M].float()), \
            f"K {K} M {M}: {(got[:M, :N].double() - ref[:M].double()).abs().max().item()} off the integer result"
        assert (got[M] == SENTINEL).all() and (got[:, N:] == SENTINEL).all(), f"K {K} M {M}: wrote outside [M][N]"


# ---------------------------------------------------------------- b. row independence
def _rows_alone(K, flags, ln):
    """Row r alone, for r in 0..15: sixteen 1-row calls."""
    o = operands(K)
    dt = torch.float32 if flags & OUT_F32 else torch.bfloat16
    out = torch.full((16, N), SENTINEL, dtype=dt, device="cuda")
    assert_kernel(1, K, ln is not None)
    for r in range(16):
        if ln is None:
            linear(o["wd"], out[r:r + 1], 1, N, K, flags, x=o["xd"][r:r + 1], bias=o["biasd"])
        else:
            linear(o["wd"], out[r:r + 1], 1, N, K, flags, xf=ln[0][r:r + 1], ln=ln[1], bias=o["biasd"])
    return out


def _ln_inputs(K, mean=50.0):
    """fp32 rows ~ N(mean, 1); gamma and beta carry an index pattern, so a misplaced chunk shows."""
    rng = np.random.default_rng(77 + K)
    xf = torch.from_numpy((mean + rng.standard_normal((16, K))).astype(np.float32))
    i = np.arange(K)
    g = torch.from_numpy((1.0 + ((i % 13) - 6) / 16.0 + (i // 256) / 8.0).astype(np.float32))
    b = torch.from_numpy((((i % 7) - 3) * 0.5 + (i // 256) * 0.125).astype(np.float32))
    return xf, g, b


@pytest.mark.parametrize("K", ALL_KS)
def test_rows_do_not_depend_on_row_count(K):
    """cbw.h, cbw_decoder_step_rows: "each row's logits equal those of a step over its window alone (bit for bit)".
    For every M in 1..16, row r of the M-row call carries the bits of the 1-row call on row r, f32 and bf16 outputs.
    (Before the dispatch kept one kernel family per K this failed at K 4096 with 8 rows and at K 5120 with 7, 8 and 16
    rows, which ran the MFMA kernel: another summation order.)"""
    o = operands(K)
    for flags in (OUT_F32, 0):
        alone = _rows_alone(K, flags, None)
        for M in range(1, 17):
            assert_kernel(M, K, False)
            y = torch.full((M, N), SENTINEL, dtype=alone.dtype, device="cuda")
            linear(o["wd"], y, M, N, K, flags, x=o["xd"], bias=o["biasd"])
            assert torch.isfinite(y.float()).all()
            diff = (y.view(torch.int32 if flags else torch.int16) != alone[:M].view(torch.int32 if flags else torch.int16))
            assert not diff.any(), (f"K {K} M {M} {'f32' if flags else 'bf16'}: {int(diff.sum())} of {M * N} elements "
                                    f"differ from the 1-row calls, max |d| "
                                    f"{(y.double() - alone[:M].double()).abs().max().item():.3g}")


@pytest.mark.parametrize("K", LN_KS)
def test_rows_do_not_depend_on_row_count_with_prologue(K):
    """The same with the LayerNorm prologue (the dot kernel's: two or four row slots per wave; the MFMA kernel's: rows
    dealt over the waves)."""
    o = operands(K)
    xf, g, b = (t.to("cuda") for t in _ln_inputs(K))
    ln = (g, b, 1e-5)
    for flags in (OUT_F32, 0):
        alone = _rows_alone(K, flags, (xf, ln))
        for M in range(1, 17):
            assert_kernel(M, K, True)
            y = torch.full((M, N), SENTINEL, dtype=alone.dtype, device="cuda")
            linear(o["wd"], y, M, N, K, flags, xf=xf, ln=ln, bias=o["biasd"])
            assert torch.isfinite(y.float()).all()
            assert torch.equal(y, alone[:M]), f"K {K} M {M} {'f32' if flags else 'bf16'}: rows differ from the 1-row calls"


# ---------------------------------------------------------------- c. float64 numerics
EPILOGUES = {
    # name: (bias, residual kind, flags)
    "plain": (True, None, 0),
    "relu": (True, None, RELU),
    "fc1": (True, None, GELU),
    "out_proj_fc2": (True, "f32", RES_F32 | OUT_F32),
    "bf16_residual": (True, "bf16", 0),
    "residual_after_act": (True, "bf16", GELU | RES_AFTER_ACT),
    "no_bias": (False, None, 0),
}


def _tolerance(K, ref, S, flags):
    """Products of two bf16 values are exact in fp32, so only additions round.  With S = sum |x_k w_k| + |bias| +
    |res| and D = chain_depth(K) additions on a product's way, the pre-activation is off by at most D 2^-24 S; GELU
    stretches that by at most max |gelu'| = 1.13 (ReLU and the identity by 1); a bf16 output adds one rounding of the
    reference, 2^-8 |ref|; an f32 output the epilogue's own few additions, 4 2^-24 (|ref| + S)."""
    t = chain_depth(K) * U * S
    if flags & GELU:
        t = t * 1.13
    return t + (4 * U * (ref.abs() + S) if flags & OUT_F32 else 2.0 ** -8 * ref.abs())


@pytest.mark.parametrize("K", ALL_KS)
def test_epilogues_vs_float64(K, capsys):
    """Every epilogue the step uses (plain, fc1's GELU, the f32 residual stream of out-proj / fc2) or admits (ReLU, a
    bf16 residual, the residual after the activation, no bias) against float64 on the same bf16 operands, 1, 5, 8, 9
    and 16 rows, at _tolerance's bound with D = chain_depth(K): 8 NL + 6 = 30 / 38 / 46 / 102 / 134 / 86 for the dot
    kernel's K 768 / 1024 / 1280 / 3072 / 4096 / 5120, 32 steps + 16 = 144 / 208 / 208 / 272 for the MFMA kernel's
    K 128 / 384 / 1536 / 2048.  Prints the largest error / tolerance per epilogue (never an input to the bound)."""
    o = operands(K)
    worst = {}
    for name, (with_bias, res_kind, flags) in EPILOGUES.items():
        pre = o["acc"].clone()
        S = o["absacc"].clone()
        if with_bias:
            pre += o["bias"].double()
            S += o["bias"].double().abs()
        res = None if res_kind is None else (o["res32"] if res_kind == "f32" else o["res16"]).double()
        if res is not None:
            S += res.abs()
            if not flags & RES_AFTER_ACT:
                pre = pre + res
        ref = torch.relu(pre) if flags & RELU else torch.nn.functional.gelu(pre) if flags & GELU else pre
        if res is not None and flags & RES_AFTER_ACT:
            ref = ref + res
        tol = _tolerance(K, ref, S, flags)
        resd = None if res_kind is None else o["res32d"] if res_kind == "f32" else o["res16d"]
        for M in (1, 5, 8, 9, 16):
            assert_kernel(M, K, False)
            y = torch.full((M, N), SENTINEL, dtype=torch.float32 if flags & OUT_F32 else torch.bfloat16, device="cuda")
            linear(o["wd"], y, M, N, K, flags, x=o["xd"], bias=o["biasd"] if with_bias else None, res=resd, res_ld=N)
            got = y.double().cpu()
            ratio = ((got - ref[:M]).abs() / tol[:M]).max().item()
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert np.isfinite(ratio) and ratio <= 1.0, f"K {K} M {M} {name}: error / tolerance = {ratio:.3g}"
    with capsys.disabled():
        print(f"\n[gemv K {K} D {chain_depth(K)}] max error / tolerance: " +
              ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---------------------------------------------------------------- d. LayerNorm prologue
LN_MS = (1, 4, 5, 8, 9, 15, 16)


def layernorm_rows(xf, g, b, rows, K, bf16=True, f32=False, eps=1e-5):
    L, lib = _lib()
    y = torch.full((rows, K), SENTINEL, dtype=torch.bfloat16, device="cuda") if bf16 else None
    y32 = torch.full((rows, K), SENTINEL, dtype=torch.float32, device="cuda") if f32 else None
    L.check(lib.cbw_layernorm_rows(xf.data_ptr(), g.data_ptr(), b.data_ptr(), L.ptr(y), L.ptr(y32), rows, K, eps,
                                   L.stream_handle()), "cbw_layernorm_rows")
    return y, y32


@pytest.mark.parametrize("K", LN_KS)
def test_prologue_equals_layernorm_then_linear(K):
    """GemvArgs: the prologue computes the rows "exactly as layernorm_kernel does".  cbw_layernorm_rows then the plain
    call = the call with the prologue, bit for bit, for rows with a large mean (x ~ N(50, 1): the mean's rounding
    shows in every element) and indexed gamma / beta -- the MFMA kernel's prologue at K 128 / 384 and the dot kernel's
    (wave_sum_x, four or two row slots per wave) at K 768 / 1024 / 1280."""
    o = operands(K)
    xf, g, b = (t.to("cuda") for t in _ln_inputs(K))
    for M in LN_MS:
        assert_kernel(M, K, True)
        assert_kernel(M, K, False)
        a, _ = layernorm_rows(xf, g, b, M, K)
        for flags in (OUT_F32, 0):
            dt = torch.float32 if flags else torch.bfloat16
            two = torch.full((M, N), SENTINEL, dtype=dt, device="cuda")
            one = torch.full((M, N), SENTINEL, dtype=dt, device="cuda")
            linear(o["wd"], two, M, N, K, flags, x=a, bias=o["biasd"])
            linear(o["wd"], one, M, N, K, flags, xf=xf, ln=(g, b, 1e-5), bias=o["biasd"])
            assert torch.isfinite(one.float()).all()
            assert torch.equal(one, two), (f"K {K} M {M}: the prologue differs from cbw_layernorm_rows + cbw_linear_rows "
                                           f"in {int((one != two).sum())} of {M * N} elements")


@pytest.mark.parametrize("mean", [0.0, 50.0], ids=["mean0", "mean50"])
@pytest.mark.parametrize("K", LN_KS)
def test_layernorm_rows_vs_float64(K, mean, capsys):
    """cbw_layernorm_rows against float64 LayerNorm of the same fp32 rows, D = K, the rows of LN_MS.

    Rows x ~ N(0, 1): the mean and the variance are sums of at most 1280 terms of size O(1) (20 additions per lane and 6
    lane exchanges), the division, the addition of eps and rsqrtf one rounding (or ulp) each, and (x - mean) rstd g + b
    four more: a handful of roundings of quantities bounded by |ref| + |beta| + 1, i.e. well inside
    2^-20 (|ref| + |beta| + 1) = 16 unit roundoffs -- the y32 bound.  bf16 output: one bf16 rounding of the reference,
    2^-8 |ref|, plus 2^-8 |beta| for the cancellation of (x - mean) rstd g against beta.

    Rows x ~ N(50, 1) (the prologue test's rows): the fp32 mean itself, near 50, is only known to half an ulp of 50,
    2^-19, more than the whole y32 bound above, and its sum of K terms of size 50 passes through C = 4 K / 256 + 6
    additions; the error of the mean, at most (C + 1) 2^-24 |mean|, moves every output of the row by that times
    rstd |g|.  For these rows this term is added to both bounds; for the N(0, 1) rows the bounds are exactly the ones
    above."""
    rng = np.random.default_rng(500 + K)
    _, g, b = _ln_inputs(K)
    xf = torch.from_numpy((mean + rng.standard_normal((16, K))).astype(np.float32))
    xd, gd, bd = xf.to("cuda"), g.to("cuda"), b.to("cuda")
    x64 = xf.double()
    mu = x64.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x64 - mu) ** 2).mean(1, keepdim=True) + 1e-5)
    ref = (x64 - mu) * rstd * g.double() + b.double()
    extra = 0.0 if mean == 0.0 else (4 * K // 256 + 6 + 1) * U * mu.abs() * rstd * g.double().abs()
    tol32 = 2.0 ** -20 * (ref.abs() + b.double().abs() + 1.0) + extra
    tol16 = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * b.double().abs() + extra
    worst = [0.0, 0.0]
    for M in LN_MS:
        y, y32 = layernorm_rows(xd, gd, bd, M, K, bf16=True, f32=True)
        for i, (got, tol) in enumerate(((y32, tol32), (y, tol16))):
            ratio = ((got.double().cpu() - ref[:M]).abs() / tol[:M]).max().item()
            worst[i] = max(worst[i], ratio)
        only16, none32 = layernorm_rows(xd, gd, bd, M, K, bf16=True, f32=False)
        assert none32 is None and torch.equal(only16, y)
    with capsys.disabled():
        print(f"\n[layernorm_rows K {K} mean {mean:g}] max error / tolerance: y32 {worst[0]:.3g}, bf16 {worst[1]:.3g}")
    assert np.isfinite(worst).all() and worst[0] <= 1.0 and worst[1] <= 1.0, \
        f"K {K} mean {mean:g}: error / tolerance y32 {worst[0]:.3g}, bf16 {worst[1]:.3g}"


# ---------------------------------------------------------------- e. K/V append
@pytest.mark.parametrize("prologue", [False, True], ids=["rows", "layernorm"])
@pytest.mark.parametrize("D", [128, 768, 1280])
def test_kv_append(D, prologue):
    """The qkv projection's epilogue (N = 3 D, kv_D = D): columns [D, 2D) / [2D, 3D) of row m also land at
    kv_k / kv_v + m kv_ld + pos[m] D -- without kv_pos (position 0), with one device position, and with one per row
    (kv_pos_rows = 1) -- and nowhere else: the caches (kv_ld larger than the positions written, one row more than M)
    keep their sentinel everywhere else, and y is the y of the call without the append."""
    K, n = D, 3 * D
    o = operands(K)
    rng = np.random.default_rng(9 + D)
    w = _bf(rng.standard_normal((n, K)) / np.sqrt(K)).to("cuda")
    bias = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to("cuda")
    xf, g, b = (t.to("cuda") for t in _ln_inputs(K))
    src = dict(xf=xf, ln=(g, b, 1e-5)) if prologue else dict(x=o["xd"])
    P = 6                       # positions per cache row
    kv_ld = P * D + 8           # wider than the positions
    for M in (1, 5, 8, 9, 16):
        assert_kernel(M, K, prologue, n)
        plain = torch.full((M, n), SENTINEL, dtype=torch.bfloat16, device="cuda")
        linear(w, plain, M, n, K, 0, bias=bias, **src)
        rows_pos = [(3 * m + 1) % P for m in range(M)]
        forms = {"no kv_pos": (None, 0, [0] * M),
                 "one kv_pos": (torch.tensor([4], dtype=torch.int32, device="cuda"), 0, [4] * M),
                 "kv_pos per row": (torch.tensor(rows_pos, dtype=torch.int32, device="cuda"), 1, rows_pos)}
        for form, (pos, pos_rows, where) in forms.items():
            kc = torch.full((M + 1, kv_ld), SENTINEL, dtype=torch.bfloat16, device="cuda")
            vc = torch.full((M + 1, kv_ld), SENTINEL, dtype=torch.bfloat16, device="cuda")
            y = torch.full((M, n), SENTINEL, dtype=torch.bfloat16, device="cuda")
            linear(w, y, M, n, K, 0, bias=bias, kv=(kc, vc, kv_ld, D, pos, pos_rows), **src)
            assert torch.equal(y, plain), f"D {D} M {M} {form}: y differs from the call without the append"
            want_k = torch.full_like(kc, SENTINEL)
            want_v = torch.full_like(vc, SENTINEL)
            for m, p in enumerate(where):
                want_k[m, p * D:(p + 1) * D] = plain[m, D:2 * D]
                want_v[m, p * D:(p + 1) * D] = plain[m, 2 * D:]
            assert torch.equal(kc, want_k), f"D {D} M {M} {form}: K cache"
            assert torch.equal(vc, want_v), f"D {D} M {M} {form}: V cache"
        assert (plain.float() != SENTINEL).all()


# ---------------------------------------------------------------- f. argument errors
def test_argument_errors():
    """Each rejection cbw_gemv makes comes back from cbw_linear_rows as CBW_ERR_INVALID (-1), and y keeps its sentinel."""
    K, D = 1280, 128
    o = operands(K)
    big = operands(1536)
    xf, g, b = (t.to("cuda") for t in _ln_inputs(K))
    xf_big = torch.zeros((16, 1536), dtype=torch.float32, device="cuda")
    g_big = torch.ones(1536, dtype=torch.float32, device="cuda")
    y = torch.full((17, 3 * D + 8), SENTINEL, dtype=torch.float32, device="cuda")   # room for every case below
    x17 = torch.zeros((17, K + 8), dtype=torch.bfloat16, device="cuda")
    kc = torch.full((16, 4 * D), SENTINEL, dtype=torch.bfloat16, device="cuda")
    vc = torch.full((16, 4 * D), SENTINEL, dtype=torch.bfloat16, device="cuda")
    ln = (g, b, 1e-5)
    w3 = torch.zeros((3 * D, D), dtype=torch.bfloat16, device="cuda")
    xs = operands(D)["xd"]
    cases = {
        "M = 0": dict(w=o["wd"], M=0, n=N, K=K, x=o["xd"]),
        "M = 17": dict(w=o["wd"], M=17, n=N, K=K, x=x17, ldx=K + 8),
        "K % 32": dict(w=o["wd"], M=4, n=N, K=K - 16, x=o["xd"], ldx=K),
        "N % 4": dict(w=o["wd"], M=4, n=N - 2, K=K, x=o["xd"], ldy=N),
        "ldx % 8": dict(w=o["wd"], M=4, n=N, K=K, x=x17, ldx=K + 4),
        "ldy % 4": dict(w=o["wd"], M=4, n=N, K=K, x=o["xd"], ldy=N + 2),
        "xf with K > 1280": dict(w=big["wd"], M=4, n=N, K=1536, xf=xf_big, ln=(g_big, g_big, 1e-5)),
        "xf without gamma": dict(w=o["wd"], M=4, n=N, K=K, xf=xf, ln=(None, b, 1e-5)),
        "xf without beta": dict(w=o["wd"], M=4, n=N, K=K, xf=xf, ln=(g, None, 1e-5)),
        "kv_k with N != 3 kv_D": dict(w=w3, M=4, n=3 * D, K=D, x=xs, kv=(kc, vc, 4 * D, D + 4, None, 0)),
        "kv_k with OUT_F32": dict(w=w3, M=4, n=3 * D, K=D, x=xs, flags=OUT_F32, kv=(kc, vc, 4 * D, D, None, 0)),
        "kv_k without kv_v": dict(w=w3, M=4, n=3 * D, K=D, x=xs, kv=(kc, None, 4 * D, D, None, 0)),
        "no rows": dict(w=o["wd"], M=4, n=N, K=K),
    }
    L, lib = _lib()
    for name, kw in cases.items():
        rc = linear(y=y, check=False, **{"flags": 0, **kw})
        assert rc == -1, f"{name}: returned {rc}, not CBW_ERR_INVALID"
        assert lib.cbw_last_error(), name
    assert lib.cbw_linear_rows_kernel(17, N, K, 0) == b"" and lib.cbw_linear_rows_kernel(4, N, 1536, 1) == b""
    rc = lib.cbw_layernorm_rows(xf.data_ptr(), g.data_ptr(), b.data_ptr(), None, None, 4, K, 1e-5, L.stream_handle())
    assert rc == -1
    rc = lib.cbw_layernorm_rows(xf.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), None, 4, K - 2, 1e-5,
                                L.stream_handle())
    assert rc == -1
    torch.cuda.synchronize()
    assert (y == SENTINEL).all() and (kc.float() == SENTINEL).all() and (vc.float() == SENTINEL).all()
