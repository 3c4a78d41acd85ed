"""The decode-step GEMV over more than 16 rows (cbw_linear_rows_wide, csrc/gemv.hip): ceil(M / 16) row groups in one
launch, each group the 16-slot kernel of cbw_linear_rows on its rows.  The reference is cbw_linear_rows itself on each
16-row slice (tests/test_gpu_gemv.py pins that kernel to float64): the output and the K/V cache must equal it bit for
bit, rows >= M and cache positions no row names keep the sentinel, and both grid orders (CBW_GEMV_WIDE_ORDER) give the
same bits.

M in {17, 24, 25, 32, 33, 79, 80}: a one-row tail, the 8 | 9 tail (a slice cbw_linear_rows runs on its 8-slot
instantiation, the wide launch on the 16-slot one), full groups and the cap.  Linears: micro's K 128 (MFMA kernel) and
large-v3's K 1280 LayerNorm -> qkv with the K/V append at per-row device positions, K 1280 out-projection with an fp32
residual, LayerNorm -> fc1 with GELU, K 5120 fc2 (dot kernel), and the vocabulary projection once at M = 80.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

GELU, RES_F32, OUT_F32 = 2, 4, 8
ROWS = (17, 24, 25, 32, 33, 79, 80)
SENTINEL = -768.0   # exact in bf16 and f32
ML = 8              # cache positions per row


def _lib():
    from cbw import _lib as L
    return L, L.load()


def _call(fn, w, y, M, n, K, flags, x, xf, ln, bias, res, kv):
    L, _ = _lib()
    g, b, eps = ln if ln else (None, None, 0.0)
    kk, vv, kv_ld, kv_D, pos = kv if kv else (None, None, 0, 0, None)
    return fn(L.ptr(x), L.ptr(xf), K, L.ptr(g), L.ptr(b), eps, L.ptr(w), L.ptr(bias), L.ptr(res), n if res is not None else 0,
              L.ptr(y), n, M, n, K, flags, L.ptr(kk), L.ptr(vv), kv_ld, kv_D, L.ptr(pos), 1 if pos is not None else 0,
              L.stream_handle())


@functools.lru_cache(maxsize=None)
def operands(K, n):
    """80 rows of one Linear, made once on the device and never changed."""
    g = torch.Generator(device="cuda")
    g.manual_seed(7000 + K + n)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda")   # noqa: E731
    return dict(x=r(80, K).to(torch.bfloat16), xf=(3.0 + r(80, K)), w=(r(n, K) / K ** 0.5).to(torch.bfloat16), bias=r(n),
                res=r(80, n), gamma=1.0 + 0.25 * r(K), beta=0.5 * r(K),
                pos=((3 * torch.arange(80, device="cuda") + 1) % ML).to(torch.int32))


def run(kind, K, n, M, wide):
    """One Linear over M rows: the wide call, or cbw_linear_rows per 16-row slice -> (y [M + 1][n], caches or None)."""
    L, lib = _lib()
    o = operands(K, n)
    ln = (o["gamma"], o["beta"], 1e-5) if kind in ("qkv", "fc1", "vocab") else None
    flags = {"qkv": 0, "out": RES_F32 | OUT_F32, "fc1": GELU, "fc2": RES_F32 | OUT_F32, "vocab": OUT_F32}[kind]
    dt = torch.float32 if flags & OUT_F32 else torch.bfloat16
    y = torch.full((M + 1, n), SENTINEL, dtype=dt, device="cuda")
    D = n // 3
    ck = cv = None
    if kind == "qkv":
        ck = torch.full((M + 1, ML, D), SENTINEL, dtype=torch.bfloat16, device="cuda")
        cv = torch.full((M + 1, ML, D), SENTINEL, dtype=torch.bfloat16, device="cuda")
    res = o["res"] if flags & RES_F32 else None
    for r0, m in ([(0, M)] if wide else [(r0, min(16, M - r0)) for r0 in range(0, M, 16)]):
        fn = lib.cbw_linear_rows_wide if wide else lib.cbw_linear_rows
        kv = (ck[r0:], cv[r0:], ML * D, D, o["pos"][r0:]) if ck is not None else None
        rc = _call(fn, o["w"], y[r0:], m, n, K, flags, None if ln else o["x"][r0:], o["xf"][r0:] if ln else None, ln,
                   o["bias"], None if res is None else res[r0:], kv)
        L.check(rc, "cbw_linear_rows_wide" if wide else "cbw_linear_rows")
    torch.cuda.synchronize()
    return y, ck, cv


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check(kind, K, n, M, monkeypatch):
    ref_y, ref_k, ref_v = run(kind, K, n, M, wide=False)
    assert torch.isfinite(ref_y[:M].float()).all() and (ref_y[M] == SENTINEL).all()
    for order in ("columns", "groups"):
        monkeypatch.setenv("CBW_GEMV_WIDE_ORDER", order)
        y, ck, cv = run(kind, K, n, M, wide=True)
        d = bits(y) != bits(ref_y)
        assert not d.any(), (f"{kind} K {K} M {M} order {order}: {int(d.sum())} elements differ from cbw_linear_rows on the "
                             f"16-row slices, first row {int(d.any(1).nonzero()[0])}")
        assert (y[M] == SENTINEL).all(), f"{kind} K {K} M {M}: wrote row M"
        if ck is not None:
            assert torch.equal(bits(ck), bits(ref_k)) and torch.equal(bits(cv), bits(ref_v)), \
                f"{kind} K {K} M {M} order {order}: K/V cache differs from the slices'"
            pos = operands(K, n)["pos"][:M].long()
            named = torch.zeros((M + 1, ML), dtype=torch.bool, device="cuda")
            named[torch.arange(M, device="cuda"), pos] = True
            D = n // 3
            for c, third in ((ck, 1), (cv, 2)):
                assert (c[~named] == SENTINEL).all(), f"{kind} K {K} M {M}: a cache position no row names was written"
                assert torch.equal(bits(c[:M][named[:M]]), bits(y[:M, third * D:(third + 1) * D])), \
                    f"{kind} K {K} M {M}: the appended rows are not the output's K / V thirds"


def test_kernel_names():
    _, lib = _lib()
    name = lambda M, n, K, ln: lib.cbw_linear_rows_wide_kernel(M, n, K, ln).decode()   # noqa: E731
    for M in (1, 16) + ROWS:
        assert name(M, 384, 128, 1) == "gemv_wide_kernel<true>" and name(M, 128, 256, 0) == "gemv_wide_kernel<false>"
        assert name(M, 3840, 1280, 1) == "gemv_dot_wide_kernel<true, 5, 2, 16, 1, 8>"
        assert name(M, 1280, 1280, 0) == "gemv_dot_wide_kernel<false, 5, 2, 16, 1, 8>"
        assert name(M, 1280, 5120, 0) == "gemv_dot_wide_kernel<false, 20, 1, 16, 2, 8>"
    assert name(0, 1280, 1280, 0) == "" and name(81, 1280, 1280, 0) == ""
    assert lib.cbw_linear_rows_kernel(17, 1280, 1280, 0).decode() == ""   # cbw_linear_rows still ends at 16 rows


@pytest.mark.parametrize("M", ROWS)
def test_micro(M, monkeypatch):
    """micro (d_model 128, ffn 256): the MFMA family, LayerNorm -> qkv with the append, out-projection, fc1, fc2."""
    check("qkv", 128, 384, M, monkeypatch)
    check("out", 128, 128, M, monkeypatch)
    check("fc1", 128, 256, M, monkeypatch)
    check("fc2", 256, 128, M, monkeypatch)


@pytest.mark.parametrize("M", ROWS)
def test_large_v3_qkv_append(M, monkeypatch):
    """K 1280 LayerNorm -> qkv, its K and V thirds appended at one device position per row into sentinel-filled caches."""
    check("qkv", 1280, 3840, M, monkeypatch)


@pytest.mark.parametrize("M", ROWS)
def test_large_v3_out_projection(M, monkeypatch):
    """K 1280 out-projection onto the fp32 residual stream."""
    check("out", 1280, 1280, M, monkeypatch)


@pytest.mark.parametrize("M", ROWS)
def test_large_v3_fc1(M, monkeypatch):
    """K 1280 LayerNorm -> fc1 with GELU."""
    check("fc1", 1280, 5120, M, monkeypatch)


@pytest.mark.parametrize("M", ROWS)
def test_large_v3_fc2(M, monkeypatch):
    """K 5120 fc2: one column per wave, the group's rows staged in two K halves."""
    check("fc2", 5120, 1280, M, monkeypatch)


def test_large_v3_vocabulary_projection(monkeypatch):
    """The final LayerNorm -> tied vocabulary projection (51 866 padded to 51 968 columns, f32 logits) at the cap."""
    check("vocab", 1280, 51968, 80, monkeypatch)


def test_rejections():
    """M = 0 and M = 81 come back as CBW_ERR_INVALID and write nothing; so does what cbw_linear_rows rejects."""
    _, lib = _lib()
    o = operands(1280, 1280)
    y = torch.full((82, 1280), SENTINEL, dtype=torch.float32, device="cuda")
    x = torch.zeros((82, 1280), dtype=torch.bfloat16, device="cuda")
    for M in (0, 81, -1):
        rc = _call(lib.cbw_linear_rows_wide, o["w"], y, M, 1280, 1280, OUT_F32, x, None, None, o["bias"], None, None)
        assert rc == -1, f"M {M}: returned {rc}, not CBW_ERR_INVALID"
    rc = _call(lib.cbw_linear_rows_wide, o["w"], y, 40, 1280, 1280, 32, x, None, None, o["bias"], None, None)
    assert rc == -1, "an unknown flag"
    rc = _call(lib.cbw_linear_rows_wide, o["w"], y, 40, 1280, 1280, OUT_F32, None, None, None, o["bias"], None, None)
    assert rc == -1, "no rows"
    rc = _call(lib.cbw_linear_rows, o["w"], y, 17, 1280, 1280, OUT_F32, x, None, None, o["bias"], None, None)
    assert rc == -1, "cbw_linear_rows keeps refusing 17 rows"
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()
