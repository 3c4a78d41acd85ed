"""CPU-only tests of the decoder's attention building blocks (cbw_decode_attention, cbw_decode_attention_ws_floats,
cbw_decode_cross_probs; include/cbw.h): the C ABI entries (header, ctypes table, exported symbols), the workspace
helper and every argument check, which come before any GPU work; and the two checks on tests/dec_attention_ref.py
under which tests/test_gpu_dec_attention.py means anything:

* the inputs discriminate: on every input of the GPU tests a wrongly restated operation (one key fewer, one key more,
  the v of the last two live keys swapped, a neighbouring K/V batch, row 4 computed from row 0's query, a mis-combined
  chunk) leaves the bound by at least 10x on every row it touches, while dropping a chunk whose factor underflows stays
  inside it;
* the bound is fair: the kernels' arithmetic restated in fp32 on the CPU (bf16 output) stays inside it on every input.

A GPU test that passes therefore says that the kernel made none of these errors, and a kernel that rounds like fp32 is
not asked for more than fp32 gives."""
import ctypes
import os
import re

import numpy as np
import pytest

import dec_attention_ref as R
from conftest import REPO

CASES = R.all_cases()
WS1 = 24 * 8 * 66            # partial floats per (row, head): 24 chunks x 8 rows x (64 outputs + max + sum)


def test_header_symbols_and_ctypes_signatures():
    from cbw import _lib
    src = open(os.path.join(REPO, "include", "cbw.h")).read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    want = {"cbw_decode_attention_ws_floats": ("int64_t", ["int B", "int H"]),
            "cbw_decode_attention": ("int", ["const uint16_t* q", "int ldq", "const uint16_t* k", "const uint16_t* v",
                                             "int64_t kv_bstride", "int n_keys", "int rows_per_kv",
                                             "const int32_t* n_keys_pos", "int nk_rows", "int causal", "int path",
                                             "uint16_t* out", "int B", "int H", "int D", "float* ws",
                                             "int64_t ws_floats", "cbw_stream_t stream"]),
            "cbw_decode_cross_probs": ("int", ["const uint16_t* q", "int ldq", "const uint16_t* k", "int n_keys", "int T",
                                               "int D", "int head", "float* out", "cbw_stream_t stream"])}
    lib = _lib.load()
    for name, (ret, params) in want.items():
        m = re.search(r"^" + ret + r"\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.M | re.S)
        assert m, f"include/cbw.h does not declare {name}"
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == params
        res, args = _lib.SIGNATURES[name]
        assert res is kinds[ret]
        assert list(args) == [ctypes.c_void_p if "*" in p or p.startswith("cbw_stream_t") else kinds[p.split()[0]]
                              for p in params]
        assert hasattr(lib, name)
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert all(name in doc for name in want)


def test_workspace_floats():
    from cbw import _lib
    lib = _lib.load()
    for B, H in [(1, 1), (5, 20), (80, 20), (448, 2), (16, 6), (1, 65535)]:
        assert lib.cbw_decode_attention_ws_floats(B, H) == B * H * WS1, (B, H)
    for B, H in [(0, 1), (1, 0), (-1, 4), (4, -1), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 20, 2 ** 10)]:
        assert lib.cbw_decode_attention_ws_floats(B, H) == -1, (B, H)
        assert b"cbw_decode_attention_ws_floats" in lib.cbw_last_error()


def _host_pointer():
    buf = np.zeros(4096, dtype=np.uint8)
    return buf, (buf.ctypes.data + 63) // 64 * 64


def test_argument_checks_come_before_any_gpu_work(monkeypatch):
    """Every refusal of include/cbw.h returns CBW_ERR_INVALID (-1) with the function's name in the message here, where
    there is no GPU; the pointers are host buffers that a call which passed its checks would hand to a kernel, so none
    may pass."""
    from cbw import _lib
    lib = _lib.load()
    for name in ("CBW_DEC_SPLIT", "CBW_DEC_SELF_ONE", "CBW_DEC_SELF_SPLIT"):
        monkeypatch.delenv(name, raising=False)
    keep, p = _host_pointer()
    big = 1 << 40
    ok = dict(q=p, ldq=192, k=p, v=p, kv_bstride=100 * 192, n_keys=100, rows_per_kv=1, n_keys_pos=None, nk_rows=0,
              causal=0, path=3, out=p, B=4, H=3, D=192, ws=p, ws_floats=big)

    def attn(**kw):
        a = {**ok, **kw}
        return lib.cbw_decode_attention(a["q"], a["ldq"], a["k"], a["v"], a["kv_bstride"], a["n_keys"], a["rows_per_kv"],
                                        a["n_keys_pos"], a["nk_rows"], a["causal"], a["path"], a["out"], a["B"], a["H"],
                                        a["D"], a["ws"], a["ws_floats"], None)

    need = lib.cbw_decode_attention_ws_floats(4, 3)
    bad = []
    for path in range(5):
        base = dict(path=path, rows_per_kv=1)
        bad += [dict(base, q=None), dict(base, k=None), dict(base, v=None), dict(base, out=None),
                dict(base, q=p + 2), dict(base, k=p + 8), dict(base, v=p + 4),
                dict(base, B=0), dict(base, B=-4), dict(base, H=0), dict(base, H=-1),
                dict(base, D=128), dict(base, H=4), dict(base, D=196, kv_bstride=100 * 196),
                dict(base, ldq=196), dict(base, ldq=184), dict(base, ldq=128),
                dict(base, kv_bstride=100 * 192 - 8), dict(base, kv_bstride=100 * 192 + 4), dict(base, kv_bstride=0),
                dict(base, n_keys=0), dict(base, n_keys=-1), dict(base, n_keys=1537, kv_bstride=big),
                dict(base, rows_per_kv=0), dict(base, rows_per_kv=-2), dict(base, rows_per_kv=3),
                dict(base, B=5, rows_per_kv=2)]
        if path != 2:
            bad += [dict(base, causal=1)]
    bad += [dict(path=4, n_keys=449, kv_bstride=big), dict(path=4, rows_per_kv=2), dict(path=4, rows_per_kv=4),
            dict(path=3, rows_per_kv=9, B=9), dict(path=3, rows_per_kv=16, B=16),
            dict(path=2, n_keys_pos=p), dict(path=2, n_keys_pos=p, causal=1),
            dict(path=5), dict(path=-1),
            # the workspace, wherever the split kernel can be chosen: path 3; the cross route with up to 8 rows per K/V
            # batch; the self route past 448 keys or with several rows per batch; any route with device counts
            dict(path=3, ws=None), dict(path=3, ws_floats=need - 1), dict(path=3, ws_floats=0),
            dict(path=1, ws=None), dict(path=1, ws_floats=need - 1), dict(path=1, rows_per_kv=4, ws=None),
            dict(path=0, n_keys=449, kv_bstride=big, ws=None), dict(path=0, rows_per_kv=2, ws_floats=need - 1),
            dict(path=1, rows_per_kv=4, n_keys_pos=p, ws=None),
            dict(path=3, B=2 ** 20, H=2 ** 10, D=2 ** 16, ldq=2 ** 16, kv_bstride=big),   # no workspace size exists
            # device counts go to the split kernel, which serves at most 8 rows per K/V batch
            dict(path=1, rows_per_kv=16, B=16, n_keys_pos=p), dict(path=0, rows_per_kv=16, B=16, n_keys_pos=p)]
    for kw in bad:
        assert attn(**kw) == -1, kw
        assert b"cbw_decode_attention:" in lib.cbw_last_error(), kw
    # the switches move the routes, and the checks with them: the self route on split + combine needs the workspace
    monkeypatch.setenv("CBW_DEC_SELF_ONE", "0")
    assert attn(path=0, ws=None) == -1 and b"cbw_decode_attention:" in lib.cbw_last_error()
    monkeypatch.delenv("CBW_DEC_SELF_ONE")

    okp = dict(q=p, ldq=192, k=p, n_keys=100, T=3, D=192, head=1, out=p)

    def probs(**kw):
        a = {**okp, **kw}
        return lib.cbw_decode_cross_probs(a["q"], a["ldq"], a["k"], a["n_keys"], a["T"], a["D"], a["head"], a["out"], None)

    for kw in [dict(q=None), dict(k=None), dict(out=None), dict(k=p + 2), dict(n_keys=0), dict(n_keys=-3),
               dict(n_keys=1537), dict(T=0), dict(T=-1), dict(head=-1), dict(head=3), dict(head=2 ** 25),
               dict(D=196), dict(D=64), dict(ldq=64)]:
        assert probs(**kw) == -1, kw
        assert b"cbw_decode_cross_probs" in lib.cbw_last_error(), kw
    del keep


def _row_ratio(mut, ref, tol, rows):
    return (np.abs(mut - ref) / tol)[rows].max(axis=1)


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_discriminate_and_bound_is_fair(name):
    """The mutants of the module docstring against the unmutated reference and its bound, then the fp32 emulation."""
    case = CASES[name]()
    assert case.name == name
    ref, tol = R.reference(case)
    assert np.isfinite(ref).all() and (tol > 0).all()
    B, cnt, equal = case.B, case.counts, case.name == "cross_equal"
    seen = {}

    def mutant(name, rows, **kw):
        rows = np.asarray(rows)
        if rows.size == 0:
            return
        mut, _ = R.reference(case, rows=rows, with_tol=False, **kw)
        ratio = _row_ratio(mut, ref, tol, rows)
        seen[name] = float(ratio.min())
        assert ratio.min() >= 10.0, (case.name, name, int(rows[ratio.argmin()]), float(ratio.min()))

    mutant("one key fewer", np.flatnonzero(cnt >= 2), counts=cnt - 1)
    mutant("one key more", np.flatnonzero(cnt < case.kv_rows), counts=cnt + 1)
    if not equal:    # uniform weights: the output does not depend on the order of the v rows
        mutant("v of the last two keys swapped", np.flatnonzero(cnt >= 2), swap_last=True)
    NB = case.k.shape[0]
    mutant("next K/V batch", np.flatnonzero(case.batch + 1 < NB), batch=case.batch + 1)
    mutant("previous K/V batch", np.flatnonzero(case.batch >= 1), batch=case.batch - 1)
    if case.name.startswith("cross") and case.rows_per_kv >= 5 and not equal:   # equal scores: q does not matter
        qrow = np.arange(B)
        r4 = np.arange(4, B, case.rows_per_kv)
        qrow[r4] = r4 - 4
        mutant("row 4 from row 0's query", r4, qrow=qrow)
    if case.hard_chunk >= 0:
        c = case.hard_chunk
        qf, H = R.f64(case.q), case.H
        for r in range(B):
            K = R.f64(case.k[case.batch[r], :cnt[r]])
            for h in range(H):
                s = K[:, 64 * h:64 * h + 64] @ qf[r, 64 * h:64 * h + 64]
                assert s[64 * c:64 * c + 64].max() <= s.max() - 200.0
        drop, _ = R.reference(case, chunk_edit=(c, "drop"), with_tol=False)
        seen["underflowing chunk dropped (neutral partial)"] = R.worst_ratio(drop, ref, tol)
        assert seen["underflowing chunk dropped (neutral partial)"] <= 1.0
        mutant("underflowing chunk with factor 1", np.arange(B), chunk_edit=(c, "one"))
        same, _ = R.reference(case, chunk_edit=(c, "exact"), with_tol=False)      # the chunked restatement itself
        assert R.worst_ratio(same, ref, tol) <= 1e-3
    emu = R.worst_ratio(R.emulate_fp32(case), ref, tol)
    print(f"{case.name}: fp32 emulation at {emu:.3f} of the bound; smallest mutant ratios {seen}")
    assert emu <= 1.0, (case.name, emu)


def test_probability_reference_is_the_attention_reference():
    """probabilities() applied to v is reference(): the two float64 statements agree to rounding"""
    case = R.probs_case(7, 257)
    ref, _ = R.reference(case)
    for h in (0, case.H - 1):
        p = R.probabilities(case, h)
        assert np.abs(p.sum(axis=1) - 1).max() < 1e-12
        out = p @ R.f64(case.v[0, :case.n_keys, 64 * h:64 * h + 64])
        np.testing.assert_allclose(out, ref[:, 64 * h:64 * h + 64], rtol=1e-10, atol=1e-12)
