"""CPU-only tests of token-level timestamps on the GPU (cbw_align_matrix, cbw_dtw_dev; include/cbw.h): the C ABI
entries (header, ctypes table, exported symbols), the workspace helper and every argument check, which come before
any GPU work; the float64 restatement that the GPU tests use as their reference (tests/token_ts_ref.py) against
cbw.token_timestamps.extract_token_timestamps, the fp32 host path, on the inputs of the GPU end-to-end test -- the
guard that those inputs are free of near-ties, so that "equal" is a fair demand there; and the CBW_DEV_TOKEN_TS
switch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import token_ts_ref as R
from conftest import REPO

E2E_SHAPES = [(3, 33, 200), (6, 65, 400), (10, 129, 1500)]
E2E_CASES = [(7, "4.37", None, None), (7, "4.37", 300, None), (7, "5.x", None, 3), (7, "5.x", 300, 3),
             (3, "5.x", 300, 3), (1, "4.37", None, None)]     # (width, variant, num_frames, num_input_ids)


def test_header_symbols_and_ctypes_signatures():
    from cbw import _lib
    src = open(os.path.join(REPO, "include", "cbw.h")).read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    want = {"cbw_token_ts_ws_bytes": ("int64_t", ["int T", "int F"]),
            "cbw_align_matrix": ("int", ["const float* probs", "int n", "int T_all", "int t0", "int T", "int F",
                                         "int width", "float* matrix", "int32_t* degenerate", "void* ws",
                                         "int64_t ws_bytes", "cbw_stream_t stream"]),
            "cbw_dtw_dev": ("int", ["const float* matrix", "int T", "int F", "int32_t* first_frame", "int32_t* text_idx",
                                    "int32_t* time_idx", "int32_t* len", "void* ws", "int64_t ws_bytes",
                                    "cbw_stream_t stream"])}
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
    doc = src[src.index("Token-level timestamps on the GPU"):src.index("int64_t cbw_token_ts_ws_bytes")]
    assert "pba_whisper.py:333-336" in doc and "425-442" in doc and "_extract_token_timestamps" in doc


def test_workspace_bytes():
    """4 T ceil((T + F - 1) / 16): one trace word per text row and block of 16 anti-diagonals (include/cbw.h)."""
    from cbw import _lib
    lib = _lib.load()
    for T, F in [(1, 1), (2, 1), (1, 16), (1, 17), (16, 1), (17, 1), (63, 65), (447, 1500), (1024, 1500), (1024, 1)]:
        assert lib.cbw_token_ts_ws_bytes(T, F) == 4 * T * -(-(T + F - 1) // 16), (T, F)
    assert lib.cbw_token_ts_ws_bytes(447, 1500) == 4 * 447 * 122
    for T, F in [(0, 10), (-1, 10), (1025, 10), (10, 0), (10, -5), (10, 1501), (2 ** 31 - 1, 2 ** 31 - 1)]:
        assert lib.cbw_token_ts_ws_bytes(T, F) == -1, (T, F)
        assert b"cbw_token_ts_ws_bytes" in lib.cbw_last_error()


def test_argument_checks_come_before_any_gpu_work():
    """Every refusal of include/cbw.h returns CBW_ERR_INVALID (-1) with a message here, where there is no GPU; the
    pointers are host buffers that a call which passed its checks would hand to a kernel, so none may pass."""
    from cbw import _lib
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    big = 1 << 40                                   # a workspace size that is never the reason
    ok_m = dict(probs=p, n=3, T_all=20, t0=3, T=10, F=100, width=7, matrix=p, degenerate=p, ws=p, ws_bytes=big)
    ok_d = dict(matrix=p, T=10, F=100, first_frame=p, text_idx=p, time_idx=p, len=p, ws=p, ws_bytes=big)

    def matrix(**k):
        a = {**ok_m, **k}
        return lib.cbw_align_matrix(a["probs"], a["n"], a["T_all"], a["t0"], a["T"], a["F"], a["width"], a["matrix"],
                                    a["degenerate"], a["ws"], a["ws_bytes"], None)

    def dtw(**k):
        a = {**ok_d, **k}
        return lib.cbw_dtw_dev(a["matrix"], a["T"], a["F"], a["first_frame"], a["text_idx"], a["time_idx"], a["len"],
                               a["ws"], a["ws_bytes"], None)

    need = lib.cbw_token_ts_ws_bytes(10, 100)
    assert need == 4 * 10 * 7
    bad_m = [dict(probs=None), dict(matrix=None), dict(degenerate=None), dict(ws=None), dict(n=0), dict(n=-2),
             dict(T=1), dict(T=0), dict(T=1025, T_all=2000), dict(t0=-1), dict(t0=11), dict(T_all=12),
             dict(t0=2 ** 31 - 1), dict(F=0), dict(F=-1), dict(F=1501), dict(width=0), dict(width=2), dict(width=6),
             dict(width=9), dict(width=-1), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=p + 2)]
    for k in bad_m:
        assert matrix(**k) == -1, k
        assert b"cbw_align_matrix" in lib.cbw_last_error(), k
    bad_d = [dict(matrix=None), dict(first_frame=None), dict(ws=None), dict(T=0), dict(T=-1), dict(T=1025), dict(F=0),
             dict(F=-7), dict(F=1501), dict(text_idx=None), dict(time_idx=None), dict(len=None),
             dict(text_idx=None, time_idx=None), dict(ws_bytes=need - 1), dict(ws_bytes=-1), dict(ws=p + 1)]
    for k in bad_d:
        assert dtw(**k) == -1, k
        assert b"cbw_dtw_dev" in lib.cbw_last_error(), k


@pytest.mark.parametrize("n,T,F", E2E_SHAPES)
@pytest.mark.parametrize("planted", [True, False])
def test_restatement_equals_host_path(n, T, F, planted):
    """extract_token_timestamps (fp32 torch ops, cbw_dtw's fp32 tables) and the float64 restatement give the same
    timestamps, bit for bit, on the inputs of the GPU end-to-end test (planted) and on plain softmax weights, for both
    variants, num_frames None and 300, num_input_ids 3, and for the widths 3 and 1 that the GPU test adds: the two
    disagree only where two DTW predecessors are closer than the fp32 rounding of the costs, and these inputs hold no
    such cell on the path."""
    from cbw.token_timestamps import extract_token_timestamps
    w = (R.planted_weights if planted else R.softmax_weights)(n, T, F, seed=T)
    for width, variant, num_frames, n_in in E2E_CASES:
        got = extract_token_timestamps(torch.from_numpy(w), width, 0.02, num_frames, variant, n_in)
        ref = R.extract(w, width, 0.02, num_frames, variant, n_in)
        assert got.dtype == torch.float32 and ref.dtype == np.float32 and tuple(got.shape) == ref.shape == (T + 1,)
        assert np.array_equal(got.numpy(), ref), (width, variant, num_frames, n_in, int((got.numpy() != ref).sum()))


def test_restatement_small_cases():
    """The restatement's pieces against the host functions where they are exact: the median filter (a selection) on
    every width and on rows too short to filter, and the DTW on matrices of small integers (exact sums, ties
    everywhere: the tie order) against cbw_dtw."""
    from cbw.token_timestamps import dtw, median_filter
    g = np.random.default_rng(0)
    for F in (1, 2, 3, 4, 7, 31):
        x = g.standard_normal((2, 5, F))
        for width in (1, 3, 5, 7):
            np.testing.assert_array_equal(R.median_filter(x, width), median_filter(torch.from_numpy(x), width).numpy())
    for T, F in [(1, 1), (1, 7), (2, 1), (3, 5), (5, 3), (17, 40), (40, 17)]:
        m = g.integers(-1, 2, (T, F)).astype(np.float64)
        for a, b in zip(R.dtw(m), dtw(m)):
            np.testing.assert_array_equal(a, b)
        ti, tj = R.dtw(m)
        ff = R.first_frames(ti, tj)
        assert ff.shape == (T,) and ff[0] == 0 and (np.diff(ff) >= 0).all()


def test_switch_is_read_at_call_time(monkeypatch):
    from model.pba_whisper import _dev_token_ts
    monkeypatch.delenv("CBW_DEV_TOKEN_TS", raising=False)
    assert _dev_token_ts() is True
    monkeypatch.setenv("CBW_DEV_TOKEN_TS", "0")
    assert _dev_token_ts() is False
    monkeypatch.setenv("CBW_DEV_TOKEN_TS", "1")
    assert _dev_token_ts() is True
