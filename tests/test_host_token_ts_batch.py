"""CPU-only tests of token-level timestamps for a batch of rows (cbw_decoder_cross_attn_probs_slot,
cbw_align_matrix_batch, cbw_dtw_dev_batch, cbw_token_ts_ws_bytes_batch; include/cbw.h): the C ABI entries (header,
ctypes table, exported symbols), the workspace helper, every refusal -- all of which come before any GPU work, so they
are tried here on host pointers -- and generate_batch's refusal of a checkpoint without alignment heads."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO


def _table(rows):
    from cbw import _lib
    t = (_lib.TokenTsWindow * len(rows))()
    for i, r in enumerate(rows):
        t[i] = _lib.TokenTsWindow(r["T_all"], r["t0"], r["T"], r["F"], r["probs_off"], r["matrix_off"], r["ws_off"])
    return t


def test_header_symbols_and_ctypes_signatures():
    from cbw import _lib
    src = open(os.path.join(REPO, "include", "cbw.h")).read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    want = {"cbw_decoder_cross_attn_probs_slot": ("int", ["cbw_decoder* h", "const int32_t* tokens", "int T",
                                                          "const int32_t* heads", "int n", "int slot", "int r0", "int B",
                                                          "int Benc", "void* state", "int64_t state_bytes",
                                                          "float* probs", "cbw_stream_t stream"]),
            "cbw_token_ts_ws_bytes_batch": ("int64_t", ["const cbw_token_ts_window* win", "int N"]),
            "cbw_align_matrix_batch": ("int", ["const float* probs", "int n", "const cbw_token_ts_window* win", "int N",
                                               "int width", "float* matrix", "int32_t* degenerate", "void* ws",
                                               "int64_t ws_bytes", "cbw_stream_t stream"]),
            "cbw_dtw_dev_batch": ("int", ["const float* matrix", "const cbw_token_ts_window* win", "int N",
                                          "int32_t* first_frame", "int ld", "void* ws", "int64_t ws_bytes",
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
    m = re.search(r"#define\s+CBW_TOKEN_TS_MAX_WINDOWS\s+(\d+)", src)
    assert m and int(m.group(1)) == _lib.TOKEN_TS_MAX_WINDOWS == 16
    # the struct of the header, field for field
    m = re.search(r"typedef struct \{([^}]*)\}\s*cbw_token_ts_window;", src)
    assert m
    fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decl = [(ty, [n.strip() for n in names.split(",")]) for ty, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", fields)]
    flat = [(n, {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}[ty]) for ty, names in decl for n in names]
    assert flat == list(_lib.TokenTsWindow._fields_)
    assert ctypes.sizeof(_lib.TokenTsWindow) == 40
    doc = src[src.index("Token-level timestamps for a batch of decoded rows"):src.index("#define CBW_TOKEN_TS_MAX_WINDOWS")]
    assert "pba_whisper.py:333-336" in doc and "425-442" in doc and "_extract_token_timestamps" in doc
    assert "multiple of 4" in doc, "the offsets' alignment is stated"


def test_workspace_bytes_batch():
    """The helper is the sum of the windows' cbw_token_ts_ws_bytes: each is a multiple of 4, the alignment of ws_off,
    so windows packed back to back need no padding.  It refuses what the calls refuse."""
    from cbw import _lib
    lib = _lib.load()
    shapes = [(1, 1), (2, 1), (3, 5), (63, 65), (64, 64), (65, 63), (129, 300), (447, 1500), (1024, 1500), (1024, 1)]
    for N in (1, 3, 10):
        rows, at = [], 0
        for T, F in shapes[:N]:
            rows.append(dict(T_all=T, t0=0, T=T, F=F, probs_off=0, matrix_off=0, ws_off=at))
            one = lib.cbw_token_ts_ws_bytes(T, F)
            assert one > 0 and one % 4 == 0
            at += one
        assert lib.cbw_token_ts_ws_bytes_batch(ctypes.addressof(_table(rows)), N) == at
    ok = dict(T_all=10, t0=0, T=10, F=100, probs_off=0, matrix_off=0, ws_off=0)
    t = _table([ok] * 17)
    for N in (0, -1, 17):
        assert lib.cbw_token_ts_ws_bytes_batch(ctypes.addressof(t), N) == -1
        assert b"cbw_token_ts_ws_bytes_batch" in lib.cbw_last_error()
    assert lib.cbw_token_ts_ws_bytes_batch(None, 1) == -1
    for bad in (dict(T=0, T_all=0), dict(T=1025, T_all=1025), dict(F=0), dict(F=1501)):
        assert lib.cbw_token_ts_ws_bytes_batch(ctypes.addressof(_table([ok, {**ok, **bad}])), 2) == -1, bad
        assert b"cbw_token_ts_ws_bytes_batch" in lib.cbw_last_error()


def test_argument_checks_come_before_any_gpu_work():
    """Every refusal of include/cbw.h returns CBW_ERR_INVALID (-1) with the entry's name, here, where there is no GPU;
    the pointers are host buffers that a call which passed its checks would hand to a kernel, so none may pass.  Each
    refusal of the single-window entries is tried on window 0 and on the last window of a table of three."""
    from cbw import _lib
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    big = 1 << 40                                   # a workspace size that is never the reason
    ok = dict(T_all=20, t0=3, T=10, F=100, probs_off=0, matrix_off=0, ws_off=0)
    need = lib.cbw_token_ts_ws_bytes(10, 100)
    assert need == 280

    def matrix(rows, **k):
        a = {**dict(probs=p, n=3, N=len(rows), width=7, matrix=p, degenerate=p, ws=p, ws_bytes=big), **k}
        t = _table(rows)
        return lib.cbw_align_matrix_batch(a["probs"], a["n"], ctypes.addressof(t), a["N"], a["width"], a["matrix"],
                                          a["degenerate"], a["ws"], a["ws_bytes"], None)

    def dtw(rows, **k):
        a = {**dict(matrix=p, N=len(rows), first_frame=p, ld=1024, ws=p, ws_bytes=big), **k}
        t = _table(rows)
        return lib.cbw_dtw_dev_batch(a["matrix"], ctypes.addressof(t), a["N"], a["first_frame"], a["ld"], a["ws"],
                                     a["ws_bytes"], None)

    per_window_m = [dict(T=1), dict(T=0), dict(T=1025, T_all=2000), dict(t0=-1), dict(t0=11), dict(T_all=12),
                    dict(t0=2 ** 31 - 1), dict(F=0), dict(F=-1), dict(F=1501), dict(probs_off=-1), dict(matrix_off=-4),
                    dict(ws_off=-4), dict(ws_off=2), dict(ws_off=6)]
    per_window_d = [dict(T=0, T_all=0, t0=0), dict(T=-1), dict(T=1025, T_all=2000), dict(F=0), dict(F=-7), dict(F=1501),
                    dict(t0=11), dict(matrix_off=-1), dict(ws_off=-8), dict(ws_off=1), dict(ws_off=1022)]
    for at in (0, 2):
        for bad in per_window_m:
            rows = [dict(ok), dict(ok), dict(ok)]
            rows[at].update(bad)
            assert matrix(rows) == -1, (at, bad)
            assert b"cbw_align_matrix_batch" in lib.cbw_last_error(), (at, bad)
        for bad in per_window_d:
            rows = [dict(ok), dict(ok), dict(ok)]
            rows[at].update(bad)
            assert dtw(rows) == -1, (at, bad)
            assert b"cbw_dtw_dev_batch" in lib.cbw_last_error(), (at, bad)
        # the workspace: too small for the window at its offset (window `at` sits last in the buffer)
        rows = [dict(ok, ws_off=need * ((i - at) % 3)) for i in range(3)]
        for call, name in ((matrix, b"cbw_align_matrix_batch"), (dtw, b"cbw_dtw_dev_batch")):
            assert call(rows, ws_bytes=3 * need - 1) == -1, at
            assert name in lib.cbw_last_error()
    three = [dict(ok, ws_off=need * i) for i in range(3)]
    bad_m = [dict(probs=None), dict(matrix=None), dict(degenerate=None), dict(ws=None), dict(ws=p + 2), dict(n=0),
             dict(n=-2), dict(width=0), dict(width=2), dict(width=6), dict(width=9), dict(width=-1), dict(N=0),
             dict(N=-3), dict(N=17), dict(ws_bytes=0), dict(ws_bytes=-1), dict(ws_bytes=need - 1)]
    for k in bad_m:
        assert matrix(three, **k) == -1, k
        assert b"cbw_align_matrix_batch" in lib.cbw_last_error(), k
    bad_d = [dict(matrix=None), dict(first_frame=None), dict(ws=None), dict(ws=p + 1), dict(N=0), dict(N=17),
             dict(ld=9), dict(ld=0), dict(ld=-1), dict(ws_bytes=0), dict(ws_bytes=-1), dict(ws_bytes=need - 1)]
    for k in bad_d:
        assert dtw(three, **k) == -1, k
        assert b"cbw_dtw_dev_batch" in lib.cbw_last_error(), k
    # ld is held against the largest T, wherever it stands
    for at in (0, 2):
        rows = [dict(ok), dict(ok), dict(ok)]
        rows[at].update(T=30, T_all=40)
        assert dtw(rows, ld=29) == -1 and b"cbw_dtw_dev_batch" in lib.cbw_last_error()
    # T = 1 is a DTW window and no matrix window, as in the single-window entries
    assert matrix([dict(ok, T=1)]) == -1 and b"needs 2 <= T" in lib.cbw_last_error()
    # the slot-taking probe: null pointers are refused under its own name before the handle is read
    for args in [(None, p, 4, p, 1, 0, 0, 1, 1, p, big, p), (p, None, 4, p, 1, 0, 0, 1, 1, p, big, p),
                 (p, p, 4, None, 1, 0, 0, 1, 1, p, big, p), (p, p, 4, p, 1, 0, 0, 1, 1, None, big, p),
                 (p, p, 4, p, 1, 0, 0, 1, 1, p, big, None)]:
        assert lib.cbw_decoder_cross_attn_probs_slot(*args, None) == -1
        assert b"cbw_decoder_cross_attn_probs_slot" in lib.cbw_last_error()


def test_generate_batch_without_alignment_heads_raises_before_any_work():
    """generate's ValueError (4.37.2 _set_num_frames), before the spotting call and before an engine exists."""
    from cbw import synth
    from model.pba_whisper import PBAWhisper
    sd = {"model.encoder." + k: v for k, v in synth.synth_whisper_encoder_state_dict("micro", seed=0).items()}
    sd.update({"model.decoder." + k: v for k, v in synth.synth_whisper_decoder_state_dict("micro", seed=0).items()})
    w = PBAWhisper(synth.WHISPER_CONFIGS["micro"], synth.WHISPER_DECODERS["micro"], sd, suppress_tokens=[1, 2, 7],
                   device=torch.device("cpu"))
    assert not w.alignment_heads
    calls = []

    def spot(input_features, start_of_prev=False):
        calls.append(1)
        return [[] for _ in range(input_features.size(0))]
    feats = torch.zeros(2, synth.WHISPER_CONFIGS["micro"][0], 3000)
    with pytest.raises(ValueError, match="alignment_heads"):
        w.generate_batch(feats, task="transcribe", language="english", keyword_spotting=spot,
                         return_token_timestamps=True)
    assert calls == [], "no spotting call"
    assert w._encoder is None and w._decoder is None, "no engine was built"
