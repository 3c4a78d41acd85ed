"""CPU-only: the batch entry points of CB-Whisper's own 12-channel spotter (one pass over [S] segments x K keywords,
model/cb_whisper.py:87-129) are part of the C ABI -- declared in include/cbw.h, exported by libcbw.so and bound in the
ctypes table with the declared argument count and types -- and what their host code can refuse without a device, it
refuses (no compute calls: no GPU here, so no handle exists; the checks that need one are in
tests/test_gpu_cnn12_batch.py::test_argument_errors)."""
import ctypes

import pytest
import torch

from test_host_cnn12_exact import TIER_ARGS, declaration

NEW = ["cbw_kws_score_resized_batch_workspace_bytes", "cbw_kws_score_resized_batch", "cbw_kws_sim_rows_bf16",
       "cbw_kws_rescore_resized_batch", "cbw_kws_rescore_resized_x3_batch"]


def names(name):
    return [a.split()[-1].lstrip("*") for a in declaration(name)]


def nulls(args):
    return [0 if "*" not in a and "stream" not in a else None for a in args]


@pytest.mark.parametrize("name", NEW)
def test_symbols_exported_declared_and_bound(name):
    from cbw import _lib
    args = declaration(name)
    lib = _lib.load()
    assert hasattr(lib, name), f"libcbw.so does not export {name}"
    restype, argtypes = _lib.SIGNATURES[name]
    assert len(argtypes) == len(args)
    assert restype is (ctypes.c_int64 if name.endswith("workspace_bytes") else ctypes.c_int)
    for a, t in zip(args, argtypes):   # pointers are bound as pointers, integers as integers
        if "*" in a or a.startswith("cbw_stream_t"):
            assert t is ctypes.c_void_p, (name, a)
        else:
            assert t is (ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int), (name, a)


def test_signatures_are_the_per_utterance_ones_with_B():
    """B follows utt in the tiers and in the bf16 pass; the bf16 workspace query takes it after K."""
    for name in ("cbw_kws_rescore_resized", "cbw_kws_rescore_resized_x3"):
        assert names(name) == TIER_ARGS
        assert names(name + "_batch") == TIER_ARGS[:2] + ["B"] + TIER_ARGS[2:]
    one = names("cbw_kws_score_resized")
    assert names("cbw_kws_score_resized_batch") == one[:2] + ["B"] + one[2:]
    assert names("cbw_kws_score_resized_batch_workspace_bytes") == ["h", "off_host", "K", "B", "Tu", "D", "Ho", "Wo",
                                                                    "chunk"]
    assert names("cbw_kws_sim_rows_bf16") == ["utt", "B", "Tu", "kwd", "R", "D", "L", "off_dev", "K", "p0", "pc", "ld",
                                              "rows", "stream"]


@pytest.mark.parametrize("name", ["cbw_kws_score_resized_batch", "cbw_kws_rescore_resized_batch",
                                  "cbw_kws_rescore_resized_x3_batch"])
def test_null_handle_refused_first(name):
    from cbw import _lib
    lib = _lib.load()
    args = declaration(name)
    assert getattr(lib, name)(*([None] + nulls(args[1:]))) == -1
    assert lib.cbw_last_error() and b"null" in lib.cbw_last_error()
    assert lib.cbw_kws_score_resized_batch_workspace_bytes(None, None, 0, 1, 1500, 1280, 150, 750, 64) == -1


def test_sim_rows_bf16_refuses_bad_arguments_before_any_launch():
    """cbw_kws_sim_rows_bf16 takes no handle: its checks run without a device.  Host buffers stand in for device
    memory: a refused call reads nothing."""
    from cbw import _lib
    lib = _lib.load()
    f = torch.zeros(1024, dtype=torch.float32)
    ix = torch.zeros(4, dtype=torch.int32)
    p, q = f.data_ptr(), ix.data_ptr()
    assert p % 16 == 0

    def rows(utt=p, B=1, Tu=4, kwd=p, R=4, D=64, L=1, off=q, K=2, p0=0, pc=1, ld=64, out=p):
        return lib.cbw_kws_sim_rows_bf16(utt, B, Tu, kwd, R, D, L, off, K, p0, pc, ld, out, None)
    assert rows(utt=None) == -1 and b"null" in lib.cbw_last_error()
    assert rows(kwd=None) == -1 and rows(off=None) == -1 and rows(out=None) == -1
    assert rows(D=96) == -1 and b"64" in lib.cbw_last_error()       # D % 64
    assert rows(D=16) == -1 and rows(D=0) == -1
    assert rows(ld=3) == -1                                          # a row pitch shorter than the utterance
    assert rows(L=17) == -1 and rows(L=0) == -1
    assert rows(B=0) == -1 and rows(B=-1) == -1
    assert rows(pc=0) == -1 and rows(pc=-1) == -1 and rows(p0=-1) == -1
    assert rows(p0=2, pc=1) == -1 and rows(p0=1, pc=2) == -1         # p0 + pc > B * K = 2
    assert rows(B=3, p0=4, pc=3) == -1                               # 7 > 6
    assert rows(K=0) == -1 and rows(Tu=0) == -1 and rows(R=0) == -1
    assert rows(utt=p + 4) == -1 and rows(kwd=p + 8) == -1           # 16-byte loads need 16-byte alignment
