"""CPU-only: the exact tiers of CB-Whisper's own 12-channel spotter are part of the C ABI -- declared in include/cbw.h,
exported by libcbw.so and bound in the ctypes table with the declared argument count -- and what their host code can
refuse without a device, it refuses (no compute calls: no GPU here, so no handle exists; the checks that need one
are in tests/test_gpu_cnn12_exact.py::test_argument_errors)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO

NEW = ["cbw_kws_build_exact", "cbw_kws_rescore_resized_workspace_bytes", "cbw_kws_rescore_resized",
       "cbw_kws_rescore_resized_x3_workspace_bytes", "cbw_kws_rescore_resized_x3", "cbw_kws_sim_rows_f32",
       "cbw_kws_sim_resize_f32"]
TIER_ARGS = ["h", "utt", "Tu", "kwd", "R", "D", "off_dev", "off_host", "K", "Ho", "Wo", "sel", "n_sel", "logits", "ws",
             "ws_bytes", "stream"]


def declaration(name):
    src = open(os.path.join(REPO, "include", "cbw.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*(?:int|int64_t)\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.M | re.S)
    assert m, f"include/cbw.h does not declare {name}"
    return [a.strip() for a in m.group(1).split(",")]


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


@pytest.mark.parametrize("name", ["cbw_kws_rescore_resized", "cbw_kws_rescore_resized_x3"])
def test_tier_signature_and_null_handle(name):
    from cbw import _lib
    args = declaration(name)
    assert [a.split()[-1].lstrip("*") for a in args] == TIER_ARGS
    assert [a.split()[-1].lstrip("*") for a in declaration(name + "_workspace_bytes")] == \
        ["h", "off_host", "K", "Tu", "D", "Ho", "Wo"]
    lib = _lib.load()
    # a null handle is refused before anything else is read
    assert getattr(lib, name)(*([None] + [0 if "*" not in a and "stream" not in a else None for a in args[1:]])) == -1
    assert lib.cbw_last_error()
    assert getattr(lib, name + "_workspace_bytes")(None, None, 0, 1500, 1280, 150, 750) == -1
    assert lib.cbw_kws_build_exact(None) == -1 and b"null" in lib.cbw_last_error()


def test_stage_entry_points_refuse_bad_arguments_before_any_launch():
    """cbw_kws_sim_rows_f32 / cbw_kws_sim_resize_f32 take no handle: their checks run without a device.  Host buffers
    stand in for device memory: a refused call reads nothing."""
    from cbw import _lib
    lib = _lib.load()
    f = torch.zeros(64, dtype=torch.float32)
    ix = torch.zeros(4, dtype=torch.int32)
    p, q = f.data_ptr(), ix.data_ptr()
    assert p % 16 == 0

    def rows(utt=p, Tu=4, kwd=p, R=4, D=16, L=1, off=q, K=1, sel=q, n=1, tk_max=4, ld=64, out=p):
        return lib.cbw_kws_sim_rows_f32(utt, Tu, kwd, R, D, L, off, K, sel, n, tk_max, ld, out, None)
    assert rows(D=24) == -1 and b"16" in lib.cbw_last_error()      # D % 16
    assert rows(D=0) == -1
    assert rows(utt=None) == -1 and rows(sel=None) == -1 and rows(off=None) == -1 and rows(out=None) == -1
    assert rows(ld=3) == -1                                       # a row pitch shorter than the utterance
    assert rows(K=0) == -1 and rows(n=0) == -1 and rows(tk_max=0) == -1 and rows(L=17) == -1
    assert rows(utt=p + 4) == -1 and rows(kwd=p + 8) == -1          # float4 loads need 16-byte alignment

    def resize(rows_=p, Tu=4, R=4, L=1, off=q, K=1, sel=q, n=1, tk_max=4, ld=64, Ho=7, Wo=7, out=p):
        return lib.cbw_kws_sim_resize_f32(rows_, Tu, R, L, off, K, sel, n, tk_max, ld, Ho, Wo, out, None)
    assert resize(rows_=None) == -1 and resize(out=None) == -1 and resize(sel=None) == -1
    assert resize(Ho=0) == -1 and resize(Wo=0) == -1 and resize(ld=3) == -1 and resize(K=0) == -1


def test_pack_keywords_dtype():
    from cbw.kws import pack_keywords
    k = [torch.randn(12, t, 32) for t in (3, 1, 5)]
    r16, off = pack_keywords(k)
    r32, off32 = pack_keywords(k, dtype=torch.float32)
    assert r16.dtype == torch.bfloat16 and r32.dtype == torch.float32
    assert off.tolist() == off32.tolist() == [0, 3, 4, 9] and off.dtype == torch.int32
    assert torch.equal(r32[:, 3:4], k[1]) and torch.equal(r16, r32.to(torch.bfloat16))
