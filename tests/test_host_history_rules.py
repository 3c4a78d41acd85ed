"""CPU-only tests of cbw_history_rules' host side: the C ABI entry (header symbol, ctypes signature, argument checks that
touch no GPU), the numpy statement of one call (tests/history_rules_ref.py) against transformers' two processors and
against the float64 oracle's restatement of them, and the engine methods' new keywords."""
import ctypes
import inspect
import os
import re
from unittest import mock

import numpy as np
import pytest

from conftest import REPO
from history_rules_ref import history_rules_ref, process_row

V = 40
CONTROLS = [(1.3, 0), (0.7, 0), (1.0, 1), (1.0, 2), (1.0, 3), (1.5, 3)]


def _rows(seed=0, count=24):
    """(logits fp32 [V], history) pairs: lengths 0 .. 60 over a small alphabet, so that tokens and n-grams repeat; a few
    logits at history ids are +-0 and -inf"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        length = [0, 1, 2, 3, 5, 9, 17, 33, 60][i % 9]
        seq = rng.integers(0, 6 if i % 2 else V, length).tolist()
        x = (rng.standard_normal(V) * 3).astype(np.float32)
        for t, v in zip(seq[:3], (0.0, -0.0, -np.inf)):
            x[t] = v
        out.append((x, seq))
    return out


def test_header_symbol_and_ctypes_signature():
    from cbw import _lib
    src = open(os.path.join(REPO, "include", "cbw.h")).read()
    m = re.search(r"^int\s+cbw_history_rules\s*\((.*?)\)\s*;", src, flags=re.M | re.S)
    assert m, "include/cbw.h does not declare cbw_history_rules"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["float* logits", "int B", "int V", "int ld", "int32_t* hist", "int hist_ld", "int32_t* hist_len",
                      "const int32_t* last_tokens", "const int32_t* pos_rows", "const int32_t* active",
                      "float repetition_penalty", "int no_repeat_ngram_size", "cbw_stream_t stream"]
    res, args = _lib.SIGNATURES["cbw_history_rules"]
    want = [ctypes.c_int if p.startswith("int ") else ctypes.c_float if p.startswith("float ") else ctypes.c_void_p
            for p in params]
    assert res is ctypes.c_int and list(args) == want
    assert hasattr(_lib.load(), "cbw_history_rules")
    kernels = open(os.path.join(REPO, "enhance-cb-whisper_amd", "csrc", "cbw_kernels.h")).read()
    assert "cbw_history_rules_launch" in kernels


def test_entry_refuses_bad_arguments_before_any_launch():
    """Every refusal comes from the entry's own checks: the pointers are host arrays no kernel may see, and this test
    runs where there is no GPU."""
    from cbw import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    ok = [p, 1, 8, 8, p, 4, p, None, p, p, 1.5, 2, None]
    bad = [(0, None), (4, None), (6, None), (8, None), (9, None),   # logits, hist, hist_len, pos_rows, active
           (1, 0), (1, 17), (2, 0), (3, 7), (5, 0), (10, 0.0), (10, -1.5), (10, float("nan")), (10, float("inf")),
           (11, -1)]
    for i, v in bad:
        args = list(ok)
        args[i] = v
        assert lib.cbw_history_rules(*args) == -1, (i, v)
        assert b"bad arguments" in lib.cbw_last_error(), (i, v)
    assert not buf.any()


@pytest.mark.parametrize("p,n", CONTROLS)
def test_reference_equals_transformers_processors(p, n):
    """RepetitionPenaltyLogitsProcessor then NoRepeatNGramLogitsProcessor (_get_logits_processor's order) on fp32
    scores, bit for bit."""
    transformers = pytest.importorskip("transformers")
    import torch
    for x, seq in _rows():
        ids = torch.tensor([seq], dtype=torch.long)
        s = torch.from_numpy(x.copy())[None]
        if p != 1.0:
            s = transformers.RepetitionPenaltyLogitsProcessor(p)(ids, s)
        if n > 0:
            s = transformers.NoRepeatNGramLogitsProcessor(n)(ids, s)
        got = x.copy()
        process_row(got, seq, p, n)
        assert np.array_equal(got.view(np.uint32), s[0].numpy().view(np.uint32)), (seq, p, n)


@pytest.mark.parametrize("p,n", CONTROLS)
def test_reference_equals_the_oracles_processor_part(p, n):
    """oracle_processed_step_fn (greedy: the processors on the raw logits) fed these rows' logits in place of the
    decoder's: the same bans exactly, the same values to fp32 rounding (the oracle multiplies and divides in float64)."""
    import oracle.decoder as od
    for x, seq in _rows():
        if not seq:
            continue   # a StepFn row holds at least the token it was just fed
        with mock.patch.object(od, "decoder_logits", lambda *a, **k: x.astype(np.float64)[None]):
            step = od.oracle_processed_step_fn({}, None, 1, V, lambda pos: None, p, n, greedy=True)
            for t, tok in enumerate(seq):
                vals, ids = step([tok], t, None)
        want = np.empty(V)
        want[ids[0]] = vals[0]
        got = x.copy()
        process_row(got, seq, p, n)
        assert np.array_equal(np.isneginf(got), np.isneginf(want)), (seq, p, n)
        fin = np.isfinite(want)
        assert np.all(np.abs(got[fin] - want[fin]) <= 2.0 ** -23 * np.abs(want[fin])), (seq, p, n)


def test_reference_history_upkeep():
    x = np.zeros((5, 8), np.float32)
    hist = np.full((5, 4), -9, np.int32)
    hist[:, :2] = [[1, 2]] * 5
    #            whole  moved  neither  inactive  full
    hist_len = np.array([2, 2, 2, 2, 4], np.int32)
    pos = np.array([1, 2, 5, 2, 4], np.int32)
    active = np.array([1, 1, 1, 0, 1], np.int32)
    last = np.array([3, 3, 3, 3, 3], np.int32)
    y, h, hl = history_rules_ref(x, 6, hist, hist_len, last, pos, active, 1.0, 1)
    assert hl.tolist() == [2, 3, 2, 2, 4] and h[1].tolist() == [1, 2, 3, -9]
    assert np.array_equal(np.delete(h, 1, 0), np.delete(hist, 1, 0))
    assert np.isneginf(y[0]).nonzero()[0].tolist() == [1, 2] and np.isneginf(y[1]).nonzero()[0].tolist() == [1, 2, 3]
    assert not y[2:].any()
    # no last_tokens: the row that moved cannot be completed and is left alone
    y, h, hl = history_rules_ref(x, 6, hist, hist_len, None, pos, active, 1.0, 1)
    assert np.array_equal(h, hist) and np.array_equal(hl, hist_len) and not y[1:].any() and y[0].any()


def test_engine_methods_take_the_two_controls():
    from cbw.decoder import DecoderEngine
    for name in ("greedy_windows", "sample_windows", "greedy_dev", "sample_dev", "_lock_step"):
        ps = inspect.signature(getattr(DecoderEngine, name)).parameters
        assert ps["repetition_penalty"].default is None, name
        assert ps["no_repeat_ngram_size"].default == 0, name
