"""repetition_penalty / no_repeat_ngram_size in the lock-step drivers (DecoderEngine.greedy_windows / sample_windows
over cbw_history_rules) on the micro decoder: the device path against the host path (processed_step_fn), windows
sharing slots against each window alone, sampling, and PBAWhisper.generate with the CBW_DEV_HISTORY switch on and
off."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cbw import synth
from conftest import GOLDEN, PKG, REPO
from test_gpu_greedy_dev import EOS, SOT, _biases, _encs, _engine, _rules
from test_oracle_golden import suppression_bias

pytestmark = pytest.mark.gpu

V = synth.WHISPER_DECODERS["micro"][0]
HEADS = synth.WHISPER_DECODERS["micro"][3]


def _near_tie(got, want, prefix, enc_out, np_bias, rp, ng):
    """test_gpu_decoder.py's rule for two greedy sequences that part: the step where they do is a near-tie (0.05) of the
    two tokens' processed scores under the float64 oracle, and lies past the first two free positions."""
    from oracle.decoder import oracle_processed_step_fn
    i = next(j for j in range(min(len(got), len(want))) if got[j] != want[j])
    assert i > len(prefix) + 2, (got, want)
    sd = synth.synth_whisper_decoder_state_dict("micro", seed=0)
    ostep = oracle_processed_step_fn(sd, enc_out, HEADS, V, np_bias, rp, ng, greedy=True)
    for t in range(i):
        sc, ix = ostep([got[t]], t, None)
    x = np.full(V, -np.inf)
    x[ix[0]] = sc[0]
    print(f"sequences part at index {i}, oracle processed-score gap {x[want[i]] - x[got[i]]:.5f}")
    assert abs(x[want[i]] - x[got[i]]) <= 0.05, (got, want)


@pytest.mark.parametrize("case,rp,ng", [("b1_repetition_penalty", 1.5, 0), ("b1_no_repeat_ngram", None, 2),
                                        ("b1_no_repeat_ngram", None, 1)])
def test_device_path_equals_host_path(case, rp, ng):
    """greedy_dev with a control against greedy over processed_step_fn, on the prefix, suppression and length of the
    transformers fixture's case; and the control changes what is decoded.  The micro decoder repeats tokens (575 575)
    but, over these 24 tokens, no bigram -- transformers' own fixture of the n = 2 case equals its greedy sequence --
    so n = 2 must leave the sequence as it is, and the same prefix is decoded with n = 1 as well, which must not."""
    from cbw.generate import greedy
    g = np.load(os.path.join(GOLDEN, "gen_controls_micro.npz"))
    d = np.load(os.path.join(GOLDEN, "decoder_micro.npz"))
    eng = _engine()
    prefix = g["prefix"].tolist()
    max_length = len(prefix) + 24
    np_bias = suppression_bias(V, g["suppress"].tolist(), len(prefix))
    begin, bias = (torch.from_numpy(np_bias(p)).float().to(eng.device) for p in (len(prefix), len(prefix) + 1))
    enc = torch.from_numpy(d["enc_out"]).to(eng.device)
    dev = eng.greedy_dev(enc, prefix, EOS, max_length, bias, begin, None, repetition_penalty=rp, no_repeat_ngram_size=ng)
    plain = eng.greedy_dev(enc, prefix, EOS, max_length, bias, begin, None)
    eng.start(enc[None], 1)
    step = eng.processed_step_fn(2, lambda pos: begin if pos == len(prefix) else bias, rp, ng, greedy=True)
    host = list(greedy(step, prefix, EOS, max_length))
    print(f"{case}: device {dev}\nhost {host}\nwithout the control {plain}\nfixture {g[case].tolist()}")
    acts = (rp is not None and rp != 1.0) or (len(set(plain)) != len(plain) if ng == 1 else _repeated_bigram(plain))
    assert acts == (ng != 2), "what the control finds to act on in this sequence changed"
    assert (dev != plain) == acts, "the control changed nothing" if acts else "a control with nothing to act on acted"
    if dev != host:
        _near_tie(dev, host, prefix, d["enc_out"], np_bias, rp, ng)


def _repeated_bigram(tokens):
    pairs = list(zip(tokens, tokens[1:]))
    return len(set(pairs)) != len(pairs)


@pytest.mark.parametrize("n", [2, 1])
def test_three_windows_in_two_slots(n):
    """Slot reuse and a replay boundary inside every window (check_every = 3), n = 2 with the timestamp rules on: each
    window as greedy_dev decodes it alone, and no bigram twice.  (A window's whole sequence is the processor's
    history, so no bigram of it may repeat one that ends inside the prefix either; the prefixes hold none twice.)
    Without the control these windows repeat tokens (a closing and an opening timestamp) but no bigram, so n = 2 has
    to leave them as they are; n = 1 runs the same windows with something to forbid: no token twice."""
    eng = _engine()
    e1, e2 = _encs()
    bias, begin = _biases()
    rules = _rules(True)
    windows = [(e1, SOT), (e2, [50361, 1000, 1001] + SOT), (e1, [50361, 900] + SOT)]
    limits = [len(p) + n for (_, p), n in zip(windows, (20, 7, 11))]
    alone = [eng.greedy_dev(enc, p, EOS, m, bias, begin, rules, return_logprobs=True, no_repeat_ngram_size=n)
             for (enc, p), m in zip(windows, limits)]
    got = eng.greedy_windows(windows, EOS, limits, bias, begin, rules, check_every=3, return_logprobs=True, max_slots=2,
                             no_repeat_ngram_size=n)
    assert eng._shape == (2, 2)
    free = [eng.greedy_dev(enc, p, EOS, m, bias, begin, rules) for (enc, p), m in zip(windows, limits)]
    for i, ((seq, lps), (seq1, lps1)) in enumerate(zip(got, alone)):
        print(f"window {i}: {seq[len(windows[i][1]):]}\nwithout the control {free[i][len(windows[i][1]):]}")
        assert seq == seq1, f"window {i}: tokens differ from the window alone"
        assert np.array_equal(np.array(lps, np.float32), np.array(lps1, np.float32)), f"window {i}: log-probs differ"
        assert not _repeated_bigram(seq), f"window {i}: a bigram twice"
        assert n != 1 or len(set(seq)) == len(seq), f"window {i}: a token twice"
        assert len(seq) == limits[i] or seq[-1] == EOS
        acts = len(set(free[i])) != len(free[i]) if n == 1 else _repeated_bigram(free[i])
        assert acts == (n == 1), f"window {i}: what the control finds to act on changed"
        assert (seq != free[i]) == acts, f"window {i}"
    # 80-row state: the same windows, one launch per slice of 16 rows
    wide = eng.greedy_windows(windows, EOS, limits, bias, begin, rules, check_every=3, return_logprobs=True, max_rows=80,
                              no_repeat_ngram_size=n)
    assert [s for s, _ in wide] == [s for s, _ in got]


def test_sampling_with_a_control_equals_each_window_alone():
    from cbw.decoder import banned_ngram_tokens
    eng = _engine()
    e1, e2 = _encs()
    bias, begin = _biases()
    windows = [(e1, SOT), (e2, [50361, 1000, 1001] + SOT), (e1, [50361, 900] + SOT)]
    limits = [len(p) + n for (_, p), n in zip(windows, (14, 6, 9))]

    def gens():
        return [torch.Generator(device=eng.device).manual_seed(100 + i) for i in range(3)]
    kw = dict(top_k=5, repetition_penalty=1.3, no_repeat_ngram_size=1)   # n = 1: a window never draws a token twice
    alone = [eng.sample_dev(enc, p, EOS, m, bias, begin, None, 0.8, gn, **kw)
             for (enc, p), m, gn in zip(windows, limits, gens())]
    got = eng.sample_windows(windows, EOS, limits, bias, begin, None, 0.8, gens(), check_every=3, max_slots=2, **kw)
    free = eng.sample_windows(windows, EOS, limits, bias, begin, None, 0.8, gens(), check_every=3, max_slots=2, top_k=5)
    for i, ((seq, lps), (seq1, lps1)) in enumerate(zip(got, alone)):
        assert seq == seq1 and np.array_equal(np.array(lps, np.float32), np.array(lps1, np.float32)), f"window {i}"
        for j in range(len(windows[i][1]), len(seq)):
            assert seq[j] not in banned_ngram_tokens(seq[:j], 1), f"window {i}: token {j} was banned"
        assert len(seq) == limits[i] or seq[-1] == EOS
    assert [s for s, _ in free] != [s for s, _ in got], "the controls changed no draw"


def test_lock_step_refuses_bad_controls():
    eng = _engine()
    e1, _ = _encs()
    bias, begin = _biases()
    for kw in ({"repetition_penalty": 0.0}, {"repetition_penalty": float("nan")}, {"no_repeat_ngram_size": -1}):
        with pytest.raises(ValueError, match="repetition_penalty"):
            eng.greedy_dev(e1, SOT, EOS, len(SOT) + 3, bias, begin, None, **kw)


_CHILD = """
import json, os, sys
import numpy as np, torch
sys.path[:0] = [{repo!r}, {pkg!r}, os.path.join({repo!r}, "tests")]
from cbw import synth
from cbw.decoder import DecoderEngine
from model.pba_whisper import PBAWhisper
from test_gpu_decoder import micro_whisper_sd
used = []
gw = DecoderEngine.greedy_windows
DecoderEngine.greedy_windows = lambda self, *a, **k: used.append(k.get("no_repeat_ngram_size", 0)) or gw(self, *a, **k)
w = PBAWhisper(synth.WHISPER_CONFIGS["micro"], synth.WHISPER_DECODERS["micro"], micro_whisper_sd(),
               suppress_tokens=[1, 2, 7], max_initial_timestamp_index=50)
g = np.load(os.path.join({golden!r}, "longform_micro.npz"))
short = torch.from_numpy(g["features"][None, :, :3000]).to(w.device)
out = [w.generate(short, language="en", max_new_tokens=40, no_repeat_ngram_size=n)[0].tolist()
       for n in json.loads(sys.argv[1])]
print("RESULT " + json.dumps({{"tokens": out, "device_calls": used}}))
"""


@functools.lru_cache(maxsize=None)
def _generate_in_child(flag, controls):
    env = dict(os.environ, CBW_DEV_HISTORY=flag)
    code = _CHILD.format(repo=REPO, pkg=PKG, golden=GOLDEN)
    r = subprocess.run([sys.executable, "-c", code, controls], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])


def test_generate_same_with_switch_on_and_off():
    """PBAWhisper.generate(short, language="en", no_repeat_ngram_size=2) under CBW_DEV_HISTORY=1 and =0, each in a
    process of its own (the switch is read from the environment): the device path is taken exactly when the switch is
    on, and the tokens are equal (or part at an oracle-confirmed near-tie).  The clip's greedy sequence repeats tokens
    but no bigram, so n = 2 must give that sequence; each process decodes with n = 1 too, which must not."""
    from test_gpu_greedy_dev import _whisper
    on, off = _generate_in_child("1", "[2, 1]"), _generate_in_child("0", "[2, 1]")
    w = _whisper()
    g = np.load(os.path.join(GOLDEN, "longform_micro.npz"))
    short = torch.from_numpy(g["features"][None, :, :3000]).to(w.device)
    plain = w.generate(short, language="en", max_new_tokens=40)[0].tolist()
    print(f"on {on}\noff {off}\nwithout the control {plain}")
    assert on["device_calls"] == [2, 1] and off["device_calls"] == []
    assert not _repeated_bigram(plain) and len(set(plain)) != len(plain)
    for k, n in enumerate((2, 1)):
        got, want = on["tokens"][k], off["tokens"][k]
        assert not _repeated_bigram(got) and not _repeated_bigram(want)
        assert (got != plain) == (n == 1), n
        assert n != 1 or len(set(got)) == len(got)
        if got != want:
            enc = w.encode(w._pack(short))[0].double().cpu().numpy()
            prefix = next(got[:j] for j in range(len(got)) if got[j] not in SOT + [50363])
            _near_tie(got, want, prefix, enc, suppression_bias(V, [1, 2, 7], len(prefix)), None, n)
