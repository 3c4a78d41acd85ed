"""DecoderEngine.sample_windows / sample_dev (temperature sampling with the token choice on the GPU, cbw_sample_select +
cbw_decoder_step_rows, replayed on the host every few steps) on the micro decoder: against the host loop
DecoderEngine.sample_search on identically seeded device generators (same tokens, log-probs and generator state
afterwards), windows admitted into slots as others finish against each window alone, and PBAWhisper.generate with the
CBW_DEV_SAMPLE switch on and off.  The setup is that of test_gpu_greedy_dev.py.

Token equality is exact: torch.multinomial on the device is the exponential race over one [V] draw that
sample_windows makes itself (tests/test_host_sample.py pins the CPU build's; the equalities below are the device's)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_greedy_dev import EOS, SOT, TB, _biases, _encs, _engine, _rules, _segments, _whisper

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator(device="cuda:0").manual_seed(seed)


def _host(eng, enc, prefix, limit, bias, begin, rules, T, gen):
    eng.start(enc[None], 1)
    return eng.sample_search(prefix, EOS, limit, lambda pos: begin if pos == len(prefix) else bias, rules, len(prefix),
                             temperature=T, generator=gen)


def _same(got, want, what):
    assert got[0] == want[0], f"{what}: tokens differ"
    assert len(got[1]) == len(want[1]) == len(got[0]) - len(what[1])
    assert np.abs(np.array(got[1]) - np.array(want[1])).max() <= 1e-4, f"{what}: log-probs differ"


def _same_generator(g1, g2):
    assert torch.equal(g1.get_state(), g2.get_state())
    assert torch.equal(torch.rand(4, device="cuda:0", generator=g1), torch.rand(4, device="cuda:0", generator=g2))


@pytest.mark.parametrize("timestamps", [True, False])
@pytest.mark.parametrize("T", [0.4, 1.0])
def test_sample_dev_draws_what_sample_search_draws(T, timestamps):
    """Windows that end at their limit inside a replay interval (prefix + 21 / 9 / 14 with a replay every 8 steps) and
    exactly on one (prefix + 16); the same generator goes on from window to window, as in a fallback ladder."""
    eng = _engine()
    e1, e2 = _encs()
    bias, begin = _biases()
    rules = _rules(timestamps)
    windows = [(e1, SOT, 21), (e2, [50361, 1000, 1001] + SOT, 9), (e1, [50361, 900] + SOT, 14), (e2, SOT, 16)]
    g_host, g_dev = _gen(11), _gen(11)
    for enc, prefix, n in windows:
        limit = len(prefix) + n
        want = _host(eng, enc, prefix, limit, bias, begin, rules, T, g_host)
        got = eng.sample_dev(enc, prefix, EOS, limit, bias, begin, rules, T, g_dev)
        print(f"T {T} timestamps {timestamps} +{n}: {got[0][len(prefix):]}")
        _same(got, want, ("window", prefix))
        assert len(got[0]) == limit or got[0][-1] == EOS
        if timestamps:   # the rules act: the first free token is a timestamp
            assert got[0][len(prefix)] >= TB
        _same_generator(g_host, g_dev)
    # other replay periods give the same tokens and leave the generator in the same state
    enc, prefix, n = windows[0]
    first = eng.sample_dev(enc, prefix, EOS, len(prefix) + n, bias, begin, rules, T, _gen(5))
    for every in (1, 3, 32):
        g = _gen(5)
        assert eng.sample_dev(enc, prefix, EOS, len(prefix) + n, bias, begin, rules, T, g, check_every=every) == first
        g_ref = _gen(5)
        _host(eng, enc, prefix, len(prefix) + n, bias, begin, rules, T, g_ref)
        _same_generator(g, g_ref)


@pytest.mark.parametrize("T", [0.4, 1.0])
def test_eos_ends_a_sampled_window(T):
    """A shared bias with +30 on EOS, begin suppression taking it out at the first free position: the first token is
    drawn from the model's scores, the second is EOS; the draws enqueued after it are given back."""
    eng = _engine()
    e1, _ = _encs()
    bias, begin = (b.clone() for b in _biases())
    bias[EOS] = 30.0
    g_host, g_dev = _gen(2), _gen(2)
    want = _host(eng, e1, SOT, 40, bias, begin, None, T, g_host)
    got = eng.sample_dev(e1, SOT, EOS, 40, bias, begin, None, T, g_dev)
    _same(got, want, ("window", SOT))
    assert len(got[0]) == len(SOT) + 2 and got[0][-1] == EOS and got[0][-2] != EOS
    _same_generator(g_host, g_dev)
    # no room at all: the prefix comes back and nothing is drawn
    g = _gen(2)
    assert eng.sample_dev(e1, SOT, EOS, len(SOT), bias, begin, None, T, g) == (SOT, [])
    _same_generator(g, _gen(2))


@pytest.mark.parametrize("timestamps", [True, False])
def test_three_windows_in_two_slots_equal_each_window_alone(timestamps):
    eng = _engine()
    e1, e2 = _encs()
    bias, begin = _biases()
    rules = _rules(timestamps)
    windows = [(e1, SOT), (e2, [50361, 1000, 1001] + SOT), (e1, [50361, 900] + SOT)]
    limits = [len(p) + n for (_, p), n in zip(windows, (21, 9, 14))]
    alone, after = [], []
    for i, ((enc, p), m) in enumerate(zip(windows, limits)):
        g = _gen(20 + i)
        alone.append(eng.sample_dev(enc, p, EOS, m, bias, begin, rules, 0.4, g))
        after.append(g)
    gens = [_gen(20 + i) for i in range(3)]
    got = eng.sample_windows(windows, EOS, limits, bias, begin, rules, 0.4, gens, max_slots=2)
    assert eng._shape == (2, 2)
    for i, (a, b) in enumerate(zip(got, alone)):
        assert a[0] == b[0], f"window {i}: tokens differ from the window alone"
        assert np.array_equal(np.array(a[1], np.float32), np.array(b[1], np.float32)), f"window {i}: log-probs differ"
        _same_generator(gens[i], after[i])
    with pytest.raises(ValueError, match="generator"):
        eng.sample_windows(windows, EOS, limits, bias, begin, rules, 0.4, [gens[0]] * 3)
    with pytest.raises(ValueError, match="temperature"):
        eng.sample_dev(e1, SOT, EOS, 10, bias, begin, rules, 0.0, gens[0])


def _both(monkeypatch, call):
    """call() with CBW_DEV_SAMPLE 1 and 0 -> the results and the number of windows sampled on the device (switch on)
    and on the host at a temperature > 0 (switch off)"""
    from cbw.decoder import DecoderEngine
    out, used = {}, {}
    sd, ss = DecoderEngine.sample_dev, DecoderEngine.sample_search
    for flag in ("1", "0"):
        monkeypatch.setenv("CBW_DEV_SAMPLE", flag)
        dev, host = [], []
        monkeypatch.setattr(DecoderEngine, "sample_dev", lambda self, *a, **k: dev.append(1) or sd(self, *a, **k))
        monkeypatch.setattr(DecoderEngine, "sample_search",
                            lambda self, *a, **k: host.append(k.get("temperature", a[6] if len(a) > 6 else 0)) or
                            ss(self, *a, **k))
        out[flag] = call()
        monkeypatch.setattr(DecoderEngine, "sample_dev", sd)
        monkeypatch.setattr(DecoderEngine, "sample_search", ss)
        used[flag] = (len(dev), sum(1 for t in host if t and t > 0))
    assert used["1"][0] >= 1 and used["1"][1] == 0, "switch on: every sampled window on the device"
    assert used["0"] == (0, used["1"][0]), "switch off: the same windows through sample_search"
    return out["1"], out["0"], used["1"][0]


@pytest.mark.parametrize("timestamps", [False, True])
def test_generate_shortform_sample_same_with_switch_on_and_off(monkeypatch, timestamps):
    w = _whisper()
    g = np.load(os.path.join(GOLDEN, "longform_micro.npz"))
    feats = torch.from_numpy(g["features"][None, :, :3000]).to(w.device)
    on, off, n = _both(monkeypatch, lambda: w.generate(input_features=feats, task="transcribe", language="en",
                                                       num_beams=1, do_sample=True, temperature=0.7, seed=9,
                                                       max_new_tokens=40, return_timestamps=timestamps))
    assert on.tolist() == off.tolist() and on.shape[1] > 4 and n == 1


def test_generate_longform_fallback_same_with_switch_on_and_off(monkeypatch):
    """temperature (0.0, 0.4) with logprob_threshold -1.0: the windows that fail the log-prob check at t = 0 are decoded
    again at t = 0.4 -- at least one must be, or this test shows nothing."""
    w = _whisper()
    g = np.load(os.path.join(GOLDEN, "longform_micro.npz"))
    feats = torch.from_numpy(g["features"][None]).to(w.device)
    on, off, n = _both(monkeypatch, lambda: w.generate(input_features=feats, task="transcribe", language="en",
                                                       num_beams=1, return_timestamps=True,
                                                       condition_on_prev_tokens=False, return_segments=True,
                                                       temperature=(0.0, 0.4), logprob_threshold=-1.0, seed=3))
    assert n >= 1
    assert on["sequences"].tolist() == off["sequences"].tolist()
    assert _segments(on) == _segments(off) and len(on["segments"][0]) >= 2
