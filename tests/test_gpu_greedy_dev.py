"""DecoderEngine.greedy_windows / greedy_dev (greedy search with the token choice on the GPU, cbw_greedy_select +
cbw_decoder_step_rows, replayed on the host every few steps) on the micro decoder: against a host loop over the same
lock-step state, windows admitted into slots as others finish against each window alone, the EOS and the limit ends,
and PBAWhisper.generate with the CBW_DEV_GREEDY switch on and off."""
import functools
import os

import numpy as np
import pytest
import torch

from cbw import synth
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TB, NO_TS, EOS = 50364, 50363, 50257
SOT = [50258, 50259, 50359]


@functools.lru_cache(maxsize=None)
def _engine():
    from cbw.decoder import DecoderEngine
    return DecoderEngine(synth.WHISPER_DECODERS["micro"], synth.synth_whisper_decoder_state_dict("micro", seed=0))


@functools.lru_cache(maxsize=None)
def _encs():
    """decoder_micro.npz's encoder output and a second one made by scaling it"""
    e = torch.from_numpy(np.load(os.path.join(GOLDEN, "decoder_micro.npz"))["enc_out"]).to("cuda:0")
    return e, (e * 0.5).contiguous()


@functools.lru_cache(maxsize=None)
def _biases():
    V = synth.WHISPER_DECODERS["micro"][0]
    bias = torch.zeros(V, device="cuda:0")
    bias[[1, 2, 7]] = float("-inf")
    begin = bias.clone()
    begin[[220, EOS]] = float("-inf")
    return bias, begin


def _rules(on):
    from cbw.timestamps import TimestampRules
    return TimestampRules(TB, NO_TS, EOS, 50) if on else None


def _host_lock_step(eng, windows, limits, bias, bias_begin, rules):
    """Greedy search of every window on one lock-step state with the choice on the host: per row
    cbw_timestamp_rules + cbw_logprob_topk(k = 1), then cbw_decoder_step_rows over all rows; an ended row is fed EOS
    and keeps its position."""
    from cbw import _lib
    lib, dev, V = eng.lib, eng.device, eng.vocab
    n = len(windows)
    eng.start_windows(n, 1)
    for s, (enc, p) in enumerate(windows):
        eng.set_window(s, enc)
        eng.prefill_window(s, 1, p)
    seqs = [list(p) for _, p in windows]
    done = [len(s) >= m for s, m in zip(seqs, limits)]
    lp = torch.empty((1, 1), dtype=torch.float32, device=dev)
    idx = torch.empty((1, 1), dtype=torch.int32, device=dev)
    out = torch.empty((1, V), dtype=torch.float32, device=dev)
    while not all(done):
        toks, inc = [], []
        for r in range(n):
            if done[r]:
                toks.append(EOS)
                inc.append(0)
                continue
            sampled = seqs[r][len(windows[r][1]):]
            b = bias_begin if not sampled else bias
            lg = eng._logits[r]
            if rules is not None:
                st = torch.tensor([rules.state(sampled)], dtype=torch.int32).to(dev)
                _lib.check(lib.cbw_timestamp_rules(lg.data_ptr(), 1, V, eng.vpad, b.data_ptr(), st.data_ptr(),
                                                   rules.timestamp_begin, rules.no_timestamps, rules.eos,
                                                   rules.max_initial, out.data_ptr(), _lib.stream_handle()), "rules")
                b = out
            _lib.check(lib.cbw_logprob_topk(lg.data_ptr(), 1, V, eng.vpad, b.data_ptr(), 0, 1, lp.data_ptr(),
                                            idx.data_ptr(), _lib.stream_handle()), "topk")
            tok = int(idx[0, 0])
            seqs[r].append(tok)
            done[r] = tok == EOS or len(seqs[r]) >= limits[r]
            toks.append(tok)
            inc.append(0 if done[r] else 1)
        if all(done):
            break
        eng.step_rows(torch.tensor(toks, dtype=torch.int32).to(dev))
        eng._posr.add_(torch.tensor(inc, dtype=torch.int32).to(dev))
    return seqs


@pytest.mark.parametrize("timestamps", [True, False])
def test_greedy_windows_matches_host_loop_over_the_same_lock_step_state(timestamps):
    eng = _engine()
    e1, e2 = _encs()
    bias, begin = _biases()
    windows = [(e1, SOT), (e2, [50361, 1000, 1001] + SOT), (e1, [50361, 900] + SOT)]
    limits = [len(p) + n for (_, p), n in zip(windows, (21, 9, 14))]   # ends inside and at replay boundaries
    want = _host_lock_step(eng, windows, limits, bias, begin, _rules(timestamps))
    got = eng.greedy_windows(windows, EOS, limits, bias, begin, _rules(timestamps))
    assert got == want
    assert [len(s) for s in got] == limits or any(s[-1] == EOS for s in got)
    if timestamps:   # the rules act: the first free token of every window is a timestamp
        assert all(s[len(p)] >= TB for s, (_, p) in zip(got, windows))


@pytest.mark.parametrize("timestamps", [True, False])
def test_five_windows_in_three_slots_equal_each_window_alone(timestamps):
    eng = _engine()
    e1, e2 = _encs()
    bias, begin = _biases()
    windows = [(e1, SOT), (e2, [50361, 1000, 1001] + SOT), (e1, [50361, 900] + SOT), (e2, SOT),
               (e2, [50361] + [1200 + i for i in range(70)] + SOT)]   # the last: self-attention past the 64-key chunk
    limits = [len(p) + n for (_, p), n in zip(windows, (5, 19, 8, 11, 3))]
    rules = _rules(timestamps)
    alone = [eng.greedy_dev(enc, p, EOS, m, bias, begin, rules, return_logprobs=True)
             for (enc, p), m in zip(windows, limits)]
    got = eng.greedy_windows(windows, EOS, limits, bias, begin, rules, return_logprobs=True, max_slots=3)
    assert eng._shape == (3, 3)
    for i, ((seq, lps), (seq1, lps1)) in enumerate(zip(got, alone)):
        assert seq == seq1, f"window {i}: tokens differ from the window alone"
        assert np.array_equal(np.array(lps, np.float32), np.array(lps1, np.float32)), f"window {i}: log-probs differ"
        assert len(lps) == len(seq) - len(windows[i][1]) and all(np.isfinite(lps) & (np.array(lps) <= 0))
    # other replay periods give the same result
    again = eng.greedy_windows(windows, EOS, limits, bias, begin, rules, return_logprobs=True, max_slots=3, check_every=3)
    assert again == got
    with pytest.raises(ValueError, match="exceeds"):
        eng.greedy_windows(windows[:1], EOS, eng.max_len + 1, bias, begin)


def test_greedy_dev_logprobs_are_the_processed_scores_log_softmax():
    """log-prob of each step = log_softmax(logits + bias + timestamp mask)[token], recomputed in float64 from the
    logits of a host-driven run of the same state along the same tokens (1e-4, cbw_logprob_topk's tolerance)."""
    from oracle.decoder import _logsumexp, timestamp_mask
    eng = _engine()
    e1, _ = _encs()
    bias, begin = _biases()
    seq, lps = eng.greedy_dev(e1, SOT, EOS, len(SOT) + 6, bias, begin, _rules(True), return_logprobs=True)
    eng.start_windows(1, 1)
    eng.set_window(0, e1)
    eng.prefill_window(0, 1, SOT)
    bh, bbh = bias.cpu().numpy().astype(np.float64), begin.cpu().numpy().astype(np.float64)
    for i, tok in enumerate(seq[len(SOT):]):
        s = eng._logits[0, :eng.vocab].double().cpu().numpy() + (bbh if i == 0 else bh)
        with np.errstate(invalid="ignore"):
            s = s + timestamp_mask(s, seq[len(SOT):len(SOT) + i], TB, NO_TS, EOS, 50)
        assert int(np.argmax(s)) == tok
        assert abs(float(s[tok] - _logsumexp(s)) - lps[i]) <= 1e-4
        eng.step_rows(torch.tensor([tok], dtype=torch.int32).to(eng.device))
        eng._posr.add_(1)


def test_eos_ends_a_window_after_two_tokens():
    """A shared bias with +30 on EOS, begin suppression taking it out at the first free position: the first token is
    the model's, the second EOS."""
    from cbw.generate import greedy
    eng = _engine()
    e1, e2 = _encs()
    bias, begin = (b.clone() for b in _biases())
    bias[EOS] = 30.0
    for enc in (e1, e2):
        seq, lps = eng.greedy_dev(enc, SOT, EOS, 40, bias, begin, None, return_logprobs=True)
        assert len(seq) == len(SOT) + 2 and seq[-1] == EOS and seq[-2] != EOS and len(lps) == 2
        eng.start(enc[None], 1)
        step = eng.step_fn(2, lambda pos: begin if pos == len(SOT) else bias)
        assert seq == greedy(step, SOT, EOS, 40)
    both = eng.greedy_windows([(e1, SOT), (e2, SOT)], EOS, 40, bias, begin)
    assert all(len(s) == len(SOT) + 2 and s[-1] == EOS for s in both)


@pytest.mark.parametrize("timestamps", [True, False])
def test_limit_of_one_new_token(timestamps):
    from cbw.generate import greedy
    eng = _engine()
    e1, _ = _encs()
    bias, begin = _biases()
    rules = _rules(timestamps)
    seq = eng.greedy_dev(e1, SOT, EOS, len(SOT) + 1, bias, begin, rules)
    eng.start(e1[None], 1)
    step = eng.step_fn(2, lambda pos: begin if pos == len(SOT) else bias, rules, len(SOT))
    assert len(seq) == len(SOT) + 1 and seq == greedy(step, SOT, EOS, len(SOT) + 1)
    # no room at all: the prefix comes back, as `greedy` returns it
    assert eng.greedy_dev(e1, SOT, EOS, len(SOT), bias, begin, rules) == SOT


@functools.lru_cache(maxsize=None)
def _whisper():
    from model.pba_whisper import PBAWhisper
    from test_gpu_decoder import micro_whisper_sd
    return PBAWhisper(synth.WHISPER_CONFIGS["micro"], synth.WHISPER_DECODERS["micro"], micro_whisper_sd(),
                      suppress_tokens=[1, 2, 7], max_initial_timestamp_index=50)


def _segments(res):
    return [[(s["start"], s["end"], s["tokens"].tolist()) for s in sb] for sb in res["segments"]]


def _both(monkeypatch, call):
    """call() with CBW_DEV_GREEDY 1 and 0; the device path must have been taken exactly when it is on"""
    from cbw.decoder import DecoderEngine
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("CBW_DEV_GREEDY", flag)
        used = []
        gw = DecoderEngine.greedy_windows
        monkeypatch.setattr(DecoderEngine, "greedy_windows", lambda self, *a, **k: used.append(1) or gw(self, *a, **k))
        out[flag] = call()
        monkeypatch.setattr(DecoderEngine, "greedy_windows", gw)
        assert bool(used) == (flag == "1")
    return out["1"], out["0"]


@pytest.mark.parametrize("timestamps", [False, True])
def test_generate_shortform_greedy_same_with_switch_on_and_off(monkeypatch, timestamps):
    w = _whisper()
    g = np.load(os.path.join(GOLDEN, "longform_micro.npz"))
    feats = torch.from_numpy(g["features"][None, :, :3000]).to(w.device)
    kws = lambda input_features, start_of_prev=False: [[w.tokens.startofprev, 1000, 1001, 1002]]   # noqa: E731
    on, off = _both(monkeypatch, lambda: w.generate(input_features=feats, task="transcribe", language="en", num_beams=1,
                                                    keyword_spotting=kws, max_new_tokens=40,
                                                    return_timestamps=timestamps))
    assert on.tolist() == off.tolist() and on.shape[1] > 4


def test_generate_longform_greedy_same_with_switch_on_and_off(monkeypatch):
    w = _whisper()
    g = np.load(os.path.join(GOLDEN, "longform_micro.npz"))
    feats = torch.from_numpy(g["features"][None]).to(w.device)
    on, off = _both(monkeypatch, lambda: w.generate(input_features=feats, task="transcribe", language="en", num_beams=1,
                                                    return_timestamps=True, condition_on_prev_tokens=False,
                                                    return_segments=True))
    assert on["sequences"].tolist() == off["sequences"].tolist()
    assert _segments(on) == _segments(off) and len(on["segments"][0]) >= 2


def test_generate_batched_longform_greedy_same_with_switch_on_and_off(monkeypatch):
    w = _whisper()
    g = np.load(os.path.join(GOLDEN, "longform_batched_micro.npz"))
    feats = torch.from_numpy(g["features"]).to(w.device)
    mask = torch.from_numpy(g["attention_mask"]).to(w.device)
    on, off = _both(monkeypatch, lambda: w.generate(input_features=feats, attention_mask=mask, task="transcribe",
                                                    language="en", num_beams=1, return_timestamps=True,
                                                    condition_on_prev_tokens=False, return_segments=True))
    assert on["sequences"].tolist() == off["sequences"].tolist()
    assert _segments(on) == _segments(off) and len(on["segments"]) == 3
