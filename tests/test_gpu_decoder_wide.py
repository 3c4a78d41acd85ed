"""cbw_decoder_step_wide and the lock-step drivers above 16 rows (a batch of short clips: up to 80 rows = 16 windows x
5 beams in one decode step).  Everything here is exact: a row of the wide step carries the bits of a step over its
window alone on a state of <= 16 rows, so the logits are compared with torch.equal and the searches return exactly what
the single-window searches (beam_search_dev, greedy_dev, sample_dev) return."""
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
def _engines(name):
    """(reference engine, lock-step engine) of one decoder, built once"""
    from cbw.decoder import DecoderEngine
    cfg, sd = synth.WHISPER_DECODERS[name], synth.synth_whisper_decoder_state_dict(name, seed=0)
    return DecoderEngine(cfg, sd), DecoderEngine(cfg, sd)


@pytest.mark.parametrize("W,nb", [(4, 5), (7, 5), (16, 5), (17, 1), (33, 1)])
@pytest.mark.parametrize("name", ["large-v3-2l", "micro"])
def test_step_wide_windows_match_single_window_steps(name, W, nb):
    """tests/test_gpu_decoder.py::test_step_rows_windows_match_single_window_steps above 16 rows: 20, 35 and 80 rows of
    5-beam windows and 17 and 33 one-row windows (a one-row tail group, a 3-row tail, full groups), each window on its
    own encoder slot and at its own position (prefixes of 5, 12 and 73 tokens: within the first 64-key chunk and past
    it), six steps with a beam reorder before the fourth (above 16 rows cbw_decoder_reorder gathers through the
    scratch rows instead of moving in place).  Every window's logits equal those of a step over that window alone."""
    ref_eng, b = _engines(name)
    cfg = synth.WHISPER_DECODERS[name]
    g = torch.Generator(device="cuda").manual_seed(21 + W)
    n_steps = 6
    encs = [torch.randn((1, 1500, cfg[1]), generator=g, device="cuda") for _ in range(min(W, 5))]
    enc_of = lambda w: encs[w % len(encs)] * (1.0 + 0.125 * (w // len(encs)))   # noqa: E731
    prefixes = [[50258, 50259, 50360] + [400 + 7 * i + w for i in range((2, 9, 70)[w % 3])] for w in range(W)]
    toks = np.random.default_rng(5).integers(0, 50000, (n_steps, W * nb))
    perm = [1, 1, 0, 4, 2] if nb == 5 else [0]
    ref = []
    for w in range(W):
        ref_eng.start(enc_of(w), nb)
        outs = [ref_eng.prefill(prefixes[w]).clone()]
        for i in range(n_steps):
            if i == 3:
                ref_eng.reorder(perm, len(prefixes[w]) + i)
            outs.append(ref_eng.step(toks[i, w * nb:(w + 1) * nb].tolist(), len(prefixes[w]) + i).clone())
        ref.append(outs)
    with pytest.raises(ValueError):
        b.start_windows(W, nb)   # more than 16 rows need max_rows
    b.start_windows(W, nb, max_rows=80)
    assert b._shape == (W * nb, W)
    for w in range(W):
        b.set_window(w, enc_of(w))
    for w in range(W):
        b.prefill_window(w, nb, prefixes[w])
    got = [[b._logits[w * nb:(w + 1) * nb, :b.vocab].clone()] for w in range(W)]
    for i in range(n_steps):
        if i == 3:
            b.reorder([p + w * nb for w in range(W) for p in perm], max(len(p) for p in prefixes) + i)
        lg = b.step_rows(torch.as_tensor(toks[i], dtype=torch.int32, device="cuda"))
        b._posr.add_(1)
        for w in range(W):
            got[w].append(lg[w * nb:(w + 1) * nb].clone())
    torch.cuda.synchronize()
    for w in range(W):
        for i, (x, y) in enumerate(zip(ref[w], got[w])):
            assert torch.isfinite(y).all()
            assert torch.equal(x, y), f"window {w} output {i}: the wide step differs from the window alone"


def test_step_wide_return_codes():
    from cbw import _lib
    _, b = _engines("micro")
    lib = b.lib
    b.start_windows(16, 5, max_rows=80)
    tok = torch.zeros((96,), dtype=torch.int32, device="cuda")
    pos = torch.zeros((96,), dtype=torch.int32, device="cuda")
    logits = torch.zeros((96, b.vpad), dtype=torch.float32, device="cuda")
    state = torch.empty(lib.cbw_decoder_state_bytes(b.h, 96, 96), dtype=torch.uint8, device="cuda")

    def step(B, Benc, pos_ptr=pos.data_ptr(), fn=lib.cbw_decoder_step_wide):
        return fn(b.h, tok.data_ptr(), pos_ptr, B, Benc, state.data_ptr(), state.numel(), logits.data_ptr(),
                  _lib.stream_handle())

    assert step(81, 81) == -1, "81 rows"
    assert step(96, 16) == -1, "96 rows"
    assert step(20, 3) == -1, "B % Benc != 0"
    assert step(18, 2) == -1, "9 rows per window"
    assert step(80, 16, None) == -1, "null pos_rows"
    assert step(0, 1) == -1, "no rows"
    assert step(17, 17, fn=lib.cbw_decoder_step_rows) == -1, "cbw_decoder_step_rows keeps refusing 17 rows"
    assert step(80, 16) == 0 and step(80, 10) == 0 and step(5, 1) == 0 and step(17, 17) == 0
    torch.cuda.synchronize()


def _jobs(cfg, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    encs = [torch.randn((1500, cfg[1]), generator=g, device="cuda") for _ in range(3)]
    jobs = []
    for i in range(n):
        prompt = [int(t) for t in rng.integers(220, 50000, (1, 37, 5, 12, 70, 20)[i % 6])]
        jobs.append(((encs[i % 3] * (1.0 + 0.25 * (i // 3))).contiguous(), [50361] + prompt + [50258, 50259, 50360]))
    return jobs


@pytest.mark.parametrize("timestamps", [True, False])
def test_beam_search_windows_wide_matches_beam_search_dev(timestamps):
    """Nine windows of 5 beams in one 45-row state (max_rows = 80), prompts of six lengths, each window with its own
    begin index, prompt length and max_length: exactly the sequence and score beam_search_dev gives each alone."""
    from cbw.timestamps import TimestampRules
    e, b = _engines("large-v3-2l")
    cfg = synth.WHISPER_DECODERS["large-v3-2l"]
    rules = TimestampRules(50365, 50364, EOS, 50) if timestamps else None
    bias = torch.zeros(cfg[0], device="cuda")
    bias[[1, 2, 7]] = float("-inf")
    begin = bias.clone()
    begin[[220, EOS]] = float("-inf")
    jobs = _jobs(cfg, 9, 31)
    lens = [len(p) for _, p in jobs]
    max_lens = [n + 10 + 2 * (i % 4) for i, n in enumerate(lens)]
    bias_ats = [(lambda pos, n=n: begin if pos == n else bias) for n in lens]
    want = []
    for (enc, prefix), n, m, ba in zip(jobs, lens, max_lens, bias_ats):
        e.start(enc[None], 5)
        want.append(e.beam_search_dev(prefix, 5, EOS, m, 10, ba, rules, n, 1, return_score=True))
    torch.cuda.synchronize()
    got = b.beam_search_windows(jobs, 5, EOS, max_lens, bias_ats, rules, lens, 1, return_score=True, max_rows=80)
    assert b._shape == (45, 9)
    for j, (w_, g_) in enumerate(zip(want, got)):
        assert list(g_[0]) == list(w_[0]), f"window {j}: sequence differs"
        assert g_[1] == w_[1], f"window {j}: score differs"
    narrow = b.beam_search_windows(jobs, 5, EOS, max_lens, bias_ats, rules, lens, 1, return_score=True)
    assert b._shape == (15, 3) and [(list(s), v) for s, v in narrow] == [(list(s), v) for s, v in got]
    with pytest.raises(ValueError, match="one value per window"):
        b.beam_search_windows(jobs, 5, EOS, max_lens[:3], bias_ats, rules, lens, 1, max_rows=80)


def test_cbw_dec_wide_switch_keeps_16_rows(monkeypatch):
    from cbw.decoder import row_cap
    assert row_cap(80, 5) == 80 and row_cap(80) == 80 and row_cap(16, 5) == 16 and row_cap(80, 9) == 16 and row_cap(200) == 80
    monkeypatch.setenv("CBW_DEC_WIDE", "0")
    assert row_cap(80, 5) == 16 and row_cap(80) == 16


@functools.lru_cache(maxsize=None)
def _micro_setup():
    e = torch.from_numpy(np.load(os.path.join(GOLDEN, "decoder_micro.npz"))["enc_out"]).to("cuda:0")
    V = synth.WHISPER_DECODERS["micro"][0]
    bias = torch.zeros(V, device="cuda:0")
    bias[[1, 2, 7]] = float("-inf")
    begin = bias.clone()
    begin[[220, EOS]] = float("-inf")
    windows = []
    for i in range(20):
        prompt = [] if i % 4 == 0 else [50361] + [1000 + 3 * i + j for j in range((2, 70, 9)[i % 3])]
        windows.append(((e * (1.0 - 0.03 * i)).contiguous(), prompt + SOT))
    limits = [len(p) + 5 + (7 * i) % 17 for i, (_, p) in enumerate(windows)]
    return windows, limits, bias, begin


@pytest.mark.parametrize("timestamps", [True, False])
def test_greedy_windows_twenty_slots_equal_each_window_alone(timestamps):
    from cbw.timestamps import TimestampRules
    eng, b = _engines("micro")
    windows, limits, bias, begin = _micro_setup()
    rules = TimestampRules(TB, NO_TS, EOS, 50) if timestamps else None
    alone = [eng.greedy_dev(enc, p, EOS, m, bias, begin, rules, return_logprobs=True)
             for (enc, p), m in zip(windows, limits)]
    got = b.greedy_windows(windows, EOS, limits, bias, begin, rules, return_logprobs=True, max_rows=80)
    assert b._shape == (20, 20)
    for i, ((seq, lps), (seq1, lps1)) in enumerate(zip(got, alone)):
        assert seq == seq1, f"window {i}: tokens differ from the window alone"
        assert np.array_equal(np.array(lps, np.float32), np.array(lps1, np.float32)), f"window {i}: log-probs differ"
    narrow = b.greedy_windows(windows, EOS, limits, bias, begin, rules, return_logprobs=True)
    assert b._shape == (16, 16) and narrow == got


def test_sample_windows_twenty_slots_equal_each_window_alone():
    from cbw.timestamps import TimestampRules
    eng, b = _engines("micro")
    windows, limits, bias, begin = _micro_setup()
    rules = TimestampRules(TB, NO_TS, EOS, 50)
    gen = lambda s: torch.Generator(device="cuda:0").manual_seed(s)   # noqa: E731
    alone, after = [], []
    for i, ((enc, p), m) in enumerate(zip(windows, limits)):
        g = gen(40 + i)
        alone.append(eng.sample_dev(enc, p, EOS, m, bias, begin, rules, 0.4, g))
        after.append(g)
    gens = [gen(40 + i) for i in range(20)]
    got = b.sample_windows(windows, EOS, limits, bias, begin, rules, 0.4, gens, max_rows=80)
    assert b._shape == (20, 20)
    for i, (a, w) in enumerate(zip(got, alone)):
        assert a[0] == w[0], f"window {i}: tokens differ from the window alone"
        assert np.array_equal(np.array(a[1], np.float32), np.array(w[1], np.float32)), f"window {i}: log-probs differ"
        assert torch.equal(gens[i].get_state(), after[i].get_state()), f"window {i}: generator state differs"
