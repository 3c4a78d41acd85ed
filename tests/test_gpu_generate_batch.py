"""A batch of short clips in one call: PBAWhisper.generate_batch equals per-clip generate, CBWhisper.transcribe_batch /
test_step_batch equal the loop of forward / test_step calls, and CBW_DEC_WIDE=0 (16 rows everywhere) gives the same
results.  Micro checkpoints; the lock-step state reaches 6 x 5 = 30 rows at 5 beams."""
import functools
import random

import pytest
import torch

from cbw import synth

pytestmark = pytest.mark.gpu

PROMPT_LENS = (0, 1, 3, 40, 300, 7)   # text tokens after <|startofprev|>; 0: no prompt at all; 300 is cut to 225


@functools.lru_cache(maxsize=None)
def _whisper():
    from model.pba_whisper import PBAWhisper
    enc_cfg, dec_cfg = synth.WHISPER_CONFIGS["micro"], synth.WHISPER_DECODERS["micro"]
    sd = {"model.encoder." + k: v for k, v in synth.synth_whisper_encoder_state_dict("micro", seed=0).items()}
    sd.update({"model.decoder." + k: v for k, v in synth.synth_whisper_decoder_state_dict("micro", seed=0).items()})
    return PBAWhisper(enc_cfg, dec_cfg, sd, suppress_tokens=[1, 2, 7])


@functools.lru_cache(maxsize=None)
def _clips():
    from cbw.whisper import log_mel
    w = _whisper()
    mels = [log_mel(torch.from_numpy(synth.synth_clip(i)).to(w.device), w.encoder_config[0])[0] for i in range(6)]
    return torch.stack(mels)


def _prompts(w):
    return [[] if n == 0 else [w.tokens.startofprev] + [1000 + 13 * c + (i % 50) for i in range(n)]
            for c, n in enumerate(PROMPT_LENS)]


def _stub(w, calls):
    """keyword_spotting stub: clip c (of the six) always gets prompt c, whether it comes alone or in the batch."""
    prompts = _prompts(w)
    feats = _clips()

    def kws(input_features, start_of_prev=False):
        calls.append((tuple(input_features.shape), start_of_prev))
        out = []
        for f in input_features:
            c = next(i for i in range(6) if torch.equal(f, feats[i]))
            out.append(list(prompts[c]))
        return out
    return kws


@pytest.mark.parametrize("max_new_tokens", [12, None])
@pytest.mark.parametrize("timestamps", [False, True])
@pytest.mark.parametrize("num_beams", [1, 5])
def test_generate_batch_equals_per_clip_generate(num_beams, timestamps, max_new_tokens, monkeypatch):
    w = _whisper()
    feats = _clips()
    calls = []
    kw = dict(task="transcribe", language="english", return_timestamps=timestamps, num_beams=num_beams,
              max_new_tokens=max_new_tokens)
    want = [w.generate(input_features=feats[i:i + 1], keyword_spotting=_stub(w, []), **kw) for i in range(6)]
    got = w.generate_batch(feats, keyword_spotting=_stub(w, calls), **kw)
    assert calls == [((6, feats.shape[1], 3000), True)], "one keyword_spotting call over all clips"
    assert w.decoder._shape == (6 * num_beams, 6)
    assert w._controls == {}
    assert len(got) == 6
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == torch.long and a.dim() == 2 and a.shape[0] == 1
        assert a.tolist() == b.tolist(), f"clip {i} (prompt of {PROMPT_LENS[i]} tokens): differs from generate"
    if max_new_tokens:
        assert all(g.shape[1] <= 4 + 12 for g in got)
    monkeypatch.setenv("CBW_DEC_WIDE", "0")
    narrow = w.generate_batch(feats, keyword_spotting=_stub(w, []), **kw)
    assert w.decoder._shape[0] <= 16
    assert [a.tolist() for a in narrow] == [a.tolist() for a in got], "CBW_DEC_WIDE=0 gives the same results"


def test_generate_batch_short_clip_is_padded_like_generate():
    w = _whisper()
    feats = _clips()[:3, :, :2000].contiguous()
    kw = dict(task="transcribe", language="english", num_beams=5, max_new_tokens=8)
    want = [w.generate(input_features=feats[i:i + 1], **kw) for i in range(3)]
    got = w.generate_batch(feats, **kw)
    assert [a.tolist() for a in got] == [b.tolist() for b in want]


@pytest.fixture(scope="module")
def cbwhisper(tmp_path_factory):
    """CBWhisper as tests/test_gpu_cbwhisper.py builds it: three keywords planted in clip 0's hidden states."""
    import oracle.cbwhisper as ocb
    import oracle.mel as omel
    from model.cb_whisper import CBWhisper
    enc_sd = synth.synth_whisper_encoder_state_dict("micro-deep", 0)
    mels = [omel.log_mel(synth.synth_clip(i), 80) for i in range(3)]
    u = ocb.utterance_hs(enc_sd, mels[0], synth.WHISPER_CONFIGS["micro-deep"][3])
    khs = {0: u[:, 100:140], 2: u[:, 700:725], 4: u[:, 1200:1260]}
    paths = synth.write_cbwhisper_fixture(str(tmp_path_factory.mktemp("cbwbatch")), keyword_hs=khs, cnn_class1_shift=-2.5)

    def build(**kw):
        args = dict(dataset="acl", split="test", root=paths["acl"], kw_type="tts", encoder_ckpt=paths["encoder"],
                    whisper_ckpt=paths["whisper"], kws_ckpt=paths["kws_ckpt"], language="English", prompt=True,
                    oracle="kws", kws_features_size=(150, 750), keywords_per_group=100,
                    keyword_prompt_prepend="The topic of today's speech is, ah, ",
                    keyword_prompt_append=". Okay, then I'll continue.", keyword_separator=", ")
        args.update(kw)
        cb = CBWhisper(**args)
        gen, gen_b = cb.whisper.generate, cb.whisper.generate_batch
        cb.whisper.generate = lambda *a, **k: gen(*a, max_new_tokens=8, **k)
        cb.whisper.generate_batch = lambda *a, **k: gen_b(*a, max_new_tokens=8, **k)
        return cb
    import numpy as np
    return build, torch.from_numpy(np.stack(mels)).cuda()


def test_transcribe_batch_equals_forward_loop(cbwhisper, monkeypatch):
    build, feats = cbwhisper
    cb = build()
    want, spotted = [], []
    for i in range(3):
        want.append(cb.forward(feats[i:i + 1], None))
        spotted += cb.last_spotted
    got = cb.transcribe_batch(feats)
    assert got == want and all(isinstance(t, str) for t in got)
    assert cb.last_spotted == spotted, "every clip its own keywords, not the union"
    assert spotted[0] == ["alpha", "charlie", "echo"]
    monkeypatch.setenv("CBW_DEC_WIDE", "0")
    assert cb.transcribe_batch(feats) == want
    assert cb.transcribe_batch(feats[:0]) == []
    with pytest.raises(ValueError):
        cb.transcribe_batch(feats, oracles=[["alpha"]])


@pytest.mark.parametrize("oracle", ["gold", "random", "kws"])
def test_test_step_batch_equals_test_step_loop(cbwhisper, oracle):
    build, feats = cbwhisper
    cb = build(oracle=oracle)
    K = len(cb.keywords)
    labels = [[0, 2], [1], []]

    def batch(i):
        lab = torch.zeros(K, dtype=torch.long)
        lab[labels[i]] = 1
        return {"utterance": {"features": feats[i:i + 1], "attention_mask": None}, "transcript": f"t{i}",
                "speaker": f"s{i}", "hotword_labels": [lab], "keywords": [cb.keywords[j] for j in labels[i]]}

    cb.on_test_epoch_start()
    r1, r2 = random.Random(3), random.Random(3)
    for i in range(3):
        cb.test_step(batch(i), i, rng=r1)
    want = cb.test_step_outputs
    cb.on_test_epoch_start()
    out = cb.test_step_batch([batch(i) for i in range(3)], rng=r2)
    assert cb.test_step_outputs == want and out == want and len(want) == 3
    assert r1.random() == r2.random(), "rng consumed as the sequential calls consume it"
