"""CPU-only: what PBAWhisper.generate_batch refuses, before any GPU work (the engines are built on first use: none of
these calls builds one), an empty batch, and that the call leaves ``_controls`` alone."""
import pytest
import torch

from cbw import synth


def _whisper(dec="micro"):
    from model.pba_whisper import PBAWhisper
    sd = {"model.encoder." + k: v for k, v in synth.synth_whisper_encoder_state_dict("micro", seed=0).items()}
    sd.update({"model.decoder." + k: v for k, v in synth.synth_whisper_decoder_state_dict(dec, seed=0).items()})
    return PBAWhisper(synth.WHISPER_CONFIGS["micro"], synth.WHISPER_DECODERS[dec], sd)


def _no_engines(w):
    return w._encoder is None and w._decoder is None


def test_generate_batch_refusals_come_before_any_gpu_work():
    w = _whisper()
    assert not w.tokens.english_only
    n_mel = synth.WHISPER_CONFIGS["micro"][0]
    spotted = []
    spot = lambda input_features, start_of_prev=False: spotted.append(1) or [[] for _ in input_features]   # noqa: E731
    with pytest.raises(ValueError, match="3000"):
        w.generate_batch(torch.zeros((2, n_mel, 3001)), language="en", keyword_spotting=spot)
    with pytest.raises(NotImplementedError, match="language"):
        w.generate_batch(torch.zeros((2, n_mel, 3000)), keyword_spotting=spot)
    with pytest.raises(NotImplementedError, match="num_beams"):
        w.generate_batch(torch.zeros((2, n_mel, 3000)), language="en", num_beams=17, keyword_spotting=spot)
    with pytest.raises(ValueError):
        w.generate_batch(torch.zeros((n_mel, 3000)), language="en", keyword_spotting=spot)
    with pytest.raises(TypeError):   # the controls are arguments: nothing else is taken
        w.generate_batch(torch.zeros((2, n_mel, 3000)), language="en", repetition_penalty=1.1)
    assert not spotted and _no_engines(w)


def test_generate_batch_empty_batch_and_controls():
    w = _whisper()
    n_mel = synth.WHISPER_CONFIGS["micro"][0]
    w._controls = {"length_penalty": 2.0}   # as if set by an enclosing generate call
    assert w.generate_batch(torch.zeros((0, n_mel, 3000)), language="en", num_beams=5, length_penalty=0.5) == []
    assert w._controls == {"length_penalty": 2.0} and _no_engines(w)
    with pytest.raises(ValueError, match="3000"):
        w.generate_batch(torch.zeros((0, n_mel, 3001)), language="en")
    assert w._controls == {"length_penalty": 2.0}
