"""cbw_resample on the GPU (resample + downmix in front of the log-mel; include/cbw.h) against the float64 restatement
in tests/resample_ref.py, which tests/test_host_resample.py checks on the CPU: every rate pair and input length at
which the kernel takes another path (table in LDS or in global memory, one block or several, inputs shorter than the
filter), the fused downmix, the public path through extract_hidden_states / build_split_folder, and the argument
checks.

Tolerance of the filter: the reference uses the float64 coefficients and the same fp32 input samples, so the device
result differs by the rounding of each coefficient to fp32 (2^-24 relative), of the channel mean (C - 1 additions and
one division, each 2^-24) and of T fused multiply-adds (one rounding each): at most (T + 1 + C) 2^-24 max|x|
sum_k |kernel[j][k]| to first order.  The bound asserted is T 2^-23 max|x| sum_k |kernel[j][k]| per output (factor 1
on the issue's formula: twice T 2^-24, which covers the 1 + C as T >= 15)."""
import numpy as np
import pytest
import torch

import resample_ref as R
from cbw import synth

pytestmark = pytest.mark.gpu

PAIRS = [(24000, 16000), (48000, 16000), (8000, 16000), (44100, 16000)]
DEV = "cuda:0"


def _call(x_dev, orig, new, out=None, ws=None, channels=None, n=None):
    """cbw_resample through ctypes on a device tensor [len] or [C, len]; returns (rc, out)"""
    from cbw import _lib
    lib = _lib.load()
    C, length = (1, x_dev.shape[0]) if x_dev.dim() == 1 else tuple(x_dev.shape)
    C, length = (C if channels is None else channels), (length if n is None else n)
    if out is None:
        out = torch.full((max(int(lib.cbw_resample_len(max(length, 0), orig, new)), 0) + 8,), float("nan"),
                         dtype=torch.float32, device=x_dev.device)
    if ws is None:
        ws = torch.empty(max(int(lib.cbw_resample_ws_bytes(orig, new)), 256), dtype=torch.uint8, device=x_dev.device)
    with torch.cuda.device(x_dev.device):
        rc = lib.cbw_resample(x_dev.data_ptr(), C, length, orig, new, out.data_ptr(), ws.data_ptr(), ws.numel(),
                              _lib.stream_handle())
    return rc, out


def _lengths(orig, new):
    o, n, width, T = R.plan(orig, new)
    # the issue's six, plus one that spans several 256-output blocks at every rate pair
    return [1, o - 1, o + 1, width, 2 * width + o + 1, 64 * o + 7, 300 * o + 7]


def _bound(x, orig, new, out_len):
    o, n, width, T = R.plan(orig, new)
    s = np.abs(R.kernel(orig, new)).sum(axis=1)                    # [n]
    return T * 2.0 ** -23 * max(np.abs(x).max(), 1e-30) * s[np.arange(out_len) % n]


@pytest.mark.parametrize("orig,new", PAIRS)
def test_resample_matches_float64(orig, new):
    """Every length against the float64 restatement within the module's bound (measured maxima: docs/
    MEASUREMENT_LOG.md); the samples behind the output's end stay untouched; two calls give the same bits, and so does
    the same input at an odd offset of a larger buffer whose other samples are NaN (nothing outside [0, len) is
    read into the sum)."""
    from cbw import _lib
    lib = _lib.load()
    g = np.random.default_rng(orig)
    worst = 0.0
    for length in _lengths(orig, new):
        x = g.standard_normal(length).astype(np.float32)
        want_len = R.out_len(length, orig, new)
        assert lib.cbw_resample_len(length, orig, new) == want_len
        xd = torch.from_numpy(x).to(DEV) if length else torch.zeros(1, device=DEV)   # n = 0 still needs a pointer
        rc, out = _call(xd, orig, new, n=length)
        assert rc == 0, lib.cbw_last_error()
        got = out.cpu().numpy()
        assert np.isnan(got[want_len:]).all(), "wrote behind the output's end"
        if length == 0:
            continue
        ref = R.resample(x, orig, new)
        err = np.abs(got[:want_len].astype(np.float64) - ref)
        bound = _bound(x, orig, new, want_len)
        worst = max(worst, float((err / bound).max()))
        print(f"{orig}->{new} len {length}: max err {err.max():.3g}, bound there {bound[err.argmax()]:.3g}")
        assert (err <= bound).all(), f"len {length}: err {err.max():.3g} above the bound {bound[err.argmax()]:.3g}"
        rc, again = _call(xd, orig, new)
        assert rc == 0 and torch.equal(again[:want_len], out[:want_len])
        big = torch.full((length + 64,), float("nan"), dtype=torch.float32, device=DEV)
        big[37:37 + length] = xd
        rc, moved = _call(big[37:37 + length], orig, new)
        assert rc == 0 and torch.equal(moved[:want_len], out[:want_len])
    print(f"{orig}->{new}: largest err / bound {worst:.3g}")


def test_table_above_the_bound_is_refused():
    """16001 -> 16000 would need 16000 phases x 16015 taps: an error, not a launch"""
    from cbw import _lib
    lib = _lib.load()
    x = torch.zeros(100, device=DEV)
    out = torch.full((128,), 7.0, device=DEV)
    rc, out = _call(x, 16001, 16000, out=out)
    assert rc == -1 and b"CBW_RESAMPLE_MAX_TABLE" in lib.cbw_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    from cbw.whisper import resample
    with pytest.raises(ValueError, match="CBW_RESAMPLE_MAX_TABLE"):
        resample(x, 16001)


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("orig,new", [(24000, 16000), (44100, 16000)])
def test_downmix_is_fused(C, orig, new):
    """[C, len] with distinct channels = the float64 resampling of the float64 channel mean"""
    o, n, width, T = R.plan(orig, new)
    length = 64 * o + 7
    x = np.random.default_rng(C).standard_normal((C, length)).astype(np.float32)
    rc, out = _call(torch.from_numpy(x).to(DEV), orig, new)
    assert rc == 0
    ref = R.resample(x, orig, new)
    got = out.cpu().numpy()[:ref.size].astype(np.float64)
    assert np.isnan(out.cpu().numpy()[ref.size:]).all()
    assert (np.abs(got - ref) <= _bound(x.astype(np.float64).mean(axis=0), orig, new, ref.size)).all()


def test_same_rate_is_the_mean_or_a_copy():
    from cbw.whisper import resample
    g = np.random.default_rng(5)
    x = g.standard_normal((2, 1031)).astype(np.float32)
    rc, out = _call(torch.from_numpy(x).to(DEV), 16000, 16000)
    assert rc == 0
    got = out.cpu().numpy()
    mean = x.astype(np.float64).mean(axis=0)
    # one fp32 addition and one division by 2 (exact): half an ulp of the sum
    assert (np.abs(got[:1031] - mean) <= 2.0 ** -24 * np.abs(x).sum(axis=0)).all() and np.isnan(got[1031:]).all()
    mono = torch.from_numpy(x[0]).to(DEV)
    rc, out = _call(mono, 22050, 22050)
    assert rc == 0 and torch.equal(out[:1031], mono)
    # the Python entry: 16 kHz mono is passed through untouched (the same storage), a host array is moved
    assert resample(mono, 16000).data_ptr() == mono.data_ptr()
    assert torch.equal(resample(x[0], 16000), mono)
    assert torch.equal(resample(x[:1], 16000), mono)
    assert torch.equal(resample(x, 16000), out.new_tensor(got[:1031]))
    y = resample(x, 24000)
    assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == (R.out_len(1031, 24000, 16000),)
    assert (np.abs(y.cpu().numpy() - R.resample(x, 24000, 16000)) <= _bound(mean, 24000, 16000, y.numel())).all()


@pytest.fixture(scope="module")
def micro_encoder():
    from cbw.whisper import EncoderEngine
    return EncoderEngine(synth.WHISPER_CONFIGS["micro"], synth.synth_whisper_encoder_state_dict("micro", seed=0))


def test_extract_hidden_states_resamples_first(micro_encoder, tmp_path):
    """24 kHz stereo through extract_hidden_states(sample_rate=24000) = extract_hidden_states of the float64-resampled
    mono signal, within the encoder's own tolerance for normalised states (tests/test_gpu_encoder.py: atol 2.5e-2) and
    with the frame count of the resampled length; build_split_folder with one rate per keyword writes .bin files of
    those lengths."""
    from cbw import _lib
    from cbw.keyword_db import KeywordDatabase, build_split_folder, extract_hidden_states, hs_frames
    lib = _lib.load()
    eng, ids = micro_encoder, [1, 2, 3]
    stereo = np.stack([synth.synth_clip(3, seconds=1.25, sr=24000), synth.synth_clip(4, seconds=1.25, sr=24000)])
    hs = extract_hidden_states(stereo, eng, ids, sample_rate=24000)
    T = hs_frames(lib.cbw_resample_len(stereo.shape[1], 24000, 16000))
    assert tuple(hs.shape) == (3, T, eng.d_model) and stereo.shape[1] == 30000 and T == hs_frames(20000) == 63
    ref = extract_hidden_states(R.resample(stereo, 24000, 16000).astype(np.float32), eng, ids)
    np.testing.assert_allclose(hs.cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=2.5e-2)
    # treating the 24 kHz samples as 16 kHz ones (what happened before) is another, longer signal
    assert extract_hidden_states(stereo[0], eng, ids).shape[1] == hs_frames(stereo.shape[1]) != T
    phone = synth.synth_clip(5, seconds=0.9, sr=8000)
    build_split_folder(str(tmp_path), ["a", "b", "c"], {0: stereo, 2: phone}, eng, "tts", ids,
                       sample_rates={0: 24000, 2: 8000})
    db = KeywordDatabase.from_split_folder(str(tmp_path), "tts")
    assert db.ghost_mask.tolist() == [1.0, 0.0, 1.0]
    np.testing.assert_array_equal(db.hidden_states[0].numpy(), hs.cpu().numpy())
    assert tuple(db.hidden_states[2].shape) == (3, hs_frames(2 * phone.size), eng.d_model)
    with pytest.raises(ValueError, match="no rate"):
        build_split_folder(str(tmp_path), ["a", "b", "c"], {0: stereo, 2: phone}, eng, "tts", ids, sample_rates={0: 24000})
    build_split_folder(str(tmp_path), ["a"], {0: stereo}, eng, "one", ids, sample_rates=24000)
    one = KeywordDatabase.from_split_folder(str(tmp_path), "one")
    np.testing.assert_array_equal(one.hidden_states[0].numpy(), hs.cpu().numpy())


def test_default_rate_keeps_its_bits(micro_encoder):
    """sample_rate=16000 (the default) is log_mel + hidden_states on the samples as they are, bit for bit"""
    from cbw.keyword_db import extract_hidden_states, hs_frames
    from cbw.whisper import log_mel
    eng, ids = micro_encoder, [1, 2, 3]
    pcm = synth.synth_clip(3, seconds=2.37)
    _, pk = log_mel(torch.from_numpy(pcm).to(eng.device), eng.n_mel, packed=True)
    want = eng.hidden_states(pk, ids, normalize=True)[0][:, :hs_frames(pcm.size)].contiguous()
    assert torch.equal(extract_hidden_states(pcm, eng, ids), want)
    assert torch.equal(extract_hidden_states(pcm, eng, ids, sample_rate=16000), want)


def test_bad_arguments_return_invalid_without_launching():
    from cbw import _lib
    lib = _lib.load()
    x = torch.ones((2, 500), device=DEV)
    out = torch.full((1024,), 7.0, device=DEV)
    ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
    st = _lib.stream_handle()
    p, o, w = x.data_ptr(), out.data_ptr(), ws.data_ptr()
    need = lib.cbw_resample_ws_bytes(24000, 16000)
    assert need == 4 * 2 * 23
    cases = {
        "null pcm": (None, 1, 500, 24000, 16000, o, w, 4096, st),
        "null out": (p, 1, 500, 24000, 16000, None, w, 4096, st),
        "null ws": (p, 1, 500, 24000, 16000, o, None, 4096, st),
        "channels 0": (p, 0, 500, 24000, 16000, o, w, 4096, st),
        "n < 0": (p, 1, -1, 24000, 16000, o, w, 4096, st),
        "orig 0": (p, 1, 500, 0, 16000, o, w, 4096, st),
        "new -1": (p, 1, 500, 24000, -1, o, w, 4096, st),
        "ws too small": (p, 1, 500, 24000, 16000, o, w, need - 1, st),
        "ws misaligned": (p, 1, 500, 24000, 16000, o, w + 2, 4000, st),
        "table above the bound": (p, 1, 500, 16001, 16000, o, w, 4096, st),
    }
    for name, args in cases.items():
        assert lib.cbw_resample(*args) == -1, name
        assert lib.cbw_last_error(), name
        with pytest.raises(ValueError):
            _lib.check(-1, "cbw_resample")
    assert lib.cbw_resample(p, 2, 0, 24000, 16000, o, w, 4096, st) == 0          # n == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote to the output"
    assert lib.cbw_resample(p, 2, 500, 24000, 16000, o, w, need, st) == 0         # the exact workspace is enough
    torch.cuda.synchronize()
    assert bool((out[:334] != 7.0).all()) and bool((out[334:] == 7.0).all())
