"""CPU-only tests of the resampler in front of the log-mel (cbw_resample): the float64 restatement the GPU tests use
as their reference (tests/resample_ref.py) against an independent polyphase evaluation and for the signal properties
that make it a resampler at all; the C ABI entries (header, ctypes table, exported symbols) with the length and
workspace helpers, which are host arithmetic; and cbw.whisper.load_wav."""
import ctypes
import os
import re
import wave

import numpy as np
import pytest

import resample_ref as R
from conftest import REPO

RATES = (24000, 48000, 8000, 44100, 22050)


@pytest.mark.parametrize("orig", RATES)
def test_restatement_equals_upfirdn(orig):
    """y[f n + j] = sum_k xpad[f o + k] kernel[j][k] is one polyphase FIR: with the prototype h[j o - n (k - width)] =
    kernel[j][k] (a one-to-one index map, o and n being coprime), scipy.signal.upfirdn(h, x, up=n) evaluated at
    m o - min_index is y[m].  Measured on random inputs of 21 o + 5 samples: largest difference 8.9e-16 (22050 Hz,
    max|y| 3.3); the bound is 10x that."""
    from scipy.signal import upfirdn
    o, n, width, T = R.plan(orig, 16000)
    K = R.kernel(orig, 16000)
    assert K.shape == (n, T)
    idx = np.arange(n)[:, None] * o - n * (np.arange(T)[None, :] - width)
    assert np.unique(idx).size == n * T
    lo = int(idx.min())
    h = np.zeros(int(idx.max()) - lo + 1)
    h[idx - lo] = K
    x = np.random.default_rng(orig).standard_normal(21 * o + 5)
    full = upfirdn(h, x, up=n)
    y = R.resample(x, orig, 16000)
    assert y.size == -(-n * x.size // o)
    p = np.arange(y.size) * o - lo
    assert p.min() >= 0 and p.max() < full.size
    err = np.abs(y - full[p]).max()
    print(f"{orig} -> 16000: o {o} n {n} T {T}, max |restatement - upfirdn| {err:.3g}")
    assert err <= 9e-15


def test_plan_sizes():
    assert R.plan(24000, 16000) == (3, 2, 10, 23)
    assert R.plan(48000, 16000) == (3, 1, 19, 41)
    assert R.plan(8000, 16000) == (1, 2, 7, 15)
    assert R.plan(44100, 16000) == (441, 160, 17, 475)


# largest deviation from the 1 kHz sine at 16 kHz, 200 samples away from either end, measured over 0.25 s
SINE_DEV = {48000: 3.99e-4, 44100: 4.00e-4, 24000: 3.96e-4, 8000: 1.71e-4}
# largest output magnitude for a unit 10 kHz sine, same window
ALIAS_MAX = {48000: 5.43e-3, 44100: 5.43e-3, 24000: 5.49e-3}


@pytest.mark.parametrize("orig", sorted(SINE_DEV))
def test_sine_in_band_comes_out_as_the_same_sine(orig):
    """A 1 kHz unit sine sampled at `orig` comes out as the 1 kHz unit sine sampled at 16 kHz (same phase: no delay).
    Measured deviations away from the edges: 48 kHz 3.99e-4, 44.1 kHz 4.00e-4, 24 kHz 3.96e-4, 8 kHz 1.71e-4 (the
    pass-band ripple of a width-6 Hann-windowed sinc); asserted with a 2x margin."""
    t = np.arange(orig // 4) / orig
    y = R.resample(np.sin(2 * np.pi * 1000 * t), orig, 16000)
    want = np.sin(2 * np.pi * 1000 * np.arange(y.size) / 16000)
    dev = np.abs(y - want)[200:-200].max()
    print(f"{orig}: 1 kHz deviation {dev:.3g}")
    assert dev <= 2 * SINE_DEV[orig]


@pytest.mark.parametrize("orig", sorted(ALIAS_MAX))
def test_tone_above_nyquist_is_attenuated(orig):
    """A 10 kHz unit sine (above the 8 kHz Nyquist frequency of the output) is filtered out instead of aliasing to
    6 kHz.  Measured largest output magnitude away from the edges: 48 kHz 5.43e-3, 44.1 kHz 5.43e-3, 24 kHz 5.49e-3
    (-45 dB); asserted with a 2x margin."""
    t = np.arange(orig // 4) / orig
    y = R.resample(np.sin(2 * np.pi * 10000 * t), orig, 16000)
    mag = np.abs(y[200:-200]).max()
    print(f"{orig}: 10 kHz residue {mag:.3g}")
    assert mag <= 2 * ALIAS_MAX[orig]


@pytest.mark.parametrize("orig", RATES)
def test_output_length(orig):
    from cbw import _lib
    lib = _lib.load()
    o, n, _, _ = R.plan(orig, 16000)
    for length in (0, 1, o - 1, o, o + 1):
        want = -(-n * length // o)
        assert R.resample(np.ones(length), orig, 16000).size == want
        assert lib.cbw_resample_len(length, orig, 16000) == want


def test_header_symbols_and_ctypes_signatures():
    from cbw import _lib
    src = open(os.path.join(REPO, "include", "cbw.h")).read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    want = {"cbw_resample_len": ("int64_t", ["int64_t n", "int orig", "int new_"]),
            "cbw_resample_ws_bytes": ("int64_t", ["int orig", "int new_"]),
            "cbw_resample": ("int", ["const float* pcm", "int channels", "int64_t n", "int orig", "int new_", "float* out",
                                     "void* ws", "int64_t ws_bytes", "cbw_stream_t stream"])}
    lib = _lib.load()
    for name, (ret, params) in want.items():
        m = re.search(r"^" + ret + r"\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.M | re.S)
        assert m, f"include/cbw.h does not declare {name}"
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == params
        res, args = _lib.SIGNATURES[name]
        assert res is kinds[ret]
        assert list(args) == [ctypes.c_void_p if "*" in p or p.startswith("cbw_stream_t") else kinds[p.split()[0]]
                              for p in params]
        assert hasattr(lib, name)
    doc = src[src.index("resample + downmix"):src.index("int64_t cbw_resample_len")]
    assert "utils.py:179-184" in doc and "dataset.py:472-483" in doc


def test_length_and_workspace_helpers():
    from cbw import _lib
    lib = _lib.load()
    for orig, new in [(24000, 16000), (48000, 16000), (8000, 16000), (44100, 16000), (22050, 16000), (16000, 8000)]:
        o, n, _, T = R.plan(orig, new)
        assert lib.cbw_resample_ws_bytes(orig, new) == 4 * n * T
        assert lib.cbw_resample_len(12345, orig, new) == -(-n * 12345 // o)
    assert lib.cbw_resample_ws_bytes(16000, 16000) == 0 and lib.cbw_resample_len(77, 16000, 16000) == 77
    assert lib.cbw_resample_ws_bytes(44100, 16000) == 4 * 160 * 475 <= 4 * (1 << 20)
    # a table above the bound, bad rates, a negative length: refused with a message
    for call in (lambda: lib.cbw_resample_ws_bytes(16001, 16000), lambda: lib.cbw_resample_len(10, 16001, 16000),
                 lambda: lib.cbw_resample_ws_bytes(0, 16000), lambda: lib.cbw_resample_ws_bytes(16000, -1),
                 lambda: lib.cbw_resample_len(-1, 24000, 16000), lambda: lib.cbw_resample_len(2 ** 62, 8000, 16000)):
        assert call() == -1
        assert b"resample" in lib.cbw_last_error()
    # the argument checks of cbw_resample come before any GPU work: they refuse here, where there is none
    assert lib.cbw_resample(None, 1, 4, 24000, 16000, None, None, 0, None) == -1


def _write_wav(path, data, rate, width):
    """data int array [len, C]"""
    with wave.open(str(path), "wb") as w:
        w.setnchannels(data.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(data.astype({1: np.uint8, 2: "<i2", 4: "<i4"}[width]).tobytes())


def test_load_wav(tmp_path):
    from cbw.whisper import load_wav
    g = np.random.default_rng(0)
    mono = g.integers(-32768, 32768, (301, 1))
    mono[:2, 0] = (-32768, 32767)
    _write_wav(tmp_path / "m.wav", mono, 22050, 2)
    x, sr = load_wav(str(tmp_path / "m.wav"))
    assert sr == 22050 and tuple(x.shape) == (1, 301) and x.dtype.is_floating_point and x.element_size() == 4
    np.testing.assert_array_equal(x.numpy()[0], (mono[:, 0] / 32768.0).astype(np.float32))
    stereo = g.integers(-32768, 32768, (77, 2))
    _write_wav(tmp_path / "s.wav", stereo, 48000, 2)
    x, sr = load_wav(str(tmp_path / "s.wav"))
    assert sr == 48000 and tuple(x.shape) == (2, 77) and x.is_contiguous()
    np.testing.assert_array_equal(x.numpy(), (stereo.T / 32768.0).astype(np.float32))
    u8 = g.integers(0, 256, (50, 1))
    u8[:3, 0] = (0, 128, 255)
    _write_wav(tmp_path / "u.wav", u8, 8000, 1)
    x, sr = load_wav(str(tmp_path / "u.wav"))
    assert sr == 8000 and tuple(x.shape) == (1, 50)
    np.testing.assert_array_equal(x.numpy()[0], ((u8[:, 0] - 128) / 128.0).astype(np.float32))
    assert x.numpy()[0, 1] == 0.0
    i32 = g.integers(-2 ** 31, 2 ** 31, (9, 2))
    _write_wav(tmp_path / "l.wav", i32, 16000, 4)
    x, sr = load_wav(str(tmp_path / "l.wav"))
    np.testing.assert_array_equal(x.numpy(), (i32.T / 2147483648.0).astype(np.float32))
    with wave.open(str(tmp_path / "t.wav"), "wb") as w:      # 24-bit: not read, and said so
        w.setnchannels(1)
        w.setsampwidth(3)
        w.setframerate(16000)
        w.writeframes(b"\x00" * 30)
    with pytest.raises(ValueError, match="24-bit"):
        load_wav(str(tmp_path / "t.wav"))
