"""float64 numpy restatement of the resampler cbw_resample implements (include/cbw.h, "resample + downmix"):
torchaudio.functional.resample with the sinc_interp_hann defaults (lowpass_filter_width 6, rolloff 0.99) as the
reference applies it after averaging the channels (src/utils.py:179-184, src/efficient_kws/dataset.py:472-483).
tests/test_host_resample.py checks it against scipy.signal.upfirdn and for its signal properties; the GPU tests use
it as their reference."""
import math

import numpy as np

LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99


def plan(orig: int, new: int):
    """(o, n, width, T): reduced rates, half width and taps per phase"""
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    base = min(o, n) * ROLLOFF
    width = int(math.ceil(LOWPASS_FILTER_WIDTH * o / base))
    return o, n, width, 2 * width + o


def kernel(orig: int, new: int) -> np.ndarray:
    """kernel[j][k], float64 [n, T]"""
    o, n, width, T = plan(orig, new)
    base = min(o, n) * ROLLOFF
    j = np.arange(n, dtype=np.float64)[:, None]
    k = np.arange(T, dtype=np.float64)[None, :]
    t = np.clip((-j / n + (k - width) / o) * base, -LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = np.cos(t * np.pi / LOWPASS_FILTER_WIDTH / 2) ** 2
    a = t * np.pi
    sinc = np.where(a == 0, 1.0, np.sin(a) / np.where(a == 0, 1.0, a))
    return sinc * window * (base / o)


def out_len(length: int, orig: int, new: int) -> int:
    o, n, _, _ = plan(orig, new)
    return -(-n * int(length) // o)


def resample(x, orig: int, new: int) -> np.ndarray:
    """x [len] or [C, len] -> float64 [ceil(n len / o)]: channel mean, then the polyphase filter over the padded
    signal (width zeros in front, width + o behind), frame f phase j at f n + j; orig == new returns the mean."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x.mean(axis=0)
    if int(orig) == int(new):
        return x.copy()
    o, n, width, T = plan(orig, new)
    h = kernel(orig, new)
    xpad = np.concatenate([np.zeros(width), x, np.zeros(width + o)])
    frames = (xpad.size - T) // o + 1
    idx = np.arange(frames)[:, None] * o + np.arange(T)[None, :]
    y = xpad[idx] @ h.T                                     # [frames, n]
    return y.reshape(-1)[: out_len(x.size, orig, new)]
