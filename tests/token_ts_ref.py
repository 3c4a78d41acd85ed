"""Float64 numpy restatement of cbw/token_timestamps.py (extract_token_timestamps and what it calls), the reference of
tests/test_host_token_ts.py and tests/test_gpu_token_ts.py: the normalisation over the positions, the reflect-padded
median along the frames, the head mean, the dynamic time warping with cbw_dtw's tie rules, the jump times and both
variants' row handling.  Everything is float64, the DTW's tables included."""
import numpy as np


def normalise(w):
    """w [heads, positions, frames] -> (w - mean) / population std over the positions"""
    w = np.asarray(w, dtype=np.float64)
    return (w - w.mean(axis=-2, keepdims=True)) / w.std(axis=-2, keepdims=True)


def reflect_windows(x, width):
    """x [..., F] -> [..., F, width]: the windows of the reflect-padded last axis (needs F > width // 2)"""
    pad = width // 2
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    return np.lib.stride_tricks.sliding_window_view(xp, width, axis=-1)


def median_filter(z, width):
    if width <= 0 or width % 2 != 1:
        raise ValueError("`filter_width` should be an odd number")
    if z.shape[-1] <= width // 2:
        return z
    return np.sort(reflect_windows(z, width), axis=-1)[..., width // 2]


def matrix(w, width):
    """-> (the negated head mean of the filtered normalised weights [positions, frames], z [heads, positions, frames])"""
    z = normalise(w)
    return -median_filter(z, width).mean(axis=0), z


def window_absmax(z, width):
    """A[t, f]: the largest |z| over the heads and over the filter window of frame f"""
    a = np.abs(z).max(axis=0)
    if z.shape[-1] <= width // 2:
        return a
    return reflect_windows(a, width).max(axis=-1)


def dtw(m):
    """cbw_dtw on float64 tables: +inf borders around cost 0, strict comparisons (the diagonal, then the row above,
    else the column to the left), swept by anti-diagonals -> (text_idx, time_idx) along the path"""
    m = np.asarray(m, dtype=np.float64)
    T, F = m.shape
    cost = np.full((T + 1, F + 1), np.inf)
    cost[0, 0] = 0.0
    trace = np.full((T + 1, F + 1), -1, dtype=np.int8)
    for d in range(T + F - 1):
        i = np.arange(max(0, d - F + 1), min(d, T - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i, j], cost[i, j + 1], cost[i + 1, j]
        t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2))
        cost[i + 1, j + 1] = m[i, j] + np.choose(t, [c0, c1, c2])
        trace[i + 1, j + 1] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j, ti, tj = T, F, [], []
    while i > 0 or j > 0:
        ti.append(i - 1)
        tj.append(j - 1)
        t = trace[i, j]
        if t != 2:
            i -= 1
        if t != 1:
            j -= 1
    return np.array(ti[::-1], dtype=np.int64), np.array(tj[::-1], dtype=np.int64)


def first_frames(text_idx, time_idx):
    """the time index at which the path enters each text row (the jumps extract_token_timestamps takes)"""
    jumps = np.pad(np.diff(text_idx), (1, 0), constant_values=1).astype(bool)
    return time_idx[jumps]


def extract(weights, width=7, time_precision=0.02, num_frames=None, variant="4.37", num_input_ids=None):
    """extract_token_timestamps -> float32 [positions + 1]"""
    w = np.asarray(weights, dtype=np.float64)
    T = w.shape[1]
    ts = np.zeros(T + 1, dtype=np.float32)
    if num_frames is not None:
        w = w[..., : int(num_frames) // 2]
    if variant == "5.x" and num_input_ids is not None:
        w = w[:, num_input_ids:]
        if w.shape[1] == 0:
            return ts
    text_idx, time_idx = dtw(matrix(w, width)[0])
    jump_times = first_frames(text_idx, time_idx) * time_precision
    if variant == "4.37":
        ts[1:] = jump_times
        return ts
    n0 = num_input_ids or 0
    return np.concatenate([np.zeros(n0), jump_times, jump_times[-1:]]).astype(np.float32)


def softmax_weights(n, T, F, seed):
    """softmax over the frames of N(0, 1) logits -> float32 [n, T, F]"""
    x = np.random.default_rng(seed).standard_normal((n, T, F))
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def planted_weights(n, T, F, seed):
    """An alignment to find: N(0, 1) logits plus 6 exp(-((f - c_t) / 3)^2 / 2) with c_t sorted uniform over the
    frames (shared by the heads), softmax over the frames -> float32 [n, T, F]"""
    g = np.random.default_rng(seed)
    c = np.sort(g.uniform(0, F, T))
    x = g.standard_normal((n, T, F)) + 6.0 * np.exp(-0.5 * ((np.arange(F)[None, :] - c[:, None]) / 3.0) ** 2)[None]
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
