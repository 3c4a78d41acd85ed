"""Token-level timestamps: transformers WhisperGenerationMixin._extract_token_timestamps, which the reference reaches
with ``return_token_timestamps`` (pba_whisper.py:333-336 in short-form; :439 -> generate_with_fallback ->
_postprocess_outputs in long-form).  The cross-attention weights of the checkpoint's alignment heads along a decoded
row are normalised over the decoder positions (mean / population std per head and frame), median-filtered along the
frames (odd width, reflect padding, sort-based median), averaged over the heads; dynamic time warping of the negated
matrix gives a monotone path, and each text position's first frame on the path, times ``time_precision``, is its time.

The weights come from libcbw (cbw_decoder_cross_attn_probs: a teacher-forced decoder pass over the row, one query row
per position -- what generate's per-step cross_attentions hold for the row that was kept, the beam's history being the
row's prefix); the DTW runs on the host in libcbw (cbw_dtw, the transformers loop step for step).
``extract_token_timestamps_dev`` is the same extraction with the matrix and the DTW on the GPU (cbw_align_matrix,
cbw_dtw_dev), ``extract_token_timestamps_batch_dev`` that for a batch of rows in one pass (cbw_align_matrix_batch,
cbw_dtw_dev_batch); ``extract_token_timestamps`` stays the reference they are tested against and their fallback.

``variant``:
  * "4.37" (the pinned transformers, requirements.txt:21): every decoder position is a DTW row; timestamps has the
    row's length, timestamps[0] = 0 and timestamps[1:] = the jump times.  Restated from the 4.37.2 text -- PARITY
    UNPINNED for this row handling (4.37.2 cannot run here); the shared core below is pinned.
  * "5.x" (the installed 5.15): the first ``num_input_ids`` positions are left out of the DTW and get 0, the last
    position repeats the last jump time -- pinned to transformers 5.15's function on the same weights
    (tests/test_host.py::test_token_timestamps_match_transformers)."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib


def median_filter(x: torch.Tensor, width: int) -> torch.Tensor:
    """transformers' _median_filter along the last dimension of a 3-D / 4-D tensor."""
    if width <= 0 or width % 2 != 1:
        raise ValueError("`filter_width` should be an odd number")
    pad = width // 2
    if x.shape[-1] <= pad:
        return x
    squeeze = x.dim() == 3
    y = torch.nn.functional.pad(x[None] if squeeze else x, (pad, pad, 0, 0), mode="reflect")
    y = y.unfold(-1, width, 1).sort()[0][..., pad]
    return y[0] if squeeze else y


def dtw(matrix: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """transformers' _dynamic_time_warping on a [rows, cols] cost matrix (libcbw cbw_dtw, host code) ->
    (text_indices, time_indices) along the path."""
    m = np.ascontiguousarray(matrix, dtype=np.float64)
    rows, cols = m.shape
    ti = np.empty(rows + cols, dtype=np.int32)
    tj = np.empty(rows + cols, dtype=np.int32)
    n = np.zeros(1, dtype=np.int32)
    lib = _lib.load()
    _lib.check(lib.cbw_dtw(m.ctypes.data, rows, cols, ti.ctypes.data, tj.ctypes.data, n.ctypes.data), "cbw_dtw")
    return ti[:n[0]].astype(np.int64), tj[:n[0]].astype(np.int64)


def _normalised_mean(w: torch.Tensor, median_filter_width: int) -> torch.Tensor:
    std = torch.std(w, dim=-2, keepdim=True, unbiased=False)
    mean = torch.mean(w, dim=-2, keepdim=True)
    return median_filter((w - mean) / std, median_filter_width).mean(dim=0)


def extract_token_timestamps(weights: torch.Tensor, median_filter_width: int = 7, time_precision: float = 0.02,
                             num_frames: Optional[int] = None, variant: str = "4.37",
                             num_input_ids: Optional[int] = None) -> torch.Tensor:
    """weights [heads, positions, frames]: the alignment heads' cross-attention weights of one decoded row (one query
    row per position; the row's last token has none) -> float32 [positions + 1], the row's token timestamps."""
    if variant not in ("4.37", "5.x"):
        raise ValueError(f"unknown variant {variant}")
    w = weights.float()
    T = w.shape[1]
    ts = torch.zeros(T + 1, dtype=torch.float32)
    if num_frames is not None:
        w = w[..., : int(num_frames) // 2]
    if variant == "5.x" and num_input_ids is not None:
        w = w[:, num_input_ids:]
        if w.shape[1] == 0:
            return ts
    matrix = _normalised_mean(w, median_filter_width)
    text_idx, time_idx = dtw(-matrix.cpu().double().numpy())
    jumps = np.pad(np.diff(text_idx), (1, 0), constant_values=1).astype(bool)
    jump_times = time_idx[jumps] * time_precision
    if variant == "4.37":
        ts[1:] = torch.tensor(jump_times)
        return ts
    n0 = num_input_ids or 0
    return torch.cat([torch.zeros(n0), torch.tensor(jump_times), torch.tensor([jump_times[-1]])]).float()


_dev_ws = _lib.Workspace()


def _per_window(v, n: int, name: str) -> list:
    """``v`` as one value per window: a list / tuple of n, or one value for all."""
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise ValueError(f"{name}: one value per window, or one for all")
        return list(v)
    return [v] * n


def extract_token_timestamps_dev(weights: torch.Tensor, median_filter_width: int = 7, time_precision: float = 0.02,
                                 num_frames: Optional[int] = None, variant: str = "4.37",
                                 num_input_ids: Optional[int] = None) -> torch.Tensor:
    """``extract_token_timestamps`` with the alignment matrix and the DTW on the GPU (cbw_align_matrix, cbw_dtw_dev on
    the current stream; one copy back of the jump frames and the degenerate flag): the same arguments, the same
    float32 tensor.  The host function itself answers where fewer than 2 positions are left, where the width is even
    or above 7 (its own error for an even one), and where a frame's variance over the positions is zero or not finite
    (the host path's NaNs are not restated).  weights [heads, positions, 1500], as cbw_decoder_cross_attn_probs writes
    them (fewer frames are padded to that row pitch first); at most 1024 positions."""
    if variant not in ("4.37", "5.x"):
        raise ValueError(f"unknown variant {variant}")
    host = lambda: extract_token_timestamps(weights, median_filter_width, time_precision, num_frames, variant,  # noqa: E731
                                            num_input_ids)
    width = int(median_filter_width)
    if width <= 0 or width % 2 != 1 or width > 7:
        return host()
    if weights.dim() != 3 or weights.shape[0] < 1 or not 1 <= weights.shape[-1] <= 1500:
        raise ValueError(f"expected weights [heads, positions, frames <= 1500], got {tuple(weights.shape)}")
    n, T_all, frames = weights.shape
    t0 = int(num_input_ids) if variant == "5.x" and num_input_ids is not None else 0
    T = T_all - t0
    F = frames if num_frames is None else min(frames, int(num_frames) // 2)
    if T < 2:
        return host()
    _lib.require_gpu()
    lib = _lib.load()
    nb = lib.cbw_token_ts_ws_bytes(T, F)
    if nb < 0:
        _lib.check(-1, "cbw_token_ts_ws_bytes")
    dev = weights.device if weights.is_cuda else torch.device(f"cuda:{torch.cuda.current_device()}")
    w = weights.to(device=dev, dtype=torch.float32)
    if frames < 1500:   # the kernels read rows of 1500 frames, cbw_decoder_cross_attn_probs' pitch
        w = torch.nn.functional.pad(w, (0, 1500 - frames))
    w = w.contiguous()
    matrix = torch.empty((T, F), dtype=torch.float32, device=dev)
    out = torch.empty(T + 1, dtype=torch.int32, device=dev)   # first_frame [T], then the flag
    with torch.cuda.device(dev):
        ws = _dev_ws.get(nb, dev)
        st = _lib.stream_handle()
        _lib.check(lib.cbw_align_matrix(w.data_ptr(), n, T_all, t0, T, F, width, matrix.data_ptr(),
                                        out.data_ptr() + 4 * T, ws.data_ptr(), ws.numel(), st), "cbw_align_matrix")
        _lib.check(lib.cbw_dtw_dev(matrix.data_ptr(), T, F, out.data_ptr(), None, None, None, ws.data_ptr(),
                                   ws.numel(), st), "cbw_dtw_dev")
    got = out.cpu().numpy()
    if got[T]:
        return host()
    jump_times = got[:T].astype(np.int64) * time_precision
    if variant == "4.37":
        ts = torch.zeros(T_all + 1, dtype=torch.float32)
        ts[1:] = torch.tensor(jump_times)
        return ts
    return torch.cat([torch.zeros(t0), torch.tensor(jump_times), torch.tensor([jump_times[-1]])]).float()


def _one_probs_buffer(ws: Sequence[torch.Tensor], dev) -> Tuple[torch.Tensor, list]:
    """The windows' weights as one f32 buffer of 1500-frame rows and each window's offset in floats: the tensors
    themselves where they are already views of one such buffer (DecoderEngine.cross_attn_probs_windows), else a copy."""
    if all(w.is_cuda and w.dtype == torch.float32 and w.shape[-1] == 1500 and w.is_contiguous() and
           w.untyped_storage().data_ptr() == ws[0].untyped_storage().data_ptr() for w in ws):
        base = min(w.data_ptr() for w in ws)
        end = max(w.data_ptr() + 4 * w.numel() for w in ws)
        flat = torch.empty(0, dtype=torch.float32, device=ws[0].device).set_(ws[0].untyped_storage(),
                                                                             (base - ws[0].untyped_storage().data_ptr()) // 4,
                                                                             ((end - base) // 4,))
        return flat, [(w.data_ptr() - base) // 4 for w in ws]
    parts, offs, at = [], [], 0
    for w in ws:
        w = w.to(device=dev, dtype=torch.float32)
        if w.shape[-1] < 1500:   # the kernels read rows of 1500 frames, cbw_decoder_cross_attn_probs' pitch
            w = torch.nn.functional.pad(w, (0, 1500 - w.shape[-1]))
        parts.append(w.reshape(-1))
        offs.append(at)
        at += parts[-1].numel()
    return torch.cat(parts), offs


def extract_token_timestamps_batch_dev(weights_list: Sequence[torch.Tensor], median_filter_width: int = 7,
                                       time_precision: float = 0.02, num_frames=None, variant="4.37",
                                       num_input_ids=None) -> list:
    """``extract_token_timestamps_dev`` for a batch of decoded rows: weights_list[i] [heads, positions_i, frames] (the
    same heads for all) -> the list of float32 tensors that the single-window function returns for each, with the
    alignment matrices in one launch and the DTW wavefronts side by side in another, in groups of at most 16 windows
    (cbw_align_matrix_batch, cbw_dtw_dev_batch: a window's arithmetic is the single-window kernels'), and one copy
    back of every window's jump frames and degenerate flag.  ``num_frames``, ``num_input_ids`` (and ``variant``) are
    one value for all windows or a list / tuple of one per window.  A window goes to the host function exactly where
    the single-window function sends it: fewer than 2 positions left, a width even or above 7, its degenerate flag."""
    N = len(weights_list)
    nf = _per_window(num_frames, N, "num_frames")
    ni = _per_window(num_input_ids, N, "num_input_ids")
    va = _per_window(variant, N, "variant")
    for v in va:
        if v not in ("4.37", "5.x"):
            raise ValueError(f"unknown variant {v}")
    host = lambda i: extract_token_timestamps(weights_list[i], median_filter_width, time_precision, nf[i], va[i],  # noqa: E731
                                              ni[i])
    width = int(median_filter_width)
    if width <= 0 or width % 2 != 1 or width > 7:
        return [host(i) for i in range(N)]
    out: list = [None] * N
    wins = []   # (index, T_all, t0, T, F) of the windows that stay on the device
    for i, w in enumerate(weights_list):
        if w.dim() != 3 or w.shape[0] < 1 or not 1 <= w.shape[-1] <= 1500:
            raise ValueError(f"expected weights [heads, positions, frames <= 1500], got {tuple(w.shape)}")
        if w.shape[0] != weights_list[0].shape[0]:
            raise ValueError("the windows of a batch share their alignment heads")
        T_all, frames = w.shape[1], w.shape[2]
        t0 = int(ni[i]) if va[i] == "5.x" and ni[i] is not None else 0
        T = T_all - t0
        F = frames if nf[i] is None else min(frames, int(nf[i]) // 2)
        if T < 2:
            out[i] = host(i)
        else:
            wins.append((i, T_all, t0, T, F))
    if not wins:
        return out
    _lib.require_gpu()
    lib = _lib.load()
    cuda = [weights_list[i] for i, *_ in wins if weights_list[i].is_cuda]
    dev = cuda[0].device if cuda else torch.device(f"cuda:{torch.cuda.current_device()}")
    probs, probs_off = _one_probs_buffer([weights_list[i] for i, *_ in wins], dev)
    M = len(wins)
    table = (_lib.TokenTsWindow * M)()
    m_at = ws_at = 0
    for k, (i, T_all, t0, T, F) in enumerate(wins):
        nb = lib.cbw_token_ts_ws_bytes(T, F)
        if nb < 0:
            _lib.check(-1, "cbw_token_ts_ws_bytes")
        table[k] = _lib.TokenTsWindow(T_all, t0, T, F, probs_off[k], m_at, ws_at)
        m_at += T * F
        ws_at += nb
    ld = max(T for _, _, _, T, _ in wins)
    n = weights_list[0].shape[0]
    matrix = torch.empty(m_at, dtype=torch.float32, device=dev)
    got = torch.empty(M * ld + M, dtype=torch.int32, device=dev)   # first_frame [M][ld], then the flags [M]
    with torch.cuda.device(dev):
        ws = _dev_ws.get(ws_at, dev)
        st = _lib.stream_handle()
        G = _lib.TOKEN_TS_MAX_WINDOWS
        for g in range(0, M, G):
            cnt = min(G, M - g)
            tab = ctypes.addressof(table) + g * ctypes.sizeof(_lib.TokenTsWindow)
            _lib.check(lib.cbw_align_matrix_batch(probs.data_ptr(), n, tab, cnt, width, matrix.data_ptr(),
                                                  got.data_ptr() + 4 * (M * ld + g), ws.data_ptr(), ws.numel(), st),
                       "cbw_align_matrix_batch")
            _lib.check(lib.cbw_dtw_dev_batch(matrix.data_ptr(), tab, cnt, got.data_ptr() + 4 * g * ld, ld,
                                             ws.data_ptr(), ws.numel(), st), "cbw_dtw_dev_batch")
    got = got.cpu().numpy()
    for k, (i, T_all, t0, T, F) in enumerate(wins):
        if got[M * ld + k]:
            out[i] = host(i)
            continue
        jump_times = got[k * ld:k * ld + T].astype(np.int64) * time_precision
        if va[i] == "4.37":
            ts = torch.zeros(T_all + 1, dtype=torch.float32)
            ts[1:] = torch.tensor(jump_times)
            out[i] = ts
        else:
            out[i] = torch.cat([torch.zeros(t0), torch.tensor(jump_times), torch.tensor([jump_times[-1]])]).float()
    return out


def alignment_pairs(alignment_heads: Sequence[Sequence[int]]) -> np.ndarray:
    """[[layer, head], ...] -> host int32 [2 n] (cbw_decoder_cross_attn_probs' heads)."""
    a = np.asarray([[int(l), int(h)] for l, h in alignment_heads], dtype=np.int32).reshape(-1)
    if a.size == 0:
        raise ValueError("alignment_heads is empty")
    return np.ascontiguousarray(a)
