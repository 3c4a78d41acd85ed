"""Whisper decoder engine over libcbw (cbw_decoder_*): cross-KV precompute once per
30 s window, one decode step per token with a self-attention KV cache, beam reorder,
log-softmax + top-k with additive suppression bias.  Drives cbw.generate."""
from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib


WIDE_ROWS = 80   # CBW_DEC_WIDE_ROWS (cbw.h): the rows of one cbw_decoder_step_wide, 16 windows x 5 beams


def dec_wide() -> bool:
    """CBW_DEC_WIDE, read at call time: lock-step states of more than 16 rows (cbw_decoder_step_wide) where a caller
    asks for them with ``max_rows``; 0 keeps 16 rows everywhere.  On by default: at 80 rows a row of the large-v3 step
    costs 0.077 ms against 0.185 ms at 15 rows (docs/MEASUREMENT_LOG.md)."""
    return os.environ.get("CBW_DEC_WIDE", "1") != "0"


def row_cap(max_rows: int, beams: int = 1) -> int:
    """The rows a lock-step state may have for a caller's ``max_rows``: 16, or up to WIDE_ROWS under CBW_DEC_WIDE when
    the windows have at most 8 rows each (cbw_decoder_step_wide's limit)."""
    if int(max_rows) <= 16 or beams > 8 or not dec_wide():
        return min(16, max(1, int(max_rows)))
    return min(WIDE_ROWS, int(max_rows))


def _per_window(v, n: int, name: str) -> list:
    """``v`` as one value per window: a list / tuple of n, or one value for all."""
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise ValueError(f"{name}: one value per window, or one for all")
        return list(v)
    return [v] * n


class DecoderEngine:
    def __init__(self, config: Tuple[int, int, int, int, int], state_dict: Dict[str, object],
                 device: Optional[torch.device] = None, max_len: int = 448):
        """config = (vocab, d_model, n_layers, n_heads, ffn_dim); HF WhisperDecoder names
        (a leading `model.decoder.` is stripped)."""
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.vocab, self.d_model, self.n_layers, self.n_heads, self.ffn = config
        self.max_len = max_len
        cfg = _lib.DecoderConfig(self.vocab, self.d_model, self.n_layers, self.n_heads, self.ffn, max_len)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cbw_decoder_create(ctypes.byref(cfg), ctypes.byref(h)), "cbw_decoder_create")
            self.h = h
            for name, v in state_dict.items():
                for pre in ("model.decoder.", "decoder."):
                    if name.startswith(pre):
                        name = name[len(pre):]
                if name == "proj_out.weight" or not (name.startswith("layers.") or name.startswith("embed") or
                                                     name.startswith("layer_norm")):
                    continue
                a = np.ascontiguousarray(v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v),
                                         dtype=np.float32)
                _lib.check(self.lib.cbw_decoder_set_param(self.h, name.encode(), a.ctypes.data, a.size),
                           f"cbw_decoder_set_param({name})")
            _lib.check(self.lib.cbw_decoder_finalize(self.h), "cbw_decoder_finalize")
        self.vpad = self.lib.cbw_decoder_vocab_padded(self.h)
        self._state = None
        self._shape = None
        self._tok = self._logits = None

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            try:
                self.lib.cbw_decoder_destroy(h)
            except Exception:
                pass

    # ------------------------------------------------------------------ window setup
    def start(self, enc_out: torch.Tensor, rows: int):
        """enc_out f32 [Benc, 1500, D] (post-LN encoder output); rows = Benc * beams."""
        enc_out = enc_out.to(self.device, torch.float32).contiguous()
        Benc = enc_out.shape[0]
        nb = self.lib.cbw_decoder_state_bytes(self.h, rows, Benc)
        if nb < 0:
            raise ValueError("rows must be a positive multiple of the encoder batch")
        if self._state is None or self._state.numel() < nb:
            self._state = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._shape = (rows, Benc)
        if self._tok is None or self._tok.numel() != rows:
            self._tok = torch.empty((rows,), dtype=torch.int32, device=self.device)
            self._logits = torch.empty((rows, self.vpad), dtype=torch.float32, device=self.device)
        self._rows = torch.empty((rows,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cbw_decoder_cross_kv(self.h, enc_out.data_ptr(), Benc, self._state.data_ptr(),
                                                     self._state.numel(), rows, _lib.stream_handle()),
                       "cbw_decoder_cross_kv")

    # ------------------------------------------------------------------ several windows in one step
    def start_windows(self, windows: int, beams: int, max_rows: int = 16):
        """State for ``windows`` windows of ``beams`` rows each decoded in lock step (cbw_decoder_step_rows):
        window w's rows are [w beams, (w + 1) beams) and attend to encoder slot w; every row at its own position
        (self._posr, device int32 [rows]).  ``max_rows`` = 80 allows up to 80 rows (of at most 8 per window) and up
        to 80 encoder slots, stepped by cbw_decoder_step_wide.  Memory: a slot's cross-attention K/V is n_layers x
        1500 x d_model x 2 x 2 bytes (large-v3: 245 MB per window, 3.9 GB for 16, 19.7 GB for 80 one-row windows) and
        a row's self-attention K/V n_layers x max_len x d_model x 2 x 2 bytes (large-v3: 73 MB, 5.9 GB at 80 rows)."""
        rows = windows * beams
        cap = min(WIDE_ROWS, max(16, int(max_rows)))
        nb = self.lib.cbw_decoder_state_bytes(self.h, rows, windows)
        if nb < 0 or rows > cap or (rows > 16 and beams > 8):
            raise ValueError(f"windows x beams must be <= {cap} rows" + (", of <= 8 per window" if rows > 16 else ""))
        if self._state is None or self._state.numel() < nb:
            self._state = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._shape = (rows, windows)
        self._tok = torch.zeros((rows,), dtype=torch.int32, device=self.device)
        self._logits = torch.zeros((rows, self.vpad), dtype=torch.float32, device=self.device)
        self._posr = torch.zeros((rows,), dtype=torch.int32, device=self.device)
        self._rows = torch.arange(rows, dtype=torch.int32, device=self.device)

    def set_window(self, slot: int, enc_out: torch.Tensor):
        """Encoder slot ``slot``'s cross-attention K/V from enc_out f32 [1500, D] (or [1, 1500, D])."""
        rows, windows = self._shape
        enc_out = enc_out.to(self.device, torch.float32).reshape(1500, self.d_model).contiguous()
        _lib.check(self.lib.cbw_decoder_cross_kv_slot(self.h, enc_out.data_ptr(), slot, windows, self._state.data_ptr(),
                                                      self._state.numel(), rows, _lib.stream_handle()),
                   "cbw_decoder_cross_kv_slot")

    def prefill_window(self, slot: int, beams: int, prefix: Sequence[int]):
        """cbw_decoder_prefill into window ``slot``'s rows: their K/V at positions 0..len-1, the last token's logits
        in each of its rows, its rows' positions set to len(prefix)."""
        rows, windows = self._shape
        r0 = slot * beams
        toks = torch.as_tensor(list(prefix), dtype=torch.int32).to(self.device)
        _lib.check(self.lib.cbw_decoder_prefill_rows(self.h, toks.data_ptr(), len(prefix), slot, r0, beams, rows,
                                                     windows, self._state.data_ptr(), self._state.numel(),
                                                     self._logits[r0].data_ptr(), _lib.stream_handle()),
                   "cbw_decoder_prefill_rows")
        self._logits[r0 + 1:r0 + beams].copy_(self._logits[r0:r0 + 1].expand(beams - 1, -1))
        self._posr[r0:r0 + beams].fill_(len(prefix))

    def step_rows(self, tokens: torch.Tensor):
        """One step of every row, row r at position self._posr[r] (tokens: device int32 [rows])."""
        rows, windows = self._shape
        # more than 16 rows: the same step as row groups of 16 (cbw_decoder_step_wide), each row's bits unchanged
        step, name = (self.lib.cbw_decoder_step_wide, "cbw_decoder_step_wide") if rows > 16 else \
            (self.lib.cbw_decoder_step_rows, "cbw_decoder_step_rows")
        _lib.check(step(self.h, tokens.data_ptr(), self._posr.data_ptr(), rows, windows, self._state.data_ptr(),
                        self._state.numel(), self._logits.data_ptr(), _lib.stream_handle()), name)
        return self._logits[:, : self.vocab]

    def step(self, tokens: Sequence[int], pos: int) -> torch.Tensor:
        rows, Benc = self._shape
        self._tok.copy_(torch.as_tensor(list(tokens), dtype=torch.int32))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cbw_decoder_step(self.h, self._tok.data_ptr(), pos, rows, Benc, self._state.data_ptr(),
                                                 self._state.numel(), self._logits.data_ptr(), _lib.stream_handle()),
                       "cbw_decoder_step")
        return self._logits[:, : self.vocab]

    def prefill(self, prefix: Sequence[int]) -> torch.Tensor:
        """The forced prefix in one pass (cbw_decoder_prefill): K/V of positions 0..len-1 in every beam row,
        the last token's logits copied to every row of the step logits; the next step() is at pos = len."""
        rows, Benc = self._shape
        toks = torch.as_tensor(list(prefix), dtype=torch.int32).to(self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cbw_decoder_prefill(self.h, toks.data_ptr(), len(prefix), rows, Benc,
                                                    self._state.data_ptr(), self._state.numel(),
                                                    self._logits.data_ptr(), _lib.stream_handle()),
                       "cbw_decoder_prefill")
        self._logits[1:].copy_(self._logits[:1].expand(rows - 1, -1))
        return self._logits[:, : self.vocab]

    def cross_attn_probs(self, tokens: Sequence[int], heads: np.ndarray) -> torch.Tensor:
        """Cross-attention probabilities of the (layer, head) pairs ``heads`` (host int32 [2 n],
        cbw.token_timestamps.alignment_pairs) along ``tokens`` teacher-forced against the encoder output of the last
        start() (cbw_decoder_cross_attn_probs; cache row 0 is overwritten) -> f32 [n, len(tokens), 1500]."""
        rows, Benc = self._shape
        T = len(tokens)
        n = heads.size // 2
        toks = torch.as_tensor(list(tokens), dtype=torch.int32).to(self.device)
        probs = torch.empty((n, T, 1500), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cbw_decoder_cross_attn_probs(self.h, toks.data_ptr(), T, heads.ctypes.data, n, rows, Benc,
                                                             self._state.data_ptr(), self._state.numel(),
                                                             probs.data_ptr(), _lib.stream_handle()),
                       "cbw_decoder_cross_attn_probs")
        return probs

    def cross_attn_probs_windows(self, windows: Sequence[Tuple[torch.Tensor, Sequence[int]]],
                                 heads: np.ndarray) -> List[torch.Tensor]:
        """``cross_attn_probs`` for several windows, windows = [(enc_out [1500, D], row tokens)]: one device tensor
        f32 [n, len(tokens_i), 1500] per window, views of one buffer.  Groups of at most 16 windows share a lock-step
        state of one row per window (start_windows(g, 1): whatever state the engine held is gone): window w of a group
        is encoder slot w and cache row w, set_window then one cbw_decoder_cross_attn_probs_slot call -- the windows'
        rows are not joined into one pass, whose GEMM tiling would follow the row count, so each window's
        probabilities are those of start() + cross_attn_probs() on it alone, bit for bit.  No host synchronisation."""
        n = heads.size // 2
        lens = [len(t) for _, t in windows]
        if min(lens, default=1) < 1:
            raise ValueError("cross_attn_probs_windows: an empty row")
        toks = torch.as_tensor([int(t) for _, row in windows for t in row], dtype=torch.int32).to(self.device)
        probs = torch.empty(n * 1500 * sum(lens), dtype=torch.float32, device=self.device)
        out, at = [], 0
        with torch.cuda.device(self.device):
            for g0 in range(0, len(windows), 16):
                group = windows[g0:g0 + 16]
                self.start_windows(len(group), 1)
                rows, slots = self._shape
                for slot, (enc_out, row) in enumerate(group):
                    T = len(row)
                    view = probs[n * 1500 * at:n * 1500 * (at + T)].view(n, T, 1500)
                    self.set_window(slot, enc_out)
                    _lib.check(self.lib.cbw_decoder_cross_attn_probs_slot(
                        self.h, toks.data_ptr() + 4 * at, T, heads.ctypes.data, n, slot, slot, rows, slots,
                        self._state.data_ptr(), self._state.numel(), view.data_ptr(), _lib.stream_handle()),
                        "cbw_decoder_cross_attn_probs_slot")
                    out.append(view)
                    at += T
        return out

    def reorder(self, src_rows: Sequence[int], length: int):
        rows, Benc = self._shape
        self._rows.copy_(torch.as_tensor(list(src_rows), dtype=torch.int32))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cbw_decoder_reorder(self.h, self._rows.data_ptr(), rows, Benc, length,
                                                    self._state.data_ptr(), self._state.numel(),
                                                    _lib.stream_handle()), "cbw_decoder_reorder")

    def _timestamp_rules(self, logits_ptr: int, rows: int, bias: Optional[torch.Tensor], st: torch.Tensor, rules,
                         out: torch.Tensor, stream: int):
        """The one cbw_timestamp_rules call: ``rows`` rows of logits at ``logits_ptr`` with rule states ``st``
        (int32 [rows, 4]) -> out f32 [rows, V] = the shared ``bias`` + the rows' timestamp masks."""
        _lib.check(self.lib.cbw_timestamp_rules(logits_ptr, rows, self.vocab, self.vpad, _lib.ptr(bias), st.data_ptr(),
                                                rules.timestamp_begin, rules.no_timestamps, rules.eos,
                                                rules.max_initial, out.data_ptr(), stream), "cbw_timestamp_rules")

    def _logprob_topk(self, logits_ptr: int, rows: int, bias: Optional[torch.Tensor], bias_ld: int, k: int,
                      lp: torch.Tensor, idx: torch.Tensor, stream: int):
        """The one cbw_logprob_topk call: top ``k`` of log_softmax(logits) + bias per row (bias [V] shared with
        bias_ld 0, or [rows, bias_ld]) -> lp f32 / idx int32 [rows, k]."""
        _lib.check(self.lib.cbw_logprob_topk(logits_ptr, rows, self.vocab, self.vpad, _lib.ptr(bias), bias_ld, k,
                                             lp.data_ptr(), idx.data_ptr(), stream), "cbw_logprob_topk")

    def topk(self, k: int, bias: Optional[torch.Tensor] = None, bias_ld: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """HF beam-search scores log_softmax(logits) + bias (bias [V] shared, or [rows, bias_ld])."""
        rows = self._shape[0]
        lp = torch.empty((rows, k), dtype=torch.float32, device=self.device)
        idx = torch.empty((rows, k), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._logprob_topk(self._logits.data_ptr(), rows, bias, bias_ld, k, lp, idx, _lib.stream_handle())
        return lp.cpu().numpy(), idx.cpu().numpy()

    def timestamp_bias(self, rules, sampled_rows, bias: Optional[torch.Tensor], states=None) -> torch.Tensor:
        """Per-row masks of WhisperTimeStampLogitsProcessor on top of the shared bias
        (cbw_timestamp_rules): -> f32 [rows, V].  ``states`` overrides the rows' rule states (TimestampRules.state)."""
        rows = self._shape[0]
        if states is None:
            states = [rules.state(s) for s in sampled_rows]
        st = torch.tensor(states, dtype=torch.int32).to(self.device)
        out = torch.empty((rows, self.vocab), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._timestamp_rules(self._logits.data_ptr(), rows, bias, st, rules, out, _lib.stream_handle())
        return out

    def beam_search_dev(self, prefix: Sequence[int], num_beams: int, eos: int, max_length: int, k: int,
                        bias_at: callable, rules=None, begin_index: int = 0, decoder_prompt_len: int = 1,
                        length_penalty: float = 1.0, check_every: int = 8, return_score: bool = False):
        """cbw.generate.beam_search with the bookkeeping on the GPU, for the one window of the
        last start(): one _BeamWindow at slot 0.  Per token its score() (timestamp rules from a device-side state,
        log-softmax + top-k, the next-beam choice of cbw_beam_select), the KV reorder by the device parent rows and
        the decode step, both reading the step's log row in place, are enqueued without a host round trip; every
        ``check_every`` tokens its replay() copies the logged candidates back once and runs them through the same
        BeamProcess the host search runs, which finds the end (EOS hypotheses, early stop, max_length) and the
        result.  Steps enqueued past the end are discarded.
        Returns None when the engine cannot run it (Benc != 1, k or rows > 16): use beam_search."""
        rows, Benc = self._shape
        if Benc != 1 or rows != num_beams or rows > 16 or k > 16 or k != 2 * num_beams or len(prefix) < 2:
            return None
        w = _BeamWindow(self, 0, 0, prefix, num_beams, k, eos, max_length, rules, begin_index, decoder_prompt_len,
                        length_penalty)
        stream = _lib.stream_handle()
        self.prefill(prefix)
        with torch.cuda.device(self.device):
            while not w.bp.finished:
                w.score(bias_at, stream)
                if w.stopped:
                    break
                _lib.check(self.lib.cbw_decoder_reorder(self.h, w.next_rows().data_ptr(), rows, Benc, w.pos,
                                                        self._state.data_ptr(), self._state.numel(), stream),
                           "cbw_decoder_reorder")
                _lib.check(self.lib.cbw_decoder_step(self.h, w.next_tokens().data_ptr(), w.pos, rows, Benc,
                                                     self._state.data_ptr(), self._state.numel(),
                                                     self._logits.data_ptr(), stream), "cbw_decoder_step")
                w.pos += 1
                if w.s - w.replayed >= check_every:
                    w.replay()
            w.replay()   # what is logged since the last replay (nothing when that one found the end)
        return w.result(return_score)

    def beam_search_windows(self, windows: Sequence[Tuple[torch.Tensor, Sequence[int]]], num_beams: int, eos: int,
                            max_length: int, bias_at: callable, rules=None, begin_index: int = 0,
                            decoder_prompt_len: int = 1, length_penalty: float = 1.0, check_every: int = 8,
                            return_score: bool = False, max_rows: int = 16) -> List:
        """Beam search with the bookkeeping on the GPU for several windows at once (the windows of one iteration of the
        batched long-form loop, pba_whisper.py:425-442: HF 4.37.2 runs their beam searches as one batch, each batch
        element's scorer independent of the others): windows = [(enc_out f32 [1500, D] post-LN, decoder prefix)], decoded in lock step
        on one decoder state of ``16 // num_beams`` slots (``max_rows`` = 80 under CBW_DEC_WIDE: ``80 // num_beams``,
        see start_windows) -- every row at its own position, each window on its own
        encoder slot (cbw_decoder_step_rows), windows admitted into slots as earlier ones finish.  ``max_length``,
        ``begin_index``, ``decoder_prompt_len`` and ``bias_at`` may each be a list of one per window (the clips of a
        batch differ in their prompts).  Each window's
        bookkeeping is one _BeamWindow (cbw_beam_select, replayed on the host every ``check_every`` steps), as in
        beam_search_dev, and each row's logits equal a step over its window alone, so every window gets the tokens
        beam_search_dev gives it.
        Returns the sequences (with ``return_score``: (sequence, score) pairs) in window order."""
        n = len(windows)
        max_lengths = [int(m) for m in _per_window(max_length, n, "max_length")]
        begins = _per_window(begin_index, n, "begin_index")
        prompt_lens = _per_window(decoder_prompt_len, n, "decoder_prompt_len")
        bias_ats = _per_window(bias_at, n, "bias_at")
        if any(m > self.max_len for m in max_lengths):
            raise ValueError(f"max_length {max(max_lengths)} exceeds the decoder's {self.max_len} positions")
        k = min(16, 2 * num_beams)
        cap = row_cap(max_rows, num_beams)
        slots = max(1, min(len(windows), cap // num_beams))
        if num_beams > 16 or any(len(p) < 2 for _, p in windows):
            raise ValueError("beam_search_windows needs num_beams <= 16 and prefixes of >= 2 tokens")
        stream = _lib.stream_handle()
        results: List = [None] * len(windows)
        with torch.cuda.device(self.device):
            self.start_windows(slots, num_beams, cap)
            rows = slots * num_beams
            inc = torch.zeros((rows,), dtype=torch.int32, device=self.device)
            tok = torch.zeros((rows,), dtype=torch.int32, device=self.device)
            ident = torch.arange(rows, dtype=torch.int32, device=self.device)
            src_rows = ident.clone()
            active: List[Optional[_BeamWindow]] = [None] * slots
            pending = list(range(len(windows)))

            def retire(w):
                inc[w.r0:w.r0 + num_beams].fill_(0)
                src_rows[w.r0:w.r0 + num_beams].copy_(ident[w.r0:w.r0 + num_beams])
                active[w.slot] = None
                results[w.index] = w.result(return_score)

            it = 0
            while pending or any(a is not None for a in active):
                for slot in range(slots):
                    if active[slot] is None and pending:
                        i = pending.pop(0)
                        enc_out, prefix = windows[i]
                        self.set_window(slot, enc_out)
                        self.prefill_window(slot, num_beams, prefix)
                        active[slot] = _BeamWindow(self, i, slot, prefix, num_beams, k, eos, max_lengths[i], rules,
                                                   begins[i], prompt_lens[i], length_penalty)
                        inc[slot * num_beams:(slot + 1) * num_beams].fill_(1)
                live = [w for w in active if w is not None]
                for w in live:
                    w.score(bias_ats[w.index], stream)
                    if not w.stopped:   # the step's tokens and (global) parent rows for this window's rows
                        tok[w.r0:w.r0 + num_beams].copy_(w.next_tokens())
                        torch.add(w.next_rows(), w.r0, out=src_rows[w.r0:w.r0 + num_beams])
                for w in live:   # windows at max_length: replayed now, no further steps
                    if w.stopped:
                        w.replay()
                        retire(w)
                live = [w for w in active if w is not None]
                if not live:
                    continue
                length = max(w.pos for w in live)
                _lib.check(self.lib.cbw_decoder_reorder(self.h, src_rows.data_ptr(), rows, slots, length,
                                                        self._state.data_ptr(), self._state.numel(), stream),
                           "cbw_decoder_reorder")
                self.step_rows(tok)
                self._posr.add_(inc)
                for w in live:
                    w.pos += 1
                it += 1
                if it % check_every == 0:   # one device -> host copy per window, then the finished ones leave
                    for w in live:
                        w.replay()
                        if w.bp.finished:
                            retire(w)
        return results

    def greedy_windows(self, windows: Sequence[Tuple[torch.Tensor, Sequence[int]]], eos: int, max_lengths,
                       bias: Optional[torch.Tensor], bias_begin: Optional[torch.Tensor], rules=None,
                       check_every: int = 8, return_logprobs: bool = False, max_slots: Optional[int] = None,
                       max_rows: int = 16, repetition_penalty: Optional[float] = None,
                       no_repeat_ngram_size: int = 0) -> List:
        """Greedy search (HF 4.37.2 greedy branch of GenerationMixin.generate, the call of pba_whisper.py:318-331 and
        :425-442 with num_beams = 1, do_sample = False) for several windows in lock step with no host round trip per
        token: windows = [(enc_out f32 [1500, D] post-LN, decoder prefix)], max_lengths one per window (or one int),
        decoded on one decoder state of min(len(windows), 16, ``max_slots``) slots of one row each (``max_rows`` = 80
        under CBW_DEC_WIDE: 80 in place of the 16), built as
        beam_search_windows builds its slots.  Per step one cbw_greedy_select per 16 rows (scores = logits + ``bias_begin`` at a window's
        first free position, ``bias`` after it, + the timestamp rules of ``rules`` from a device-side state; argmax;
        log-prob of the processed scores) writes the step's row of a device log, cbw_decoder_step_rows reads its tokens
        from there, and the rows still active move one position.  Every ``check_every`` steps the new log rows come
        back in one copy and cbw.generate.greedy_replay reads them: finished windows leave, pending ones take their
        slots; steps enqueued past a row's end are ignored (cbw_greedy_select's invariant keeps them inside the
        cache).  Begin suppression and the rules' begin index are len(prefix); no forced positions.
        ``repetition_penalty`` / ``no_repeat_ngram_size``: the caller's two history processors in front of the choice
        (cbw_history_rules, see _lock_step); unset, nothing is allocated or launched for them.
        Returns the sequences (prefix included) in window order; with ``return_logprobs`` (sequence, per-step
        log-probs) pairs."""
        def select(args, live, r0, stream):
            _lib.check(self.lib.cbw_greedy_select(*args, stream), "cbw_greedy_select")
        return self._lock_step("greedy_windows", windows, eos, max_lengths, bias, bias_begin, rules, select,
                               check_every, return_logprobs, max_slots, max_rows=max_rows,
                               repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)

    def _lock_step(self, name: str, windows, eos: int, max_lengths, bias, bias_begin, rules, select: callable,
                   check_every: int, return_logprobs: bool, max_slots: Optional[int], replayed: Optional[callable] = None,
                   max_rows: int = 16, repetition_penalty: Optional[float] = None,
                   no_repeat_ngram_size: int = 0) -> List:
        """The lock-step driver greedy_windows and sample_windows share: slot admission, the device log of
        ``check_every`` steps, the one copy per replay, cbw.generate.greedy_replay and the divergence check.  Per step
        and slice of 16 rows starting at ``r0`` (those kernels take at most 16; every argument is row-indexed)
        ``select(args, live, r0, stream)`` makes the rows' choice: ``args`` are the arguments cbw_greedy_select and
        cbw_sample_select have in common (logits ... logprob, writing the step's row of the log), ``live[slot]`` the
        window in each slot (None: empty).  ``replayed(window, taken, finished)`` is called after every replay with the
        number of logged steps the window took from it.
        With ``repetition_penalty`` (not None and != 1) or ``no_repeat_ngram_size`` > 0, HF 4.37.2's
        RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor run on the slice's logits in front of
        ``select`` (cbw_history_rules, one launch per step and slice) from a token history per slot on the device:
        ``hist`` int32 [slots, max_len + 1] and ``hist_len`` [slots], the prefix written on admission, every later token
        appended by the kernel itself from the previous step's token row of the log (the previous replay batch's last
        row for a batch's first step; none at the very first step).  The kernel appends only where hist_len == the
        position of the row's last token, so a reused slot, whose fresh history is one longer than that, takes
        nothing from the token row its previous window left.  Neither control set: nothing is allocated or launched
        for them."""
        from .generate import greedy_replay
        penalty = 1.0 if repetition_penalty is None else float(repetition_penalty)
        ngram = int(no_repeat_ngram_size or 0)
        if not (penalty > 0 and math.isfinite(penalty)) or ngram < 0:
            raise ValueError(f"{name} needs a finite repetition_penalty > 0 and no_repeat_ngram_size >= 0")
        history = penalty != 1.0 or ngram > 0
        n = len(windows)
        limits = [int(max_lengths)] * n if isinstance(max_lengths, int) else [int(m) for m in max_lengths]
        if len(limits) != n:
            raise ValueError(f"{name} needs one max_length per window")
        if any(m > self.max_len for m in limits):
            raise ValueError(f"max_length {max(limits)} exceeds the decoder's {self.max_len} positions")
        if any(len(p) < 2 for _, p in windows):
            raise ValueError(f"{name} needs prefixes of >= 2 tokens")
        check_every = max(1, int(check_every))
        results: List = [None] * n
        pending = []
        for i, (_, p) in enumerate(windows):   # nothing to decode: `greedy` returns the prefix
            if len(p) >= limits[i]:
                results[i] = (list(p), []) if return_logprobs else list(p)
            else:
                pending.append(i)
        if not pending:
            return results
        dev, stream = self.device, _lib.stream_handle()
        tb, no_ts, max_initial = (rules.timestamp_begin, rules.no_timestamps, rules.max_initial) if rules is not None \
            else (-1, -1, -1)
        with torch.cuda.device(dev):
            cap = row_cap(max_rows)
            slots = max(1, min(len(pending), cap, cap if max_slots is None else int(max_slots)))
            self.start_windows(slots, 1, cap)
            ts_state = torch.zeros((slots, 4), dtype=torch.int32, device=dev)
            limit = torch.zeros((slots,), dtype=torch.int32, device=dev)
            active = torch.zeros((slots,), dtype=torch.int32, device=dev)
            # the log: per step one row of {tokens, log-probs (f32 bits), active} x slots, so a replay is one copy
            log = torch.zeros((check_every, 3, slots), dtype=torch.int32, device=dev)
            log_lp = log.view(torch.float32)
            if history:
                hist = torch.zeros((slots, self.max_len + 1), dtype=torch.int32, device=dev)
                hist_len = torch.zeros((slots,), dtype=torch.int32, device=dev)
                last_pos = torch.zeros((slots,), dtype=torch.int32, device=dev)   # self._posr - 1: the last tokens'
                last_tok = 0   # the previous step's token row of the log (0: none yet)
            live: List[Optional[int]] = [None] * slots   # the window in each slot
            seqs: List[Optional[List[int]]] = [None] * slots
            lps: List[List[float]] = [[] for _ in range(slots)]
            while pending or any(w is not None for w in live):
                for slot in range(slots):
                    if live[slot] is None and pending:
                        i = pending.pop(0)
                        enc_out, prefix = windows[i]
                        self.set_window(slot, enc_out)
                        self.prefill_window(slot, 1, prefix)
                        ts_state[slot] = torch.tensor([0, -1, -1, -1], dtype=torch.int32)
                        limit[slot:slot + 1].fill_(limits[i])
                        active[slot:slot + 1].fill_(1)
                        if history:
                            hist[slot, :len(prefix)] = torch.tensor(list(prefix), dtype=torch.int32)
                            hist_len[slot:slot + 1].fill_(len(prefix))
                        live[slot], seqs[slot], lps[slot] = i, list(prefix), []
                # no row needs more steps than the longest remainder; the step after the last of those is not run
                left = max(limits[w] - len(seqs[s]) for s, w in enumerate(live) if w is not None)
                steps = min(check_every, left)
                lg, tsp, posp, limp, actp = (t.data_ptr() for t in (self._logits, ts_state, self._posr, limit, active))
                for c in range(steps):
                    tokp, lpp = log[c, 0].data_ptr(), log_lp[c, 1].data_ptr()
                    if history:
                        torch.sub(self._posr, 1, out=last_pos)
                    for r0 in range(0, slots, 16):
                        o = 4 * r0   # int32 / f32 rows
                        if history:
                            _lib.check(self.lib.cbw_history_rules(
                                lg + o * self.vpad, min(16, slots - r0), self.vocab, self.vpad,
                                hist.data_ptr() + o * hist.shape[1], hist.shape[1], hist_len.data_ptr() + o,
                                last_tok + o if last_tok else None, last_pos.data_ptr() + o, actp + o, penalty, ngram,
                                stream), "cbw_history_rules")
                        select((lg + o * self.vpad, min(16, slots - r0), self.vocab, self.vpad, _lib.ptr(bias),
                                _lib.ptr(bias_begin), tb, no_ts, eos, max_initial, tsp + 4 * o, posp + o, limp + o,
                                actp + o, tokp + o, lpp + o), live, r0, stream)
                    log[c, 2].copy_(active)
                    last_tok = tokp
                    if c + 1 == left:
                        break
                    self.step_rows(log[c, 0])
                    self._posr.add_(active)
                host = log[:steps].cpu()   # the one device -> host copy (and sync) per check_every steps
                toks, lpv, act = host[:, 0].numpy(), host[:, 1].view(torch.float32).numpy(), host[:, 2].numpy()
                limits_s = [limits[w] if w is not None else 0 for w in live]
                for slot, rep in enumerate(greedy_replay(toks, lpv, seqs, limits_s, eos)):
                    if rep is None:
                        continue
                    seq, new_lps, finished = rep
                    if bool(act[steps - 1, slot]) == finished:
                        raise RuntimeError("GPU greedy bookkeeping diverged from the host replay")
                    seqs[slot] = seq
                    lps[slot] += new_lps
                    if replayed is not None:
                        replayed(live[slot], len(new_lps), finished)
                    if finished:
                        results[live[slot]] = (seq, lps[slot]) if return_logprobs else seq
                        live[slot], seqs[slot], lps[slot] = None, None, []
        return results

    def greedy_dev(self, enc_out: torch.Tensor, prefix: Sequence[int], eos: int, max_length: int,
                   bias: Optional[torch.Tensor], bias_begin: Optional[torch.Tensor], rules=None, check_every: int = 8,
                   return_logprobs: bool = False, repetition_penalty: Optional[float] = None,
                   no_repeat_ngram_size: int = 0):
        """greedy_windows over one window: enc_out f32 [1500, D] (or [1, 1500, D]) -> the sequence, or with
        ``return_logprobs`` (sequence, per-step log-probs)."""
        return self.greedy_windows([(enc_out, prefix)], eos, [max_length], bias, bias_begin, rules, check_every,
                                   return_logprobs, repetition_penalty=repetition_penalty,
                                   no_repeat_ngram_size=no_repeat_ngram_size)[0]

    def sample_windows(self, windows: Sequence[Tuple[torch.Tensor, Sequence[int]]], eos: int, max_lengths,
                       bias: Optional[torch.Tensor], bias_begin: Optional[torch.Tensor], rules, temperature: float,
                       generators, top_k: int = 50, check_every: int = 8, max_slots: Optional[int] = None,
                       max_rows: int = 16, repetition_penalty: Optional[float] = None,
                       no_repeat_ngram_size: int = 0) -> List:
        """Temperature sampling (HF 4.37.2 sample branch of GenerationMixin.generate: the call of
        pba_whisper.py:318-331 with do_sample = True, and every temperature > 0 rung of generate_with_fallback,
        :425-442) for several windows in lock step with no host round trip per token: greedy_windows' driver with
        cbw_sample_select as the step's choice (the processed scores of cbw_greedy_select, top-``top_k`` and
        ``temperature`` warpers, the draw, the log-prob of the top-k-filtered scores).  The draw is torch.multinomial's
        exponential race with its noise made here: per step and live window one ``exponential_`` of [V] numbers from
        that window's own generator into the window's row of a noise buffer (an asynchronous torch op), so a
        window's tokens depend neither on its slot nor on the other windows, and are the tokens sample_search draws
        with an identically seeded generator (except where an fp32 tie in the race resolves differently).
        ``generators``: one device torch.Generator per window (a single one for a single window), each used by no
        other window.  Steps enqueued past a window's end consume draws; after the replay that ends a window its
        generator is set back to the state right after the draw of its last token, where sample_search leaves it.
        ``repetition_penalty`` / ``no_repeat_ngram_size``: as greedy_windows (the processors act on the raw logits,
        before the warpers).
        Returns (sequence incl. the prefix, per-step log-probs) per window, as sample_search."""
        if not (temperature > 0 and math.isfinite(temperature)) or top_k < 1:
            raise ValueError("sample_windows needs a finite temperature > 0 and top_k >= 1")
        gens = [generators] if isinstance(generators, torch.Generator) else list(generators)
        if len(gens) != len(windows) or len({id(g) for g in gens}) != len(gens):
            raise ValueError("sample_windows needs one generator of its own per window")
        V = self.vocab
        noise: List[Optional[torch.Tensor]] = [None]
        states: List[list] = [[] for _ in gens]   # per window: the generator's state after each draw since the last replay

        def select(args, live, r0, stream):
            if noise[0] is None:
                noise[0] = torch.ones((len(live), V), dtype=torch.float32, device=self.device)
            for slot in range(r0, min(r0 + 16, len(live))):   # the draws of this slice's windows, in slot order
                w = live[slot]
                if w is not None:
                    noise[0][slot].exponential_(generator=gens[w])
                    states[w].append(gens[w].get_state())
            _lib.check(self.lib.cbw_sample_select(*args, float(temperature), int(top_k),
                                                  noise[0].data_ptr() + 4 * r0 * V, V, stream), "cbw_sample_select")

        def replayed(w, taken, finished):
            if finished:
                gens[w].set_state(states[w][taken - 1])
            states[w].clear()
        return self._lock_step("sample_windows", windows, eos, max_lengths, bias, bias_begin, rules, select,
                               check_every, True, max_slots, replayed, max_rows=max_rows,
                               repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)

    def sample_dev(self, enc_out: torch.Tensor, prefix: Sequence[int], eos: int, max_length: int,
                   bias: Optional[torch.Tensor], bias_begin: Optional[torch.Tensor], rules, temperature: float,
                   generator: torch.Generator, top_k: int = 50, check_every: int = 8,
                   repetition_penalty: Optional[float] = None, no_repeat_ngram_size: int = 0):
        """sample_windows over one window -> (sequence, per-step log-probs)."""
        return self.sample_windows([(enc_out, prefix)], eos, [max_length], bias, bias_begin, rules, temperature,
                                   [generator], top_k, check_every, repetition_penalty=repetition_penalty,
                                   no_repeat_ngram_size=no_repeat_ngram_size)[0]

    def sample_search(self, prefix: Sequence[int], eos: int, max_length: int, bias_at: callable, rules=None,
                      begin_index: int = 0, temperature: float = 0.0, top_k: int = 50,
                      generator: Optional[torch.Generator] = None, forced: Optional[dict] = None,
                      free_pos: Optional[int] = None) -> Tuple[list, list]:
        """One row, token by token, with the per-step log-probs transformers' fallback checks read
        (cbw.fallback.avg_logprob): the processed scores (logits + suppression bias + timestamp rules, the
        processors of HF's greedy / sample loops) -> temperature 0: argmax (ties -> lower id, as
        cbw_logprob_topk), log-prob = log_softmax(scores)[token]; temperature T > 0: HF's sampling warpers
        (scores / T, all but the top_k set to -inf; GenerationConfig's default top_k 50), a token drawn from
        their softmax with ``generator`` (a seeded device RNG), log-prob = log_softmax(warped * T)[token].  The
        decoder step, timestamp rules and masks run in libcbw; the draw is a torch op on the device.
        ``forced`` (position -> token) / ``free_pos``: the free language position of short-form ``language=None``
        and the forced positions after it (``free_position_state``).
        Returns (full sequence incl. the prefix, per-generated-step log-probs)."""
        forced = forced or {}
        rows, Benc = self._shape
        if rows != 1 or Benc != 1:
            raise ValueError("sample_search decodes one row")
        seq = list(prefix)
        lps = []
        if len(prefix) > 1:
            self.prefill(prefix)
        else:
            self.step(list(prefix), 0)
        pos = len(prefix)
        V = self.vocab
        while len(seq) < max_length:
            if pos in forced:   # ForceTokensLogitsProcessor: the forced token at log-prob 0
                tok = int(forced[pos])
                lps.append(0.0)
                seq.append(tok)
                self.step([tok], pos)
                pos += 1
                continue
            b = bias_at(pos)
            logits = self._logits[:, :V]
            if rules is not None and pos == free_pos:
                scores = logits + self.timestamp_bias(rules, None, b, [free_position_state(rules)])
            elif rules is not None and pos >= begin_index:
                scores = logits + self.timestamp_bias(rules, [seq[begin_index:]], b)
            else:
                scores = logits + b if b is not None else logits.clone()
            if temperature and temperature > 0:
                kth = torch.topk(scores, min(top_k, V), dim=-1).values[:, -1:]
                w = torch.where(scores >= kth, scores / temperature, torch.full_like(scores, float("-inf")))
                tok = int(torch.multinomial(torch.softmax(w, -1), 1, generator=generator)[0, 0])
                lp = torch.log_softmax(w * temperature, -1)[0, tok]
            else:
                tok = int(torch.argmax(scores[0]))
                lp = torch.log_softmax(scores, -1)[0, tok]
            lps.append(float(lp))
            seq.append(tok)
            if tok == eos or len(seq) >= max_length:
                break
            self.step([tok], pos)
            pos += 1
        return seq, lps

    def logits_row(self, row: int) -> torch.Tensor:
        """The last step's fp32 logits of one row over the vocabulary (a device view)."""
        return self._logits[row, :self.vocab]

    def no_speech_prob(self, prefix: Sequence[int], sot_index: int, no_speech_token: int) -> float:
        """WhisperNoSpeechDetection: softmax(logits at the <|startoftranscript|> position)[no_speech_token] for the
        window whose decoder input is ``prefix`` (one row; the caller restarts the window before decoding)."""
        if sot_index > 0:
            self.prefill(list(prefix[:sot_index + 1]))
        else:
            self.step([prefix[0]], 0)
        return float(torch.softmax(self._logits[0, :self.vocab].double(), -1)[no_speech_token])

    def _stepper(self, scores: callable):
        """The step function scores_fn, processed_step_fn and step_fn share: fn(tokens, pos, reorder_rows) reorders the
        KV cache, tracks every row's sequence so far, runs one step and returns ``scores(pos + 1, seqs)``; fn.prefill
        (Benc = 1) runs the forced prefix in one pass and returns the scores for position len(prefix)."""
        seqs = []

        def fn(tokens, pos, reorder_rows):
            nonlocal seqs
            if pos == 0:
                seqs = [[] for _ in tokens]
            if reorder_rows is not None:
                self.reorder(reorder_rows, pos)
                seqs = [list(seqs[r]) for r in reorder_rows]
            for r, t in enumerate(tokens):
                seqs[r].append(int(t))
            self.step(tokens, pos)
            return scores(pos + 1, seqs)

        def prefill(prefix):
            nonlocal seqs
            if self._shape[1] != 1:
                return None
            seqs = [list(prefix) for _ in range(self._shape[0])]
            self.prefill(prefix)
            return scores(len(prefix), seqs)
        fn.prefill = prefill
        return fn

    def scores_fn(self, bias_at: callable, rules=None, begin_index: int = 0):
        """A cbw.generate.beam_sample scores function: reorder the KV cache, run one step, return every row's
        processed log-probs for the next position as a device tensor [rows, V]: log_softmax(logits) + the
        suppression bias (bias_at(pos)) and, with ``rules``, the per-row timestamp rules over each row's tokens since
        ``begin_index`` (the masks step_fn's top-k sees)."""

        def scores(pos, seqs):
            b = bias_at(pos)
            lp = torch.log_softmax(self._logits[:, :self.vocab].float(), dim=-1)
            if rules is not None and pos >= begin_index:
                return lp + self.timestamp_bias(rules, [s[begin_index:] for s in seqs], b)
            return lp + b if b is not None else lp

        return self._stepper(scores)

    def processed_step_fn(self, k: int, bias_at: callable, repetition_penalty: Optional[float] = None,
                          no_repeat_ngram_size: int = 0, greedy: bool = False):
        """A cbw.generate StepFn with a caller's repetition_penalty / no_repeat_ngram_size (4.37.2's processor order:
        RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, then the suppression processors) on the
        step's scores -- log_softmax(logits) for beam search, the raw logits for greedy, as HF applies its processors
        to each.  Each row's token history is the row's sequence so far (decoder prompt included).  The penalty is
        multiplicative, so the scores are formed with torch ops on the device logits and the top-k by a stable sort
        (ties -> lower id, as cbw_logprob_topk); no timestamp rules (the caller raises for that combination)."""
        V = self.vocab

        def scores(pos, seqs):
            x = self._logits[:, :V].float()
            x = x.clone() if greedy else torch.log_softmax(x, dim=-1)
            for r, sq in enumerate(seqs):
                if repetition_penalty is not None and repetition_penalty != 1.0 and sq:
                    ids = torch.tensor(sorted(set(sq)), dtype=torch.long, device=x.device)
                    g = x[r, ids]
                    x[r, ids] = torch.where(g < 0, g * repetition_penalty, g / repetition_penalty)
                ban = banned_ngram_tokens(sq, no_repeat_ngram_size)
                if ban:
                    x[r, torch.tensor(ban, dtype=torch.long, device=x.device)] = float("-inf")
            b = bias_at(pos)
            if b is not None:
                x = x + b
            v, i = torch.sort(x, dim=-1, descending=True, stable=True)
            return v[:, :k].cpu().numpy(), i[:, :k].to(torch.int32).cpu().numpy()

        return self._stepper(scores)

    def step_fn(self, k: int, bias_at: callable, rules=None, begin_index: int = 0, free_pos: Optional[int] = None):
        """A cbw.generate StepFn: reorder the KV cache, run one step, return the top-k of
        log_softmax(logits) + the processors' masks for the next position: the suppression bias
        (bias_at(pos) -> tensor or None) and, with ``rules`` (cbw.timestamps.TimestampRules), the
        per-row timestamp rules over each row's tokens since ``begin_index``; at ``free_pos`` (the free language
        position of short-form ``language=None``, before ``begin_index``) the rules in ``free_position_state``."""

        def scores(pos, seqs):
            b = bias_at(pos)
            if rules is not None and pos == free_pos:
                return self.topk(k, self.timestamp_bias(rules, None, b, [free_position_state(rules)] * len(seqs)),
                                 self.vocab)
            if rules is None or pos < begin_index:
                return self.topk(k, b)
            return self.topk(k, self.timestamp_bias(rules, [s[begin_index:] for s in seqs], b), self.vocab)

        return self._stepper(scores)


def banned_ngram_tokens(seq: Sequence[int], n: int) -> List[int]:
    """NoRepeatNGramLogitsProcessor (transformers 4.37.2 _get_ngrams / _calc_banned_ngram_tokens) for one row: the
    tokens that would complete an n-gram already in ``seq`` (the row's tokens so far, decoder prompt included)."""
    if n <= 0 or len(seq) + 1 < n:
        return []
    prev = tuple(seq[len(seq) - n + 1:]) if n > 1 else ()
    out = []
    for i in range(len(seq) - n + 1):
        if tuple(seq[i:i + n - 1]) == prev:
            out.append(int(seq[i + n - 1]))
    return out


def free_position_state(rules) -> Tuple[int, int, int, int]:
    """WhisperTimeStampLogitsProcessor (4.37.2) at a position before its begin_index -- the free language position
    of short-form ``language=None``: input_ids[k, begin_index:] is empty (no pair rule, no floor) and
    input_ids.shape[1] != begin_index (no initial-timestamp rule); <|notimestamps|> is still suppressed and the
    timestamp-mass rule still applies.  As a cbw_timestamp_rules state (TimestampRules.state's fields)."""
    return (0, 1, int(rules.timestamp_begin), 0)


class _BeamWindow:
    """One window's beam search with the bookkeeping on the GPU, the only statement of it: DecoderEngine.beam_search_dev
    runs one (slot 0 of a start() state, stepped by cbw_decoder_step), beam_search_windows one per slot of its lock-step
    state (cbw_decoder_step_rows).  Holds the window's HF 4.37.2 BeamProcess, the device log cbw_beam_select writes (one
    row per step: candidate scores / rows / tokens, next tokens, next parent rows, ok flag) and the timestamp-rule
    state of its rows.  ``score`` enqueues one step's choice, ``replay`` reads the new log rows back in one copy and
    runs them through the BeamProcess, ``result`` is the search's outcome; the caller steps the decoder and advances
    ``pos``."""

    def __init__(self, eng: "DecoderEngine", index, slot, prefix, beams, k, eos, max_length, rules, begin_index,
                 decoder_prompt_len, length_penalty):
        from .generate import BeamProcess
        dev = eng.device
        self.eng, self.index, self.slot, self.r0, self.beams, self.k = eng, index, slot, slot * beams, beams, k
        self.eos, self.max_length, self.rules, self.begin = eos, max_length, rules, begin_index
        self.bp = BeamProcess(prefix, beams, eos, max_length, length_penalty, decoder_prompt_len)
        n_max = max(1, max_length - len(prefix))
        self.lp = torch.empty((beams, k), dtype=torch.float32, device=dev)
        self.idx = torch.empty((beams, k), dtype=torch.int32, device=dev)
        self.scores = torch.tensor([0.0] + [-1e9] * (beams - 1), dtype=torch.float64, device=dev)
        # one log row per step, every field a column range of one byte buffer, so a replay is ONE device -> host
        # copy (six separate .cpu() calls cost ~33 copy launches per replay)
        self.f = (0, 8 * k, 12 * k, 16 * k, 16 * k + 4 * beams, 16 * k + 8 * beams)
        row_bytes = (self.f[5] + 4 + 7) // 8 * 8
        self.log = torch.zeros((n_max, row_bytes), dtype=torch.uint8, device=dev)
        self.c_score, self.c_row, self.c_tok, self.nxt_tok, self.nxt_row, self.ok = self.fields(self.log)
        self.tb = rules.timestamp_begin if rules is not None else 1 << 30
        sampled = list(prefix[begin_index:]) if begin_index < len(prefix) else []
        tsl = [t for t in sampled if t >= self.tb]
        ts0 = [len(sampled), sampled[-1] if sampled else -1, sampled[-2] if len(sampled) > 1 else -1,
               tsl[-1] if tsl else -1]
        self.ts_state = torch.tensor([ts0] * beams, dtype=torch.int32, device=dev)
        self.st = torch.tensor([list(rules.state(sampled)) if rules is not None else [0, 1, 0, 1]] * beams,
                               dtype=torch.int32, device=dev)
        self.tsb = torch.empty((beams, eng.vocab), dtype=torch.float32, device=dev) if rules is not None else None
        self.pos = len(prefix)
        self.s = 0           # log rows written
        self.replayed = 0    # log rows the host has replayed
        self.stopped = False   # reached max_length: no further steps

    def fields(self, buf):
        """(candidate scores, rows, tokens, next tokens, next parent rows, ok) column views of log rows"""
        f = self.f
        return (buf[:, f[0]:f[1]].view(torch.float64), buf[:, f[1]:f[2]].view(torch.int32),
                buf[:, f[2]:f[3]].view(torch.int32), buf[:, f[3]:f[4]].view(torch.int32),
                buf[:, f[4]:f[5]].view(torch.int32), buf[:, f[5]:f[5] + 4].view(torch.int32)[:, 0])

    def next_tokens(self) -> torch.Tensor:
        """The step just scored: its rows' next tokens (device int32 [beams], a view of the log row)."""
        return self.nxt_tok[self.s - 1]

    def next_rows(self) -> torch.Tensor:
        """The step just scored: its rows' parent rows within the window (device int32 [beams], as next_tokens)."""
        return self.nxt_row[self.s - 1]

    def score(self, bias_at, stream):
        """This window's logits (its rows of the engine's step logits) -> scores -> next beams, into log row self.s:
        the next tokens / parent rows go straight there, where the reorder and the decode step can read them."""
        eng, nb, s = self.eng, self.beams, self.s
        b = bias_at(self.pos)
        lg = eng._logits[self.r0].data_ptr()
        ts_on = self.rules is not None and self.pos >= self.begin
        if ts_on:
            eng._timestamp_rules(lg, nb, b, self.st, self.rules, self.tsb, stream)
            bias, bias_ld = self.tsb, eng.vocab
        else:
            bias, bias_ld = b, 0
        eng._logprob_topk(lg, nb, bias, bias_ld, self.k, self.lp, self.idx, stream)
        _lib.check(eng.lib.cbw_beam_select(self.lp.data_ptr(), self.idx.data_ptr(), nb, self.k, self.eos,
                                           self.scores.data_ptr(), self.c_score[s].data_ptr(),
                                           self.c_row[s].data_ptr(), self.c_tok[s].data_ptr(),
                                           self.nxt_tok[s].data_ptr(), self.nxt_row[s].data_ptr(),
                                           self.ok[s].data_ptr(), self.ts_state.data_ptr(), self.st.data_ptr(),
                                           self.tb, int(ts_on), stream),
                   "cbw_beam_select")
        self.s += 1
        if self.pos + 1 >= self.max_length:
            self.stopped = True

    def replay(self):
        """The log rows written since the last replay, in one device -> host copy, through the BeamProcess."""
        if self.s <= self.replayed:
            return
        cs, cr, ct, nt, nr, okh = (t.numpy() for t in self.fields(self.log[self.replayed:self.s].cpu()))
        for i in range(self.s - self.replayed):
            toks, par = self.bp.process([(float(cs[i, j]), int(cr[i, j]), int(ct[i, j])) for j in range(self.k)])
            if not self.bp.finished and (not okh[i] or toks != nt[i].tolist() or par != nr[i].tolist()):
                raise RuntimeError("GPU beam bookkeeping diverged from the host replay")
            if self.bp.finished:
                break
        self.replayed = self.s

    def result(self, return_score: bool = False):
        """The finished search's sequence (prefix included), with ``return_score`` (sequence, its score)."""
        if not self.bp.finished:
            raise RuntimeError("GPU beam search ended before the host replay finished")
        seq = self.bp.result()
        return (seq, self.bp.score) if return_score else seq
