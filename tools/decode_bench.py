"""Whisper decoder step timing (large-v3 by default) at 5 beams: cross-KV precompute per 30 s window and
one decode step per token (KV cache append, self + cross attention, MLP, vocabulary projection), against
the step's HBM roofline (every decoder weight + the KV caches read once per step).
usage: python tools/decode_bench.py [model] [beams] [steps]; DB_POS0=P: the timed steps start at position P (the
keyword-prompted windows of C5 / e2e decode from ~150-230 prefix tokens: self-attention over several key chunks);
DB_HISTORY=P,N (e.g. 1.3,3): also the lock-step greedy step of DB_ROWS rows (default 1; cbw_greedy_select +
cbw_decoder_step_rows, as DecoderEngine.greedy_windows enqueues it) without and with the cbw_history_rules pre-pass at
repetition_penalty P and no_repeat_ngram_size N, every row's history pos0 tokens long at the first timed step"""
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
from cbw import synth  # noqa: E402
from cbw.decoder import DecoderEngine  # noqa: E402

model = sys.argv[1] if len(sys.argv) > 1 else "large-v3"
beams = int(sys.argv[2]) if len(sys.argv) > 2 else 5
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 64
dev = torch.device("cuda:0")
cfg = synth.WHISPER_DECODERS[model]
V, D, L, H, F = cfg
sd = synth.synth_whisper_decoder_state_dict(model, seed=0)
dec = DecoderEngine(cfg, sd, dev)
enc = torch.randn((1, 1500, D), device=dev)
for _ in range(2):
    dec.start(enc, beams)
torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(5):
    dec.start(enc, beams)
torch.cuda.synchronize()
t_cross = (time.perf_counter() - t) / 5
tok = [50258] * beams
pos0 = int(os.environ.get("DB_POS0", "4"))
dec.start(enc, beams)
for p in range(pos0):
    dec.step(tok, p)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for p in range(pos0, pos0 + steps):
    dec.step(tok, p)
e1.record()
torch.cuda.synchronize()
t_step = e0.elapsed_time(e1) / steps * 1e-3
# bytes per step: bf16 weights of every decoder linear (self qkv/out, cross q/out, fc1, fc2) + the
# vocabulary projection (tied embedding V x D) + self KV caches (mean length, per beam) + the window's
# cross KV (1500 rows, shared by the beams)
w_bytes = 2 * (L * (4 * D * D + 2 * D * D + 2 * D * F) + V * D)
kv_bytes = 2 * L * 2 * D * (beams * (pos0 + steps / 2) + 1500)
bytes_step = w_bytes + kv_bytes
print(f"decoder {model} beams={beams} pos0={pos0} self_split={os.environ.get('CBW_DEC_SELF_SPLIT', '0')}: cross-KV {t_cross * 1e3:.2f} ms/window, step {t_step * 1e3:.3f} ms "
      f"({1 / t_step:.0f} steps/s, {beams / t_step:.0f} beam-tokens/s); {bytes_step / 1e9:.2f} GB/step -> "
      f"{bytes_step / t_step / 1e12:.2f} TB/s = {bytes_step / t_step / 8e12:.1%} of 8 TB/s")

if os.environ.get("DB_HISTORY"):
    from cbw import _lib  # noqa: E402
    pen, ngram = os.environ["DB_HISTORY"].split(",")
    pen, ngram = float(pen), int(ngram)
    rows = int(os.environ.get("DB_ROWS", "1"))
    lib, st = dec.lib, _lib.stream_handle()
    prefix = [50258 + (i % 7) for i in range(max(2, pos0))]

    def lock_step(history: bool) -> float:
        """ms per step of select + decode step over ``rows`` one-row windows, the launches of _lock_step"""
        dec.start_windows(rows, 1)
        for s_ in range(rows):
            dec.set_window(s_, enc[0])
            dec.prefill_window(s_, 1, prefix)
        ts_state = torch.tensor([[0, -1, -1, -1]] * rows, dtype=torch.int32, device=dev)
        limit = torch.full((rows,), dec.max_len, dtype=torch.int32, device=dev)
        active = torch.ones((rows,), dtype=torch.int32, device=dev)
        log = torch.zeros((steps + 8, 2, rows), dtype=torch.int32, device=dev)
        hist = torch.zeros((rows, dec.max_len + 1), dtype=torch.int32, device=dev)
        hist[:, :len(prefix)] = torch.tensor(prefix, dtype=torch.int32)
        hist_len = torch.full((rows,), len(prefix), dtype=torch.int32, device=dev)
        last_pos = torch.zeros((rows,), dtype=torch.int32, device=dev)
        lg = dec._logits.data_ptr()
        no_eos = torch.zeros((V,), dtype=torch.float32, device=dev)   # EOS suppressed: the rows never end
        no_eos[50257] = float("-inf")

        def run(c0, c1):
            for c in range(c0, c1):
                if history:
                    torch.sub(dec._posr, 1, out=last_pos)
                    _lib.check(lib.cbw_history_rules(lg, rows, V, dec.vpad, hist.data_ptr(), hist.shape[1],
                                                     hist_len.data_ptr(), log[c - 1, 0].data_ptr() if c else None,
                                                     last_pos.data_ptr(), active.data_ptr(), pen, ngram, st),
                               "cbw_history_rules")
                _lib.check(lib.cbw_greedy_select(lg, rows, V, dec.vpad, no_eos.data_ptr(), no_eos.data_ptr(), -1, -1,
                                                 50257, -1, ts_state.data_ptr(),
                                                 dec._posr.data_ptr(), limit.data_ptr(), active.data_ptr(),
                                                 log[c, 0].data_ptr(), log[c, 1].data_ptr(), st), "cbw_greedy_select")
                dec.step_rows(log[c, 0])
                dec._posr.add_(active)
        run(0, 8)
        torch.cuda.synchronize()
        e0.record()
        run(8, 8 + steps)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    if rows > 16 or len(prefix) + steps + 8 >= dec.max_len:
        sys.exit("DB_HISTORY: DB_ROWS <= 16 and pos0 + steps + 8 < max_len")
    off = [lock_step(False) for _ in range(3)]
    on = [lock_step(True) for _ in range(3)]
    print(f"lock-step greedy step, {rows} rows, history from {len(prefix)} tokens: without the pre-pass "
          f"{min(off):.4f} ms (three runs {' '.join(f'{v:.4f}' for v in off)}), with cbw_history_rules(p={pen}, n={ngram}) "
          f"{min(on):.4f} ms ({' '.join(f'{v:.4f}' for v in on)}): +{(min(on) - min(off)) * 1e3:.1f} us")
