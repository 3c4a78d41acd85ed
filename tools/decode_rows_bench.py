"""Decode-step cost of several windows in one step (cbw_decoder_step_rows) vs one window's step, and the
WindowBatcher's whole iteration (per-window scoring + reorder + step) -- GPU time from events, host time from
the wall clock.  usage: python tools/decode_rows_bench.py [model] [steps] [windows,...]

python tools/decode_rows_bench.py [model] [steps] wide [rounds]: the step over more than 16 rows
(cbw_decoder_step_wide) beside the unchanged one -- 5 and 15 rows on cbw_decoder_step_rows, 20, 40 and 80 rows wide
with the column blocks and with the row groups as the fast grid coordinate (CBW_GEMV_WIDE_ORDER) -- every
configuration measured once per round, the rounds interleaved, median and range over the rounds printed last as one
JSON line."""
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
from cbw import synth  # noqa: E402
from cbw.decoder import DecoderEngine  # noqa: E402

model = sys.argv[1] if len(sys.argv) > 1 else "large-v3"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 48
wide_mode = len(sys.argv) > 3 and sys.argv[3] == "wide"
only = [] if wide_mode else [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 2, 3]
beams = 5
dev = torch.device("cuda:0")
cfg = synth.WHISPER_DECODERS[model]
V, D, L, H, F = cfg
sd = synth.synth_whisper_decoder_state_dict(model, seed=0)
dec = DecoderEngine(cfg, sd, dev)
enc = torch.randn((1500, D), device=dev)
prefix = [50258, 50259, 50360, 50364]


def timed(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, (time.perf_counter() - t) * 1e3 / n


# one window, the classic step
dec.start(enc[None], beams)
tok = [50258] * beams
pos = [4]


def one():
    dec.step(tok, pos[0])
    pos[0] += 1


def rows_step(wins, order=None):
    """ms per step (GPU events) of `wins` windows x 5 beams on one lock-step state, freshly prefilled"""
    if order is not None:
        os.environ["CBW_GEMV_WIDE_ORDER"] = order
    dec.start_windows(wins, beams, max_rows=80)
    for s in range(wins):
        dec.set_window(s, enc)
        dec.prefill_window(s, beams, prefix)
    rows = wins * beams
    toks = torch.full((rows,), 50258, dtype=torch.int32, device=dev)
    inc = torch.ones((rows,), dtype=torch.int32, device=dev)

    def many():
        dec.step_rows(toks)
        dec._posr.add_(inc)

    return timed(many, steps)[0]


if wide_mode:
    import json
    import statistics
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    configs = [(1, None), (3, None)] + [(w, o) for w in (4, 8, 16) for o in ("columns", "groups")]
    got = {c: [] for c in configs}
    for r in range(rounds):
        for c in configs:
            got[c].append(rows_step(*c))
            print(f"round {r}: {c[0] * beams} rows{' ' + c[1] if c[1] else ''}: {got[c][-1]:.3f} ms per step", flush=True)
    out = []
    for (w, o), v in got.items():
        med = statistics.median(v)
        out.append({"rows": w * beams, "order": o or "step_rows", "ms_per_step": round(med, 4), "min": round(min(v), 4),
                    "max": round(max(v), 4), "ms_per_row": round(med / (w * beams), 5), "rounds": rounds})
    print(json.dumps({"model": model, "steps": steps, "decode_rows_wide": out}))
    sys.exit(0)

if 0 in only or len(sys.argv) <= 3:
    g, w = timed(one, steps)
    print(f"step (1 window x {beams} beams): {g:.3f} ms GPU-event, {w:.3f} ms wall")
for wins in [x for x in only if x > 0]:
    dec.start_windows(wins, beams)
    for s in range(wins):
        dec.set_window(s, enc)
        dec.prefill_window(s, beams, prefix)
    rows = wins * beams
    toks = torch.full((rows,), 50258, dtype=torch.int32, device=dev)
    inc = torch.ones((rows,), dtype=torch.int32, device=dev)

    def many():
        dec.step_rows(toks)
        dec._posr.add_(inc)

    g, w = timed(many, steps)
    print(f"step_rows ({wins} windows x {beams} beams = {rows} rows): {g:.3f} ms GPU-event, {w:.3f} ms wall, "
          f"{g / wins:.3f} ms per window-step")
