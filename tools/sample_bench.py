"""Temperature sampling per token: the host loop (DecoderEngine.sample_search: per token a full-vocabulary top-k,
softmax, multinomial and log_softmax as torch ops and two device -> host syncs) vs the token choice on the GPU
(DecoderEngine.sample_dev, and sample_windows at 4 / 16 windows in lock step), with greedy_dev as the floor, on the
synthetic decoder with the timestamp rules on, a 200-token prefix and temperature 0.4.  Wall clock of the whole call
(cross-attention K/V, prefill, every step, the replays) over the tokens it generated; the paths alternate in one
process, three repeats each after a warm-up.  EOS is suppressed so every run generates ``steps`` tokens.
usage: python tools/sample_bench.py [model] [steps]"""
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
from cbw import synth  # noqa: E402
from cbw.decoder import DecoderEngine  # noqa: E402
from cbw.timestamps import TimestampRules  # noqa: E402

model = sys.argv[1] if len(sys.argv) > 1 else "large-v3"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 64
REPEATS, T = 3, 0.4
dev = torch.device("cuda:0")
cfg = synth.WHISPER_DECODERS[model]
V, D = cfg[0], cfg[1]
EOS, NO_TS = 50257, V - 1502
rules = TimestampRules(NO_TS + 1, NO_TS, EOS, 50)
dec = DecoderEngine(cfg, synth.synth_whisper_decoder_state_dict(model, seed=0), dev)
g = torch.Generator(device=dev).manual_seed(3)
encs = [torch.randn((1500, D), generator=g, device=dev) for _ in range(16)]
prefix = [50361] + [1000 + i for i in range(196)] + [50258, 50259, 50360]
max_length = len(prefix) + steps
bias = torch.zeros(V, device=dev)
bias[[1, 2, 7, EOS]] = float("-inf")
begin = bias.clone()
begin[220] = float("-inf")


def gens(n):
    return [torch.Generator(device=dev).manual_seed(100 + i) for i in range(n)]


def host_loop():
    dec.start(encs[0][None], 1)
    return [dec.sample_search(prefix, EOS, max_length, lambda pos: begin if pos == len(prefix) else bias, rules,
                              len(prefix), temperature=T, generator=gens(1)[0])[0]]


def on_device(n):
    return lambda: [s for s, _ in dec.sample_windows([(e, prefix) for e in encs[:n]], EOS, max_length, bias, begin,
                                                     rules, T, gens(n))]


paths = [("host loop (sample_search)", host_loop), ("sample_dev", on_device(1)),
         ("greedy_dev (the floor)", lambda: [dec.greedy_dev(encs[0], prefix, EOS, max_length, bias, begin, rules)]),
         ("sample_windows, 4 windows", on_device(4)), ("sample_windows, 16 windows", on_device(16))]
out = {}
for name, fn in paths:   # warm-up, and what each path decodes
    out[name] = fn()
    torch.cuda.synchronize()
times = {name: [] for name, _ in paths}
for _ in range(REPEATS):
    for name, fn in paths:
        torch.cuda.synchronize()
        t = time.perf_counter()
        seqs = fn()
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t) * 1e3 / sum(len(s) - len(prefix) for s in seqs))
same = out["sample_dev"][0] == out[paths[0][0]][0]
print(f"{model}, {len(prefix)}-token prefix, {steps} tokens per window, temperature {T}, timestamp rules on; "
      f"sample_dev tokens == host loop tokens: {same}")
print(f"{'path':<36} {'ms per (window-)token, each repeat':<36} {'min':>7} {'max':>7}")
for name, _ in paths:
    ts = times[name]
    print(f"{name:<36} {'  '.join(f'{x:.3f}' for x in ts):<36} {min(ts):7.3f} {max(ts):7.3f}")
