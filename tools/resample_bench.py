"""cbw.whisper.resample on 30 s clips (the log-mel window) at the rates a keyword database meets: device-event time of
the whole call (the table's upload and the kernel) per clip, the cases alternating in one process, REPEATS windows of
ITERS calls each after a warm-up, next to cbw_mel on the 16 kHz result for scale.
usage: python tools/resample_bench.py"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
from cbw.whisper import log_mel, resample  # noqa: E402

ITERS, REPEATS = 200, 3
dev = torch.device("cuda:0")
g = np.random.default_rng(0)
cases = [(8000, 1), (24000, 1), (48000, 2), (22050, 1), (44100, 2), (16000, 2)]
clips = {c: torch.from_numpy(g.standard_normal((c[1], 30 * c[0])).astype(np.float32)).to(dev) for c in cases}
mono = resample(clips[(24000, 1)], 24000)
paths = [(f"{sr} Hz x {ch} ch -> 16000", (lambda x=clips[(sr, ch)], sr=sr: resample(x, sr))) for sr, ch in cases]
paths.append(("cbw_mel of 30 s at 16000 (80 mel)", lambda: log_mel(mono, 80)))
for _, fn in paths:
    fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in paths}
for _ in range(REPEATS):
    for name, fn in paths:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        torch.cuda.synchronize()
        times[name].append(a.elapsed_time(b) / ITERS * 1e3)
for name, _ in paths:
    print(f"{name:40s} us per call: " + ", ".join(f"{t:.1f}" for t in times[name]))
