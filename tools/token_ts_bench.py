"""Token-level timestamps behind the alignment heads' weights: cbw.token_timestamps.extract_token_timestamps (torch
ops, a copy of the matrix to the host, cbw_dtw there) against extract_token_timestamps_dev (cbw_align_matrix and
cbw_dtw_dev, one copy back of T + 1 integers) on random softmax weights of n = 10 heads over 1500 frames at
T in {32, 128, 447} positions, each call ending with its timestamps on the host: device-event time per call, the cases
alternating in one process, REPEATS windows of ITERS calls each after a warm-up; for T = 447 the two kernels on their
own.
usage: python tools/token_ts_bench.py"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
from cbw import _lib  # noqa: E402
from cbw.token_timestamps import extract_token_timestamps, extract_token_timestamps_dev  # noqa: E402

ITERS, REPEATS = 20, 3
N, F = 10, 1500
dev = torch.device("cuda:0")
g = np.random.default_rng(0)
lib = _lib.load()
weights = {T: torch.softmax(torch.from_numpy(g.standard_normal((N, T, F)).astype(np.float32)), -1).to(dev)
           for T in (32, 128, 447)}
paths = []
for T, w in weights.items():
    paths.append((f"T {T}: host path", lambda w=w: extract_token_timestamps(w, 7, 0.02)))
    paths.append((f"T {T}: device path", lambda w=w: extract_token_timestamps_dev(w, 7, 0.02)))
    print(f"T {T}: the two paths give the same timestamps: {torch.equal(paths[-1][1](), paths[-2][1]())}")

T = 447
w = weights[T]
nb = lib.cbw_token_ts_ws_bytes(T, F)
matrix = torch.empty((T, F), dtype=torch.float32, device=dev)
out = torch.empty(T + 1, dtype=torch.int32, device=dev)
ws = torch.empty(nb, dtype=torch.uint8, device=dev)


def align():
    _lib.check(lib.cbw_align_matrix(w.data_ptr(), N, T, 0, T, F, 7, matrix.data_ptr(), out.data_ptr() + 4 * T,
                                    ws.data_ptr(), nb, _lib.stream_handle()), "cbw_align_matrix")


def dtw():
    _lib.check(lib.cbw_dtw_dev(matrix.data_ptr(), T, F, out.data_ptr(), None, None, None, ws.data_ptr(), nb,
                               _lib.stream_handle()), "cbw_dtw_dev")


paths += [(f"T {T}: cbw_align_matrix alone", align), (f"T {T}: cbw_dtw_dev alone", dtw)]
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
    print(f"{name:32s} us per call: " + ", ".join(f"{t:.1f}" for t in times[name]))
