"""Token-level timestamps for a batch of rows against the same rows one by one, WINDOWS = 16 windows of n = 10 heads
over 1500 frames at T in {32, 128, 447} positions, every case ending with its timestamps on the host:
  * extraction: one extract_token_timestamps_batch_dev call (cbw_align_matrix_batch, cbw_dtw_dev_batch, one copy back)
    against 16 extract_token_timestamps_dev calls (two launches and one blocking copy each);
  * the two batched kernels on their own at T = 447, beside the single-window kernels on one window;
  * the weights: DecoderEngine.cross_attn_probs_windows (16 cbw_decoder_cross_attn_probs_slot calls on one lock-step
    state) against 16 start() + cross_attn_probs() on a one-window state, TSB_MODEL widths (default large-v3-2l:
    two decoder layers of large-v3's widths) with seeded random weights.
Device-event time per case, the cases alternating in one process, REPEATS windows of ITERS calls each after a warm-up.
usage: python tools/token_ts_batch_bench.py"""
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
from cbw import _lib, synth  # noqa: E402
from cbw.decoder import DecoderEngine  # noqa: E402
from cbw.token_timestamps import (alignment_pairs, extract_token_timestamps_batch_dev,  # noqa: E402
                                  extract_token_timestamps_dev)

ITERS, REPEATS = 10, 3
WINDOWS, N, F = 16, 10, 1500
dev = torch.device("cuda:0")
g = np.random.default_rng(0)
lib = _lib.load()
paths = []
weights = {}
for T in (32, 128, 447):
    flat = torch.softmax(torch.from_numpy(g.standard_normal((WINDOWS, N, T, F)).astype(np.float32)), -1).to(dev)
    ws = weights[T] = [flat[i] for i in range(WINDOWS)]   # views of one buffer, as cross_attn_probs_windows returns them
    paths.append((f"T {T}: 16 single-window calls", lambda ws=ws: [extract_token_timestamps_dev(w, 7, 0.02) for w in ws]))
    paths.append((f"T {T}: one batched call", lambda ws=ws: extract_token_timestamps_batch_dev(ws, 7, 0.02)))
    same = all(torch.equal(a, b) for a, b in zip(paths[-1][1](), paths[-2][1]()))
    print(f"T {T}: the two give the same timestamps: {same}")

T = 447
nb = lib.cbw_token_ts_ws_bytes(T, F)
table = (_lib.TokenTsWindow * WINDOWS)(*[_lib.TokenTsWindow(T, 0, T, F, i * N * T * F, i * T * F, i * nb)
                                         for i in range(WINDOWS)])
probs = weights[T][0]
matrix = torch.empty((WINDOWS, T, F), dtype=torch.float32, device=dev)
out = torch.empty(WINDOWS * T + WINDOWS, dtype=torch.int32, device=dev)
ws_all = torch.empty(WINDOWS * nb, dtype=torch.uint8, device=dev)


def align_batch():
    _lib.check(lib.cbw_align_matrix_batch(probs.data_ptr(), N, ctypes.addressof(table), WINDOWS, 7, matrix.data_ptr(),
                                          out.data_ptr() + 4 * WINDOWS * T, ws_all.data_ptr(), ws_all.numel(),
                                          _lib.stream_handle()), "cbw_align_matrix_batch")


def dtw_batch():
    _lib.check(lib.cbw_dtw_dev_batch(matrix.data_ptr(), ctypes.addressof(table), WINDOWS, out.data_ptr(), T,
                                     ws_all.data_ptr(), ws_all.numel(), _lib.stream_handle()), "cbw_dtw_dev_batch")


def align_one():
    _lib.check(lib.cbw_align_matrix(probs.data_ptr(), N, T, 0, T, F, 7, matrix.data_ptr(), out.data_ptr() + 4 * T,
                                    ws_all.data_ptr(), nb, _lib.stream_handle()), "cbw_align_matrix")


def dtw_one():
    _lib.check(lib.cbw_dtw_dev(matrix.data_ptr(), T, F, out.data_ptr(), None, None, None, ws_all.data_ptr(), nb,
                               _lib.stream_handle()), "cbw_dtw_dev")


paths += [(f"T {T}: cbw_align_matrix, 1 window", align_one), (f"T {T}: cbw_align_matrix_batch, 16", align_batch),
          (f"T {T}: cbw_dtw_dev, 1 window", dtw_one), (f"T {T}: cbw_dtw_dev_batch, 16", dtw_batch)]

model = os.environ.get("TSB_MODEL", "large-v3-2l")
cfg = synth.WHISPER_DECODERS[model]
eng = DecoderEngine(cfg, synth.synth_whisper_decoder_state_dict(model, seed=0))
heads = alignment_pairs([[l % cfg[2], (3 * l + 1) % cfg[3]] for l in range(N)])
gen = torch.Generator(device="cuda").manual_seed(1)
encs = [torch.randn((1500, cfg[1]), generator=gen, device=dev) for _ in range(WINDOWS)]
for T in (32, 128, 447):
    rows = [[50258, 50259, 50359] + [int(t) for t in g.integers(300, 50000, T - 3)] for _ in range(WINDOWS)]

    def loop(rows=rows):
        out = []
        for e, r in zip(encs, rows):
            eng.start(e[None], 1)
            out.append(eng.cross_attn_probs(r, heads))
        return out
    paths.append((f"T {T}: 16 start + cross_attn_probs", loop))
    paths.append((f"T {T}: 16 slot probes, one state", lambda rows=rows: eng.cross_attn_probs_windows(list(zip(encs, rows)), heads)))
    same = all(torch.equal(a, b) for a, b in zip(paths[-1][1](), paths[-2][1]()))
    print(f"T {T}: the two give the same probabilities: {same}")

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
    print(f"{name:40s} us per case: " + ", ".join(f"{t:.1f}" for t in times[name]))
