"""The beam path's three token-choice launches by themselves (tools/decode_bench.py times the decode step, which ends at
the logits): cbw_timestamp_rules, cbw_logprob_topk (CBW_TOPK_SPLIT=0 in the environment: its one-pass kernel) and
cbw_beam_select on random large-v3-sized logits, at 5 and 16 rows with k = 2 x rows (<= 16).  Microseconds per launch
from device events around 200 back-to-back launches, three repeats after a warm-up.
usage: python tools/token_select_bench.py"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
from cbw import _lib  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda:0")
V, LD, TB, NO_TS, EOS = 51866, 51968, 50365, 50364, 50257
N, REPEATS = 200, 3


def timed(fn):
    for _ in range(20):
        fn()
    out = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / N * 1e3)
    return ", ".join(f"{t:.2f}" for t in out)


g = torch.Generator(device=dev).manual_seed(0)
st = _lib.stream_handle()
print(f"token choice, V {V}, us per launch x {REPEATS} (CBW_TOPK_SPLIT={os.environ.get('CBW_TOPK_SPLIT', 'unset')})")
for B in (5, 16):
    k = min(2 * B, 16)
    x = torch.randn((B, LD), generator=g, device=dev) * 4
    bias = torch.zeros(V, device=dev)
    bias[[1, 2, 7]] = float("-inf")
    state = torch.tensor([[0, 1, TB + 7, 0]] * B, dtype=torch.int32, device=dev)
    tsb = torch.empty((B, V), device=dev)
    lp = torch.empty((B, k), device=dev)
    idx = torch.empty((B, k), dtype=torch.int32, device=dev)
    scores = torch.zeros(B, dtype=torch.float64, device=dev)
    cs = torch.empty(k, dtype=torch.float64, device=dev)
    cr, ct = (torch.empty(k, dtype=torch.int32, device=dev) for _ in range(2))
    tok, par = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    ok = torch.empty(1, dtype=torch.int32, device=dev)
    ts_state = torch.tensor([[3, 17, TB + 6, TB + 6]] * B, dtype=torch.int32, device=dev)
    ts0, st_out = ts_state.clone(), torch.empty((B, 4), dtype=torch.int32, device=dev)

    def rules():
        _lib.check(lib.cbw_timestamp_rules(x.data_ptr(), B, V, LD, bias.data_ptr(), state.data_ptr(), TB, NO_TS, EOS,
                                           50, tsb.data_ptr(), st), "rules")

    def topk():
        _lib.check(lib.cbw_logprob_topk(x.data_ptr(), B, V, LD, tsb.data_ptr(), V, k, lp.data_ptr(), idx.data_ptr(),
                                        st), "topk")

    def beam():   # count 0: the history state stays put over the repeats
        _lib.check(lib.cbw_beam_select(lp.data_ptr(), idx.data_ptr(), B, k, EOS, scores.data_ptr(), cs.data_ptr(),
                                       cr.data_ptr(), ct.data_ptr(), tok.data_ptr(), par.data_ptr(), ok.data_ptr(),
                                       ts_state.data_ptr(), st_out.data_ptr(), TB, 0, st), "beam")

    print(f"  rows {B:2d} k {k:2d}: rules {timed(rules)} | top-k {timed(topk)} | beam select {timed(beam)}")
    assert ts_state.tolist() == ts0.tolist()
