"""Time the fp32 re-scoring path (cbw_kws_rescore) on LEF pairs (large-v3 D, maps 75x750).

RS_MODE=cnn12: the exact tiers of CB-Whisper's own 12-channel spotter instead (cbw_kws_rescore_resized / _x3): RS_N
ragged keywords (20-192 frames) of D 1280 against 1500 utterance frames, maps (150, 750); per tier the time per
selected keyword, the share of it the fp32 front takes (similarity rows + resize, timed alone over the same passes of
32), and the bf16 pass (cbw_kws_score_resized) over the same keywords beside them.  HIP events around RS_REPS calls
after a warm-up call.

RS_MODE=cnn12_batch: RS_B (4) segments against RS_K (1000) such keywords in one pass (cbw_kws_score_resized_batch,
KwsEngine.score_resized_batch_exact at a band of 3 % of the pairs) against the loop of per-utterance calls, each of
RS_REPS calls timed on its own, and sim_rows_bf16_kernel alone on RS_PC (64) pairs."""
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
from cbw import _lib, synth  # noqa: E402
from cbw.kws import KwsEngine, pack_keywords  # noqa: E402

N = int(os.environ.get("RS_N", "64"))


def timed(fn, reps):
    """Mean milliseconds of fn() over reps calls between two events, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def cnn12():
    reps = int(os.environ.get("RS_REPS", "3"))
    L, D, Tu, size = 12, 1280, 1500, (150, 750)
    hp = dict(n_layers=L, embedding_dim=D, learn_features=False, proj_mlp=False)
    eng = KwsEngine(hp, synth.synth_kws_state_dict(seed=3, **hp)).build_exact()
    d = eng.device
    g = torch.Generator(device=d).manual_seed(0)
    lens = torch.randint(20, 193, (N,), generator=torch.Generator().manual_seed(0)).tolist()
    utt = torch.randn((L, Tu, D), generator=g, device=d)
    utt = utt / utt.norm(dim=-1, keepdim=True)
    kwd = []
    for T in lens:
        k = torch.randn((L, T, D), generator=g, device=d)
        kwd.append(k / k.norm(dim=-1, keepdim=True))
    p32 = pack_keywords(kwd, d, dtype=torch.float32)
    p16 = pack_keywords(kwd, d)
    del kwd
    sel = torch.arange(N, device=d, dtype=torch.int32)
    logits = torch.zeros((N, 2), device=d)
    t16 = timed(lambda: eng.score_resized(utt, p16, size), reps)
    print(f"cnn12 {N} keywords, mean {sum(lens) / N:.0f} frames: bf16 score_resized {t16:.1f} ms = {t16 / N:.3f} ms per "
          f"keyword")
    # the front alone, in the fp32 tier's passes of 32
    rows_k, off = p32
    off_dev = off.to(d)
    tk_max, ld, P = max(lens), (Tu + 63) // 64 * 64, 32
    rows = torch.empty((P, L, tk_max, ld), device=d)
    maps = torch.empty((P, size[0], size[1], L), device=d)
    st = _lib.stream_handle()

    def front(resize=True):
        for c0 in range(0, N, P):
            cn = min(P, N - c0)
            s = sel[c0:c0 + cn]
            _lib.check(eng.lib.cbw_kws_sim_rows_f32(utt.data_ptr(), Tu, rows_k.data_ptr(), rows_k.shape[1], D, L,
                                                    off_dev.data_ptr(), N, s.data_ptr(), cn, tk_max, ld, rows.data_ptr(),
                                                    st), "cbw_kws_sim_rows_f32")
            if resize:
                _lib.check(eng.lib.cbw_kws_sim_resize_f32(rows.data_ptr(), Tu, rows_k.shape[1], L, off_dev.data_ptr(), N,
                                                          s.data_ptr(), cn, tk_max, ld, size[0], size[1], maps.data_ptr(),
                                                          st), "cbw_kws_sim_resize_f32")
    tf, tr = timed(front, reps), timed(lambda: front(False), reps)
    print(f"  fp32 front alone: {tf:.1f} ms = {tf / N:.3f} ms per keyword (similarity rows {tr / N:.3f}, resize "
          f"{(tf - tr) / N:.3f})")
    for tier in ("x3", "f32"):
        t = timed(lambda: eng.rescore_resized(utt, p32, size, logits, sel, tier=tier, trusted=True), reps)
        print(f"  tier {tier}: {t:.1f} ms = {t / N:.3f} ms per keyword; the front is {100 * tf / t:.0f} % of it; "
              f"{t / t16:.1f} x the bf16 pass")


def each(fn, reps):
    """Milliseconds of each of reps calls of fn() (one event pair per call), after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def cnn12_batch():
    """RS_MODE=cnn12_batch: B segments against RS_K ragged keywords in one pass (cbw_kws_score_resized_batch,
    KwsEngine.score_resized_batch_exact) against the loop of B per-utterance calls, both in this process; then
    sim_rows_bf16_kernel alone on one chunk of pairs."""
    reps = int(os.environ.get("RS_REPS", "3"))
    K, B = int(os.environ.get("RS_K", "1000")), int(os.environ.get("RS_B", "4"))
    L, D, Tu, size = 12, 1280, 1500, (150, 750)
    hp = dict(n_layers=L, embedding_dim=D, learn_features=False, proj_mlp=False)
    eng = KwsEngine(hp, synth.synth_kws_state_dict(seed=3, **hp)).build_exact()
    d = eng.device
    g = torch.Generator(device=d).manual_seed(0)
    lens = torch.randint(20, 193, (K,), generator=torch.Generator().manual_seed(0)).tolist()
    utt = torch.randn((B, L, Tu, D), generator=g, device=d)
    utt = utt / utt.norm(dim=-1, keepdim=True)
    kwd = []
    for T in lens:
        k = torch.randn((L, T, D), generator=g, device=d)
        kwd.append(k / k.norm(dim=-1, keepdim=True))
    p32 = pack_keywords(kwd, d, dtype=torch.float32)
    p16 = pack_keywords(kwd, d)
    del kwd
    utt16 = utt.to(torch.bfloat16)

    def fmt(ts):
        return f"{sum(ts) / len(ts):.1f} ms (" + ", ".join(f"{t:.1f}" for t in ts) + ")"
    print(f"cnn12_batch B {B}, K {K} keywords, mean {sum(lens) / K:.0f} frames, chunk "
          f"{eng.default_chunk(*size, budget_bytes=1 << 30)}")
    loop = each(lambda: [eng.score_resized(utt16[b], p16, size) for b in range(B)], reps)
    batch = each(lambda: eng.score_resized_batch(utt16, p16, size), reps)
    print(f"  bf16 pass: loop of {B} score_resized {fmt(loop)}; score_resized_batch {fmt(batch)}; batch / loop "
          f"{sum(batch) / sum(loop):.3f}, loop spread {(max(loop) - min(loop)) / (sum(loop) / reps) * 100:.1f} %")
    # a band that selects a few percent of the pairs
    lg = eng.score_resized_batch(utt16, p16, size)
    dist = (torch.softmax(lg.view(-1, 2).double(), -1)[:, 1] - 0.5).abs()
    band = float(torch.quantile(dist, 0.03))
    n_in = int((dist <= band).sum())
    loop = each(lambda: [eng.score_resized_exact(utt[b], p16, p32, size, band) for b in range(B)], reps)
    batch = each(lambda: eng.score_resized_batch_exact(utt, p16, p32, size, band), reps)
    print(f"  cascade, band {band:.3e} ({n_in} of {B * K} pairs): loop of {B} score_resized_exact {fmt(loop)}; "
          f"score_resized_batch_exact {fmt(batch)}; batch / loop {sum(batch) / sum(loop):.3f}, loop spread "
          f"{(max(loop) - min(loop)) / (sum(loop) / reps) * 100:.1f} %")
    # the rows kernel alone: one chunk of pairs that straddles an utterance boundary
    rows_k, off = p16
    off_dev = off.to(d)
    pc = min(int(os.environ.get("RS_PC", "64")), B * K)
    p0 = max(0, min(K - pc // 2, B * K - pc))
    n_rows = sum(lens[p % K] for p in range(p0, p0 + pc))
    ld = (Tu + 127) // 128 * 128
    rows = torch.empty((L, n_rows, ld), device=d)
    st = _lib.stream_handle()
    t = timed(lambda: _lib.check(eng.lib.cbw_kws_sim_rows_bf16(utt16.data_ptr(), B, Tu, rows_k.data_ptr(),
                                                               rows_k.shape[1], D, L, off_dev.data_ptr(), K, p0, pc, ld,
                                                               rows.data_ptr(), st), "cbw_kws_sim_rows_bf16"), 10)
    fl = 2.0 * L * n_rows * Tu * D
    print(f"  sim_rows_bf16_kernel alone, pairs [{p0}, {p0 + pc}) = {n_rows} rows: {t * 1e3:.0f} us, "
          f"{fl / t / 1e9:.1f} TFLOP/s ({fl / pc / 1e9:.1f} GFLOP per pair)")


if os.environ.get("RS_MODE") == "cnn12":
    cnn12()
    sys.exit(0)
if os.environ.get("RS_MODE") == "cnn12_batch":
    cnn12_batch()
    sys.exit(0)

hp = dict(n_layers=3, embedding_dim=1280, learn_features=True, proj_mlp=True, frames_conv=True)
eng = KwsEngine(hp, synth.synth_kws_state_dict(seed=0, **hp))
d = eng.device
g = torch.Generator(device=d).manual_seed(0)
kwd = torch.randn((N, 3, 75, 64), generator=g, device=d)
kwd = kwd / kwd.norm(dim=-1, keepdim=True)
utt = torch.randn((3, 750, 64), generator=g, device=d)
utt = utt / utt.norm(dim=-1, keepdim=True)
km, um = torch.ones((N, 3, 75), device=d), torch.ones((3, 750), device=d)
logits = torch.zeros((N, 2), device=d)
sel = torch.arange(N, device=d, dtype=torch.int32)
eng.rescore(utt, um, kwd, km, logits, sel)
torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(3):
    eng.rescore(utt, um, kwd, km, logits, sel)
torch.cuda.synchronize()
dt = (time.perf_counter() - t) / 3
print(f"fp32 re-score: {N} pairs in {dt * 1e3:.1f} ms -> {N / dt:.0f} pairs/s, {N * 10.08e9 / dt / 1e12:.1f} TFLOP/s")
