"""Pair lists and utterance batches in one pass (cbw_kws_score_pairs) against the per-utterance loops they replace,
at real sizes: LEF / ResNet-50, D = 1280, features 150 x 1500 (maps 75 x 750), seeded weights and features.

  paired batch    K pairs (utterance i, keyword i), the training / validation shape: K ``score`` calls of one pair
                  each (the loop KWSModel.forward ran before score_pairs) against one ``score_pairs`` call;
  utterance batch B utterances x K keywords: B sequential ``score`` calls against one ``score_batch`` call.

Device-event timing around each variant, the two variants alternating within a repeat, warm-up first, medians over
the repeats; the outputs of the two variants are compared bit for bit.
usage: python tools/pairs_bench.py [paired K = 50] [B = 8] [K = 200] [repeats = 7]"""
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
from cbw import synth  # noqa: E402
from cbw.kws import KwsEngine  # noqa: E402

KP = int(sys.argv[1]) if len(sys.argv) > 1 else 50
B = int(sys.argv[2]) if len(sys.argv) > 2 else 8
K = int(sys.argv[3]) if len(sys.argv) > 3 else 200
REPEATS = max(5, int(sys.argv[4]) if len(sys.argv) > 4 else 7)
L, D, TK, TU = 3, 1280, 150, 1500

hp = dict(n_layers=L, embedding_dim=D, learn_features=True, proj_mlp=True, frames_conv=True, proj_mlp_units=64,
          resnet_version="resnet-50")
eng = KwsEngine(hp, synth.synth_kws_state_dict(seed=0, **hp))
dev = eng.device
gen = torch.Generator(device=dev)
gen.manual_seed(11)


def projected(n, T):
    """n seeded sequences of T L2-normalised frames, projected (bf16 [n, L, T', 64]); ragged lengths in the masks."""
    out, masks = [], []
    for i in range(0, n, 8):
        m = min(8, n - i)
        x = torch.randn((m, L, T, D), generator=gen, device=dev)
        x = x / x.norm(dim=-1, keepdim=True)
        lens = torch.randint(T // 2, T + 1, (m,), generator=gen, device=dev)
        mask = (torch.arange(T, device=dev)[None, None, :] < lens[:, None, None]).float().expand(m, L, T).contiguous()
        p, pm = eng.project(x * mask[..., None], mask)
        out.append(p)
        masks.append(pm)
    return torch.cat(out), torch.cat(masks)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def compare(name, loop, one, pairs):
    for _ in range(2):   # warm-up of every shape the timed window uses
        ref, got = loop(), one()
    torch.cuda.synchronize()
    same = torch.equal(ref.reshape(-1, 2), got.reshape(-1, 2))
    t_loop, t_one = [], []
    for _ in range(REPEATS):
        t_loop.append(timed(loop)[0])
        t_one.append(timed(one)[0])
    ml, mo = statistics.median(t_loop), statistics.median(t_one)
    print(f"{name}: {pairs} pairs; loop {ml:.2f} ms (min {min(t_loop):.2f}, max {max(t_loop):.2f}), one call "
          f"{mo:.2f} ms (min {min(t_one):.2f}, max {max(t_one):.2f}), medians of {REPEATS}; x{ml / mo:.2f}; "
          f"{pairs / mo * 1e3:.0f} pairs/s in one call; outputs bit-identical: {same}")


Tk, Tu = eng.out_frames(TK), eng.out_frames(TU)
chunk = eng.default_chunk(Tk, Tu)
print(f"LEF ResNet-50 D={D} maps {Tk}x{Tu}; default_chunk {chunk}; streams CBW_KWS_STREAMS="
      f"{os.environ.get('CBW_KWS_STREAMS', 'default')}")

pk, pkm = projected(max(KP, K), TK)
pu, pum = projected(max(KP, B), TU)

# paired batch: pair i = (utterance i, keyword i)
ku, kum, kk, kkm = pu[:KP].contiguous(), pum[:KP].contiguous(), pk[:KP].contiguous(), pkm[:KP].contiguous()
ar = torch.arange(KP, dtype=torch.int32, device=dev)
print(f"paired batch: chunks in one call {-(-KP // chunk)}, in the loop {KP} x 1")
compare(f"paired batch K={KP}",
        lambda: torch.cat([eng.score(ku[i], kum[i], kk[i:i + 1], kkm[i:i + 1]) for i in range(KP)]),
        lambda: eng.score_pairs(ku, kum, kk, kkm, ar, ar, trusted=True), KP)

# utterance batch: every utterance against every keyword
bu, bum, bk, bkm = pu[:B].contiguous(), pum[:B].contiguous(), pk[:K].contiguous(), pkm[:K].contiguous()
print(f"utterance batch: chunks in one call {-(-(B * K) // chunk)}, in the loop {B} x {-(-K // chunk)}")
compare(f"utterance batch B={B} x K={K}",
        lambda: torch.stack([eng.score(bu[b], bum[b], bk, bkm) for b in range(B)]),
        lambda: eng.score_batch(bu, bum, bk, bkm), B * K)
