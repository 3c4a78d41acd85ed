"""Exact decisions for a batch of clips in one call (KwsEngine.score_batch_exact) against the B per-clip
``score_exact`` calls it replaces, at bench.py's shapes: the large-v3 encoder's LEF features of B seeded clips
(D = 1280, 1500 frames -> maps 75 x 750), bench.py's seeded keyword database and bias calibration, band 0.015 into
the compensated tier and 1e-4 into fp32, chunk 1112.

Device-event timing around each variant, the two variants alternating within a repeat, warm-up of both first,
medians over the repeats; the logits of the two variants are compared bit for bit and the band counts printed.
Needs the GPU: there is no CPU path.
usage: python tools/batch_exact_bench.py [B = 4] [K = 10000] [repeats = 7]"""
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
import bench  # noqa: E402
from cbw import synth  # noqa: E402
from cbw.kws import KwsEngine  # noqa: E402
from cbw.whisper import EncoderEngine, default_layer_ids, log_mel  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
K = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
REPEATS = max(5, int(sys.argv[3]) if len(sys.argv) > 3 else 7)
THR, BAND, BAND_X3, CHUNK, N_CAL = 0.5, 0.015, 1e-4, 1112, 512

assert torch.cuda.is_available(), "tools/batch_exact_bench.py measures on the GPU"
dev = torch.device("cuda:0")
cfg = synth.WHISPER_CONFIGS["large-v3"]
n_mel, D, n_layers = cfg[0], cfg[1], cfg[2]
enc = EncoderEngine(cfg, synth.synth_whisper_encoder_state_dict("large-v3", seed=0), dev)
ids = default_layer_ids(n_layers)
hp = dict(n_layers=3, embedding_dim=D, learn_features=True, proj_mlp=True, frames_conv=True, proj_mlp_units=64,
          resnet_version="resnet-50", threshold=THR)
kws = KwsEngine(hp, synth.synth_kws_state_dict(seed=0, **hp), dev)
db, dbm, db32 = bench.build_keyword_db(kws, K, D, f32=True)
bench.calibrate_kws(kws, enc, ids, n_mel, K, D, min(N_CAL, K), dev)

hs = []
for clip in range(B):
    _, mel = log_mel(torch.from_numpy(synth.synth_clip(clip)).to(dev), n_mel, packed=True)
    hs.append(enc.hidden_states(mel, ids, normalize=True))
hs = torch.cat(hs)
um = torch.ones((B, 3, hs.shape[-2]), device=dev)
pu, pum = kws.project(hs, um)
pu32, _ = kws.project_f32(hs, um)
del enc, hs
print(f"LEF ResNet-50 D={D}: {B} clips x {K} keywords, maps {db.shape[2]}x{pu.shape[2]}, band {BAND} -> x3, "
      f"{BAND_X3} -> fp32, chunk {CHUNK}")


def loop():
    out = [kws.score_exact(pu[b], pum[b], db, dbm, pu32[b], db32, THR, BAND, chunk=CHUNK, band_x3=BAND_X3)
           for b in range(B)]
    return torch.stack([lg for lg, _ in out]), {k: sum(st[k] for _, st in out) for k in ("band", "fp32", "bf16")}


def one():
    return kws.score_batch_exact(pu, pum, db, dbm, pu32, db32, THR, BAND, chunk=CHUNK, band_x3=BAND_X3)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


for _ in range(2):   # warm-up of every shape the timed window uses
    (ref, ref_stats), (got, stats) = loop(), one()
torch.cuda.synchronize()
same = torch.equal(ref, got)
t_loop, t_one = [], []
for _ in range(REPEATS):
    t_loop.append(timed(loop)[0])
    t_one.append(timed(one)[0])
ml, mo = statistics.median(t_loop), statistics.median(t_one)
print(f"{B} score_exact calls: {ml:.2f} ms (min {min(t_loop):.2f}, max {max(t_loop):.2f}); one score_batch_exact call: "
      f"{mo:.2f} ms (min {min(t_one):.2f}, max {max(t_one):.2f}); medians of {REPEATS}; x{ml / mo:.2f}")
print(f"stats loop {ref_stats}, one call {stats}; logits bit-identical: {same}")
sys.exit(0 if same and stats == ref_stats else 1)
