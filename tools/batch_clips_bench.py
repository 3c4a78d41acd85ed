"""A batch of short clips in one call against the same clips one by one: PBAWhisper.generate_batch(N clips) vs N
generate calls, large-v3 widths with seeded random weights, 5 beams, a keyword prompt of PROMPT tokens per clip from a
stub spotter (the spotter itself is not timed here), at most MAX_NEW tokens.  The two are run alternately for ROUNDS
rounds after one warm-up each; wall clock around work that ends in a device synchronise.  Prints one JSON line with
clips/s of each (median, min, max) and whether the outputs were equal.  With --token-timestamps the two cases are
generate_batch without and with return_token_timestamps=True (ten alignment heads, as large-v3 has): what the token
timestamps of every clip cost the call.
usage: python tools/batch_clips_bench.py [--token-timestamps] [clips] [max_new_tokens] [rounds] [prompt_tokens]"""
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
from cbw import synth  # noqa: E402
from cbw.whisper import log_mel  # noqa: E402
from model.pba_whisper import PBAWhisper  # noqa: E402

token_ts = "--token-timestamps" in sys.argv
sys.argv = [a for a in sys.argv if a != "--token-timestamps"]
clips = int(sys.argv[1]) if len(sys.argv) > 1 else 16
max_new = int(sys.argv[2]) if len(sys.argv) > 2 else 64
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
n_prompt = int(sys.argv[4]) if len(sys.argv) > 4 else 64
model = os.environ.get("BCB_MODEL", "large-v3")
beams = 5
dev = torch.device("cuda:0")
enc_cfg, dec_cfg = synth.WHISPER_CONFIGS[model], synth.WHISPER_DECODERS[model]
sd = {"model.encoder." + k: v for k, v in synth.synth_whisper_encoder_state_dict(model, seed=0).items()}
sd.update({"model.decoder." + k: v for k, v in synth.synth_whisper_decoder_state_dict(model, seed=0).items()})
heads = [[(7 + 2 * i) % dec_cfg[2], (5 * i + 1) % dec_cfg[3]] for i in range(10)] if token_ts else None
w = PBAWhisper(enc_cfg, dec_cfg, sd, device=dev, alignment_heads=heads)
del sd
feats = torch.stack([log_mel(torch.from_numpy(synth.synth_clip(i)).to(dev), enc_cfg[0])[0] for i in range(clips)])


def spot(input_features, start_of_prev=False):
    return [[w.tokens.startofprev] + [1000 + (7919 * (i + 1)) % 40000 for i in range(n_prompt)] for _ in input_features]


kw = dict(task="transcribe", language="english", num_beams=beams, max_new_tokens=max_new, keyword_spotting=spot)


def one_by_one():
    return [w.generate(input_features=feats[i:i + 1], **kw) for i in range(clips)]


def batch():
    return w.generate_batch(feats, **kw)


def batch_ts():
    return w.generate_batch(feats, return_token_timestamps=True, **kw)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


if token_ts:
    _, b = timed(batch)
    _, c = timed(batch_ts)
    equal = [x.tolist() for x in b] == [x["sequences"].tolist() for x in c]
    t0, t1 = [], []
    for r in range(rounds):
        t0.append(timed(batch)[0])
        t1.append(timed(batch_ts)[0])
        print(f"round {r}: batch {clips / t0[-1]:.3f} clips/s, with token timestamps {clips / t1[-1]:.3f} clips/s",
              flush=True)
    rate = lambda ts: {"median": round(clips / statistics.median(ts), 3), "min": round(clips / max(ts), 3),   # noqa: E731
                       "max": round(clips / min(ts), 3)}
    print(json.dumps({"model": model, "clips": clips, "beams": beams, "max_new_tokens": max_new,
                      "prompt_tokens": n_prompt, "tokens_returned": sum(x.shape[1] for x in b),
                      "sequences_equal": equal, "generate_batch_clips_per_s": rate(t0),
                      "generate_batch_token_timestamps_clips_per_s": rate(t1)}))
    sys.exit(0)
_, a = timed(one_by_one)
_, b = timed(batch)
equal = [x.tolist() for x in a] == [x.tolist() for x in b]
tokens = sum(x.shape[1] for x in b)
t1, tb = [], []
for r in range(rounds):
    t1.append(timed(one_by_one)[0])
    tb.append(timed(batch)[0])
    print(f"round {r}: one by one {clips / t1[-1]:.3f} clips/s, batch {clips / tb[-1]:.3f} clips/s", flush=True)
rate = lambda ts: {"median": round(clips / statistics.median(ts), 3), "min": round(clips / max(ts), 3),   # noqa: E731
                   "max": round(clips / min(ts), 3)}
print(json.dumps({"model": model, "clips": clips, "beams": beams, "max_new_tokens": max_new, "prompt_tokens": n_prompt,
                  "rows": w.decoder._shape[0], "wide": os.environ.get("CBW_DEC_WIDE", "1") != "0",
                  "tokens_returned": tokens, "outputs_equal": equal, "generate_clips_per_s": rate(t1),
                  "generate_batch_clips_per_s": rate(tb)}))
