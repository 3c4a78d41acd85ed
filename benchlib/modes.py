"""bench.py's non-headline modes: --plumbing (the multi-rank envelope on the CPU), --mode longform / e2e (C5 and
CBWhisper.forward end to end) and --mode api (the drop-in KWSModel.test_step path).  The headline clip / kwshard
modes stay in bench.py."""
from __future__ import annotations

import hashlib
import json
import os
import time

import numpy as np
import torch

from benchlib.common import (OP_POSITIVE_FRAC, _init_dist, _rank_device, build_keyword_db, calibrate_fp8_tier,
                             calibrate_kws, dump_outputs, keyword_hs, kws_hparams, log, rank_times,
                             realistic_bias_shift)


def run_plumbing(args):
    """--plumbing (test only, no GPU): the multi-rank envelope of the clip bench on the CPU -- gloo group, barrier,
    K timed steps, barrier, all-gather of every rank's elapsed time, max over ranks, rank 0's JSON line.  A step is a
    sleep of (rank + 1) x --plumbing-ms, so the slowest rank is known; nothing here measures the hot path."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    import torch.distributed as dist
    if world == 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29543")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    dist.init_process_group("gloo")
    dev = torch.device("cpu")
    step_s = (rank + 1) * args.plumbing_ms * 1e-3
    for _ in range(args.warmup):
        time.sleep(step_s)
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(step_s)
    dist.barrier()
    elapsed, per = rank_times(dist, time.perf_counter() - t0, dev)
    if rank == 0:
        print(json.dumps({"metric": "plumbing (no hot path)", "value": round(world * args.steps / elapsed, 4),
                          "unit": "steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
                          "scaling": "weak", "vs_baseline": None, "dtype": "none", "data": "none",
                          "config": {"workload": "plumbing"},
                          "rank_elapsed_s": [round(x, 6) for x in per]}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def run_longform(args):
    """C5 (BASELINE.json configs[4]): PBAWhisper long-form + LEF keyword spotting, clip-parallel across audios.
    One step = one synthetic audio of --audio-seconds per rank through the whole path: long-form log-mel of the
    audio (cbw_mel_long), then PBAWhisper.generate's seek loop (pba_whisper.py:343-475; return_timestamps,
    condition_on_prev_tokens, num_beams 5 -- CBWhisper.forward's long-form arguments, cb_whisper.py:166-178):
    per 30 s window the CB-Whisper keyword spotter (large-v3 hs[19..21] -> LEF -> ResNet-50 against K keywords,
    exact-decision tiers) builds the <|startofprev|> prompt, the window is encoded and decoded with the
    timestamp rules, and the seek moves to the last closed segment.  The windows of one audio are sequential
    (the seek depends on the decoded timestamps); ranks process independent audios, no collective but the
    timing max.  value = audio seconds transcribed per second (whole job)."""
    import tempfile
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dev = _rank_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        _init_dist(dist, dev)
    from cbw import synth
    from cbw.kws import KwsEngine
    from cbw.tokenizer import WhisperTokenizerLite
    from cbw.whisper import log_mel_long
    from model.cb_whisper import CBWhisper
    from model.pba_whisper import PBAWhisper
    import threading
    t_setup = time.time()
    enc_cfg, dec_cfg = synth.WHISPER_CONFIGS[args.model], synth.WHISPER_DECODERS[args.model]
    n_mel, D = enc_cfg[0], enc_cfg[1]
    tokdir = tempfile.mkdtemp(prefix="cbw_tok_")
    synth.write_synth_tokenizer(tokdir, dec_cfg[0])
    K = args.keywords
    exact = args.exact_band > 0
    e2e = args.mode == "e2e"
    if e2e:   # one 30 s clip per step and lane: the short-form path CBWhisper.forward takes
        args.audio_seconds, args.generate_batch = 30.0, 1
    A = max(1, args.audios_in_flight)
    G = max(1, args.generate_batch)   # audios per PBAWhisper.generate call (pba_whisper.py:351-475, batch_size > 1)
    words = [synth.TOKENIZER_WORDS[i % len(synth.TOKENIZER_WORDS)] + str(i) for i in range(K)]
    gen_kw = dict(task="transcribe", language="english", return_timestamps=True, condition_on_prev_tokens=True,
                  return_segments=True, num_beams=args.beams, do_sample=False, temperature=0)
    if args.max_new_tokens:
        gen_kw["max_new_tokens"] = args.max_new_tokens

    class Lane:
        """One audio in flight: its own PBAWhisper + spotter engines (the decoder state, the KWS workspace and the
        calibrated biases are per engine), HIP stream and host thread.  The lanes of a rank share the GPU: the
        decode steps are latency-bound chains of small launches that leave most CUs idle, which another lane's
        launches (spotting, encoder or decode) fill."""

        def __init__(self, j):
            self.whisper = PBAWhisper(enc_cfg, dec_cfg, wsd, suppress_tokens=[1, 2, 7], device=dev,
                                      tokenizer=WhisperTokenizerLite.from_dir(tokdir))
            kws_hp = kws_hparams(args.variant, D, args.threshold)
            from cbw.whisper import default_layer_ids
            ids = default_layer_ids(enc_cfg[2])
            kws_sd = synth.synth_kws_state_dict(seed=0, **kws_hp)
            self.kws = KwsEngine(kws_hp, kws_sd, dev)
            if args.operating_point != "synthetic":   # the clip bench's realistic / sparse point (class-1 bias lowered)
                if op_shift[0] is None:
                    op_shift[0] = realistic_bias_shift(self.kws, self.whisper.encoder, ids, n_mel, K, D, dev,
                                                       OP_POSITIVE_FRAC[args.operating_point])
                kws_sd = dict(kws_sd)
                b = np.array(kws_sd["model.classifier.1.bias"], dtype=np.float32).copy()
                b[1] -= op_shift[0]
                kws_sd["model.classifier.1.bias"] = b
                del self.kws
                self.kws = KwsEngine(kws_hp, kws_sd, dev)
            db, dbm, *db32 = build_keyword_db(self.kws, K, D, f32=exact)
            if exact and args.bias_calibrate > 0:   # the same calibration as the clip bench (the spotter's hs[19..21])
                calibrate_kws(self.kws, self.whisper.encoder, ids, n_mel, K, D, args.bias_calibrate, dev)
            fp8_band = None
            if args.fp8_first:   # the e4m3 first tier in front of the bf16 pass (C5 "fp8 MFMA")
                if not exact:
                    raise SystemExit("--fp8-first runs the exact tiers after it (--exact-band > 0)")
                fp8_band, self.fp8_err, _ = calibrate_fp8_tier(self.kws, self.whisper.encoder, ids, n_mel, K, D, dev)
                fp8_cal[0] = {"fp8_band": round(fp8_band, 5), "fp8_max_err_held_out": round(self.fp8_err, 5)}
            self.cb = CBWhisper.from_components(self.whisper, self.kws, self.whisper.encoder, words, db, dbm,
                                                num_beams=args.beams, keyword_feats32=db32[0] if exact else None,
                                                exact_band=args.exact_band, fp8_band=fp8_band,
                                                keyword_prompt_prepend="The topic of today's speech is, ah, ",
                                                keyword_prompt_append=". Okay, then I'll continue.",
                                                keyword_separator=", ")
            # --lane-priority (with lanes): the lane's decode runs on a high-priority stream and its spotting on a
            # normal-priority one, so another lane's compute-bound spotting does not delay the latency-bound decode
            prio = args.lane_priority and A > 1
            self.stream = torch.cuda.Stream(device=dev, priority=-1 if prio else 0)
            self.spot_stream = torch.cuda.Stream(device=dev, priority=0) if prio else None
            self.stats = {"windows": 0, "tokens": 0, "spotted": 0, "spot_s": 0.0, "transcript_tokens": 0}
            self.digests = {}   # audio index -> sha1 of its transcript's token ids
            self.tokens = {}    # audio index -> those token ids (--dump-outputs)
            self.error = None
            spot0 = self.cb.keyword_spotting

            def spotting(input_features, start_of_prev=False):
                t = time.perf_counter()
                if self.spot_stream is not None:
                    self.spot_stream.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(self.spot_stream):
                        out = spot0(input_features, start_of_prev)
                    torch.cuda.current_stream().wait_stream(self.spot_stream)
                else:
                    out = spot0(input_features, start_of_prev)   # ends on the host (prompt ids): its wall time is its cost
                self.stats["spot_s"] += time.perf_counter() - t
                self.stats["windows"] += input_features.shape[0]
                self.stats["spotted"] += sum(len(k) for k in self.cb.last_spotted)
                if self.stats["windows"] % 10 == 0:   # progress (a 30 min audio is ~60 windows)
                    log(f"[bench] longform lane {j}: {self.stats['windows']} windows")
                return out
            self.gen_kw = dict(gen_kw, keyword_spotting=spotting)
            if e2e:   # CBWhisper.forward calls its own keyword_spotting: the counting wrapper stands in for it
                self.cb.keyword_spotting = spotting
                tok = self.whisper.tokenizer
                self.last_ids = []

                def detok(ids):   # forward's detokenize hook: the transcript's token ids (special tokens dropped, as
                    self.last_ids = list(ids)   # skip_special_tokens)
                    return tok.decode(ids)
                self.cb.detokenize = detok
                self.decoded = []
                dw0 = self.whisper.decode_window

                def dw(enc_out, prefix, *a, **k):   # the decoded tokens after the forced prefix: the digest and count
                    out = dw0(enc_out, prefix, *a, **k)   # source (the returned transcript is sliced by the untruncated
                    seq = out[0] if isinstance(out, tuple) else out   # keyword prompt's length, pba_whisper.py:338,
                    self.decoded.append([int(t) for t in seq[len(prefix):]])   # so a long prompt leaves it empty)
                    return out
                self.whisper.decode_window = dw

        def transcribe(self, idxs):
            """one generate call over the audios idxs (several: padded features + attention_mask, the reference's
            batched long-form); each audio's transcript = its segments' tokens.  --mode e2e: each 30 s clip through
            CBWhisper.forward (short-form: no timestamps, 5 beams, the keyword prompt; cb_whisper.py:151-187), its
            transcript = the decoded text"""
            with torch.cuda.device(dev), torch.cuda.stream(self.stream):
                feats = [log_mel_long(audios[i], n_mel) for i in idxs]
                if e2e:
                    for f, i in zip(feats, idxs):
                        self.decoded.clear()
                        self.cb.forward(f[None], torch.ones((1, f.shape[-1]), dtype=torch.long, device=dev))
                        gen = [t for d in self.decoded for t in d]
                        self.stats["tokens"] += len(gen)
                        self.stats["transcript_tokens"] += len(self.last_ids)
                        self.digests[i] = hashlib.sha1(np.asarray(gen, dtype=np.int64).tobytes()).hexdigest()[:16]
                        self.tokens[i] = gen
                    self.stream.synchronize()
                    return None
                if len(feats) == 1:
                    res = self.whisper.generate(input_features=feats[0][None], **self.gen_kw)
                else:
                    T = max(f.shape[-1] for f in feats)
                    x = torch.zeros((len(feats), n_mel, T), dtype=torch.float32, device=dev)
                    mask = torch.zeros((len(feats), T), dtype=torch.long, device=dev)
                    for b, f in enumerate(feats):
                        x[b, :, :f.shape[-1]] = f
                        mask[b, :f.shape[-1]] = 1
                    res = self.whisper.generate(input_features=x, attention_mask=mask, **self.gen_kw)
                for b, i in enumerate(idxs):
                    toks = [int(t) for s_ in res["segments"][b] for t in s_["tokens"].tolist()]
                    self.stats["tokens"] += len(toks)
                    self.digests[i] = hashlib.sha1(np.asarray(toks, dtype=np.int64).tobytes()).hexdigest()[:16]
                    self.tokens[i] = toks
                self.stream.synchronize()
            return res

        def run(self, calls):
            try:
                for idxs in calls:
                    self.transcribe(idxs)
            except BaseException as e:   # re-raised by the main thread
                self.error = e

    op_shift = [None]   # the realistic point's class-1 bias shift (computed once, every lane the same network)
    fp8_cal = [None]
    wsd = {"model.encoder." + k: v for k, v in synth.synth_whisper_encoder_state_dict(args.model, seed=0).items()}
    wsd.update({"model.decoder." + k: v for k, v in synth.synth_whisper_decoder_state_dict(args.model, seed=0).items()})
    lanes = [Lane(j) for j in range(A)]
    del wsd
    n = int(args.audio_seconds * 16000)
    audios = []   # audio u = (i * A + j) * G + g (step i, lane j, g-th of its generate call): seed 100000 * rank +
    # 1000 * u; a generate call's audios differ in length by 17 s steps; warm-up audios cut to <= 60 s
    for i in range(args.warmup + args.steps):
        for j in range(A):
            for g in range(G):
                u = (i * A + j) * G + g
                ni = max(16000, n - int(g * args.batch_length_step * 16000))
                ni = ni if i >= args.warmup else min(ni, 60 * 16000)
                a = np.concatenate([synth.synth_clip(100000 * rank + 1000 * u + q) for q in range(ni // 480000 + 1)])[:ni]
                audios.append(torch.from_numpy(a).to(dev))

    def run_lanes(first, count):
        """lane j transcribes audios (i * A + j) for i in [first, first + count), all lanes concurrently"""
        def calls(j):
            return [[(i * A + j) * G + g for g in range(G)] for i in range(first, first + count)]
        if A == 1:
            lanes[0].run(calls(0))
        else:
            th = [threading.Thread(target=ln.run, args=(calls(j),)) for j, ln in enumerate(lanes)]
            for t in th:
                t.start()
            for t in th:
                t.join()
        for ln in lanes:
            if ln.error is not None:
                raise ln.error

    log(f"[bench] longform setup {time.time() - t_setup:.1f} s: {args.model} + LEF/resnet-50 vs {K} keywords, "
        f"{args.audio_seconds:.0f} s audio per lane per step, {A} lane(s), {args.beams} beams")
    run_lanes(0, args.warmup)
    torch.cuda.synchronize()
    for ln in lanes:
        for k in ln.stats:
            ln.stats[k] = 0
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_lanes(args.warmup, args.steps)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    stats = {k: sum(ln.stats[k] for ln in lanes) for k in lanes[0].stats}
    timed = range(args.warmup * A * G, (args.warmup + args.steps) * A * G)
    digests = {i: d for ln in lanes for i, d in ln.digests.items() if i in timed}
    elapsed, rank_elapsed = rank_times(dist, elapsed, dev)
    if dist is not None:
        tot = torch.tensor([stats["windows"], stats["tokens"]], dtype=torch.float64, device=dev)
        dist.all_reduce(tot)
        stats["windows"], stats["tokens"] = int(tot[0]), int(tot[1])
    audio_s = sum(len(audios[u]) for u in timed) / 16000 * world
    if args.dump_outputs and rank == 0:   # the transcripts of the last timed step's audios (this rank's), as token ids
        last = range((args.warmup + args.steps - 1) * A * G, (args.warmup + args.steps) * A * G)
        dump_outputs(args.dump_outputs, {f"tokens_audio{i}": np.asarray(t, dtype=np.int64)
                                         for ln in lanes for i, t in ln.tokens.items() if i in last})
    if rank == 0 and e2e:
        clips = len(timed) * world
        rec = {"metric": f"utterances/sec end to end (30 s clips: {args.model} encoder hs -> CB-Whisper LEF spotting vs "
                         f"{K} keywords -> keyword prompt -> PBAWhisper {args.beams}-beam decode)",
               "value": round(clips / elapsed, 4), "unit": "utterances/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 1), "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": "e4m3+bf16" if args.fp8_first else "bf16",
               "data": "synthetic (seeded clips, seeded random weights, synthetic keyword hs and tokenizer)",
               "config": {"workload": f"CBWhisper.forward (cb_whisper.py:151-187): short-form generate, {args.beams} "
                                      f"beams, keyword prompt from LEF spotting vs {K} keywords (exact band "
                                      f"{args.exact_band})",
                          "parallelism": f"clip-parallel x{world}, {A} clip(s) in flight per GPU",
                          "operating_point": {"name": args.operating_point,
                                              **({"class1_bias_shift": round(-op_shift[0], 4)} if op_shift[0] else {})},
                          "spotting_first_tier": "fp8 (e4m3 MFMA)" if args.fp8_first else "bf16",
                          "max_new_tokens": args.max_new_tokens},
               "rank_elapsed_s": [round(x, 4) for x in rank_elapsed],
               "ms_per_clip": round(elapsed * world * A / max(1, clips) * 1e3, 1),
               "tokens_generated": stats["tokens"],
               "transcript_tokens": stats["transcript_tokens"],
               "note": "tokens_generated / transcript_digests: the decoded tokens after the forced prefix; the returned "
                       "transcript drops the first len(keyword prompt) tokens (pba_whisper.py:338 slices by the "
                       "untruncated prompt, which the decoder sees cut to its last 225 tokens)",
               "spotted_keywords_per_clip": round(stats["spotted"] / max(1, stats["windows"]), 1),
               "spotting_ms_per_clip": round(stats["spot_s"] / max(1, stats["windows"]) * 1e3, 1),
               "transcript_digests": {str(i): digests[i] for i in sorted(digests)}}
        print(json.dumps(rec), flush=True)
    elif rank == 0:
        rec = {"metric": f"audio seconds/sec (long-form PBAWhisper-{args.model} + CB-Whisper LEF spotting vs {K} "
                         f"keywords, clip-parallel)",
               "value": round(audio_s / elapsed, 3), "unit": "audio s/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 1), "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": "e4m3+bf16" if args.fp8_first else "bf16",
               "data": "synthetic (seeded audio, seeded random weights, synthetic keyword hs and tokenizer)",
               "config": {"workload": f"PBAWhisper.generate long-form ({args.audio_seconds:.0f} s per audio, "
                                      f"{args.beams} beams, timestamps, condition_on_prev_tokens) + CB-Whisper LEF "
                                      f"spotting per 30 s window vs {K} keywords (exact band {args.exact_band})",
                          "parallelism": f"clip-parallel x{world} (independent audios), {A} audio(s) in flight per GPU",
                          "audios_in_flight": A, "lane_priority": bool(args.lane_priority and A > 1),
                          "generate_batch": G,
                          "operating_point": {"name": args.operating_point,
                                              **({"class1_bias_shift": round(-op_shift[0], 4)} if op_shift[0] else {})},
                          "spotting_first_tier": "fp8 (e4m3 MFMA)" if args.fp8_first else "bf16",
                          "fp8_first": fp8_cal[0],
                          "max_new_tokens": args.max_new_tokens},
               "rank_elapsed_s": [round(x, 4) for x in rank_elapsed],
               "windows_per_s": round(stats["windows"] / elapsed, 3), "windows": stats["windows"],
               "tokens_generated": stats["tokens"],
               "ms_per_window": round(elapsed * world * A / max(1, stats["windows"]) * 1e3, 1),
               "spotted_keywords_per_window": round(stats["spotted"] / max(1, stats["windows"]), 1),
               "spotting_ms_per_window": round(stats["spot_s"] / max(1, stats["windows"]) * 1e3, 1),
               "transcript_digests": {str(i): digests[i] for i in sorted(digests)}}
        print(json.dumps(rec), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def run_api(args):
    """--mode api: the drop-in API path (efficient_kws.model.KWSModel.test_step, the call run_efficient_kws.py test
    makes per utterance; reference model.py:748-802) on the bench's workload.  One step = one synthetic 30 s clip:
    mel -> large-v3 encoder -> hs[19..21] (the utterance features the dataset would hand over) -> test_step with
    the bench's 10 000 seeded keywords as the dataset groups them (raw hs [50, 3, 150, D] fp32 + masks per group of
    hotwords_per_group = 50, eval-LEF-comp-acl.yaml:121; device-resident, the same tensor objects every step as a
    cached dataset hands them).  KWSModel keeps the groups' projections across calls and scores all groups in one
    chunked call; exact_band "auto" (calibrated at the first call, a warm-up step).  No pipelining: test_step is
    synchronous.  The spotted digest of the last timed clip equals the engine path's (both exact)."""
    from cbw import synth
    from cbw.whisper import EncoderEngine, default_layer_ids, log_mel
    from efficient_kws.model import KWSModel
    if int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--mode api is the one-GPU drop-in path (--gpus 1)")
    dev = _rank_device(int(os.environ.get("LOCAL_RANK", "0")))
    t_setup = time.time()
    enc_cfg = synth.WHISPER_CONFIGS[args.model]
    n_mel, D, n_layers, _, _ = enc_cfg
    enc = EncoderEngine(enc_cfg, synth.synth_whisper_encoder_state_dict(args.model, seed=0), dev)
    ids = default_layer_ids(n_layers)
    kws_hp = kws_hparams(args.variant, D, args.threshold, features_size=[150, 1500])
    model = KWSModel(**kws_hp)
    model.load_state_dict(synth.synth_kws_state_dict(seed=0, **kws_hp))
    model.engine()
    K = args.keywords
    groups, gmasks = [], []
    for _, x, m in keyword_hs(K, D, dev):
        for a in range(0, x.shape[0], 50):
            groups.append(x[a:a + 50].contiguous())
            gmasks.append(m[a:a + 50].contiguous())
    ghost = [torch.ones(g.shape[0], device=dev) for g in groups]
    clips = [torch.from_numpy(synth.synth_clip(i)).to(dev) for i in range(args.warmup + args.steps)]
    utt_mask = torch.ones((3, 1500), device=dev)
    log(f"[bench] api setup {time.time() - t_setup:.1f} s: {len(groups)} groups of 50 raw keyword hs")
    last = [None]

    def step(i):
        _, mel_pk = log_mel(clips[i], n_mel, packed=True)
        hs = enc.hidden_states(mel_pk, ids, normalize=True)
        out = model.test_step({"kwd": groups, "kwd_mask": gmasks, "utt": hs[0], "utt_mask": utt_mask,
                               "hotword_mask": ghost}, i)
        last[0] = out["preds"]

    t_w = time.perf_counter()
    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    warm_s = time.perf_counter() - t_w
    model.test_step_outputs = []
    t0 = time.perf_counter()
    for i in range(args.warmup, args.warmup + args.steps):
        step(i)
        model.test_step_outputs = []
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    spotted = torch.nonzero(last[0] >= args.threshold).flatten().to(torch.int32)
    digest = hashlib.sha1(spotted.cpu().numpy().tobytes()).hexdigest()[:16]
    if args.dump_outputs:   # what test_step returned for the last timed clip
        dump_outputs(args.dump_outputs, {"preds": last[0], "spotted_indices": spotted})
    rec = {"metric": "utterances/sec (30 s clips) via efficient_kws.model.KWSModel.test_step (drop-in API), "
                     "Whisper-large-v3 LEF 10k kw",
           "value": round(args.steps / elapsed, 4), "unit": "utterances/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
           "data": "synthetic (seeded 30 s clips, seeded random weights, 10k synthetic keyword hs in groups of 50)",
           "config": {"workload": f"whisper-{args.model} encoder + KWSModel.test_step (LEF, resnet-50) vs {K} "
                                  f"keywords in {len(groups)} groups of 50, one 30 s clip per step",
                      "keywords": K, "kwd_cache": model.kwd_cache},
           "pairs_per_s": round(args.steps / elapsed * K, 1), "warmup_s": round(warm_s, 2),
           "band_calibration": model.band_calibration, "exact_band": model.exact_band,
           "spotted_last_clip": int(spotted.numel()), "spotted_digest": digest}
    print(json.dumps(rec), flush=True)
