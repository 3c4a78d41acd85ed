"""efficient_kws.model.KWSModel — MI355X drop-in for src/efficient_kws/model.py:18-952.

Keeps the reference constructor (same hyper-parameters, unused ones inert as in
the reference), ``forward(kwd_features, utt_features, labels, kwd_mask,
utt_mask) -> KWSOutput`` (model.py:129-208), the ``test_step`` decision
(model.py:748-802), ``load_from_checkpoint`` for Lightning ``.ckpt`` files
(with the legacy key remap of ``on_load_checkpoint``, model.py:931-952) and
``state_dict``/``load_state_dict`` with the reference parameter names.

Everything numeric runs in libcbw on the GPU (cbw.kws.KwsEngine); there is no
CPU path.  Deviations from the reference, all documented in DESIGN.md:
  * LEF masks are max-pooled like the features (the reference crashes at
    model.py:186-191); masks already at the pooled length are
    used as given;
  * learn_features=True with proj_mlp=False (train-L.yaml) builds the L
    classifier instead of raising AttributeError;
  * training (training_step/optimizers/metrics) is out of scope.
"""
from __future__ import annotations

import re
import warnings
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from cbw.kws import KwsEngine, VARIANT_L, VARIANT_LEF, spot, variant_of
from cbw.metrics import binary_precision_recall_curve, evaluate_with_conf_int, operating_point
from cbw.synth import kws_param_shapes

from .utils import KWSOutput

_DEFAULTS = dict(
    num_domains=72, sampling="utterance-examples", resample_every_epoch=True, kw_type="tts", kw_p=0.5,
    features_size=(160, 1000), learn_features=False, load_embeddings=True, n_layers=12,
    pad_long_before_resize=False, kws_whisper_ckpt="openai/whisper-large-v2", embedding_dim=1024,
    features_with_conv=False, features_with_attn=False, frames_conv=False, proj_mlp=False, proj_mlp_units=64,
    batch_size=1, accumulate_grad_batches=1, learning_rate_sru=1e-4, learning_rate=1e-4, warmup_proportion=0.0,
    max_epochs=200, features_lr=1e-4, classifier_lr=1e-4, lr_step=40, weight_decay=0.0, beta_1=0.9, beta_2=0.99,
    condensed_dimension="embeddings", resnet_version="resnet-50", compile=False, threshold=0.5,
    task_type="keyword-spotting", diag_size=5, alpha_max_epochs=10, min_alpha=0.1,
)


EXACT_BAND = 0.03   # the band before the first auto-calibration (and for the per-group forward)
X3_BAND = 1e-4     # the compensated tier's band into fp32 (its max |p - p_fp32| measured 2.8e-5)


class KWSModel:
    def __init__(self, **kwargs):
        hp = dict(_DEFAULTS)
        hp.update(kwargs)
        self.hparams = SimpleNamespace(**hp)
        print("threshold: ", self.hparams.threshold)
        self._hp = hp
        self.variant = variant_of(hp)
        self._sd: Dict[str, torch.Tensor] = {}
        self._engine: Optional[KwsEngine] = None
        self.training = False
        self.test_step_outputs = []
        # fp32 re-scoring of the pairs whose bf16 probability lies within exact_band of the threshold
        # (0 = off, 1.0 = every pair): the decision then follows the reference's fp32 evaluation
        # (eval-*-comp-*.yaml:8 precision 32-true).  "auto" (default): calibrated on these weights at the first
        # scored utterance (_calibrate_band: bias correction of the bf16 network, then the band = 2x the largest
        # bf16-vs-fp32 probability error over held-out pairs); a number is used as given.  Without the fp32
        # network (n_layers > 4) the band is off and decisions are bf16's.
        band = kwargs.get("exact_band", "auto")
        self._band_auto = isinstance(band, str)
        if self._band_auto and band != "auto":
            raise ValueError(f"exact_band must be a number or 'auto', got {band!r}")
        self.exact_band = EXACT_BAND if self._band_auto else float(band)
        self.band_calibration: Optional[dict] = None
        # keyword-database cache of test_step (projections of the whole database, bf16 + fp32): "content" (default)
        # re-projects unless every group tensor has the shape, dtype and full-content 64-bit checksum it had
        # (cbw_checksum on the device: ~23 GB / ~5 TB/s for 10k raw keyword groups at D 1280), whatever object holds
        # it; "identity" trusts the same tensor objects at the same torch version counters (writes through other
        # paths go unseen); "off" re-projects every call, as the reference does
        self.kwd_cache = kwargs.get("kwd_cache", "content")
        if self.kwd_cache not in ("content", "identity", "off"):
            raise ValueError(f"kwd_cache must be 'content', 'identity' or 'off', got {self.kwd_cache!r}")
        self._db = None

    # ------------------------------------------------------------------ parameters
    def _param_shapes(self):
        return kws_param_shapes(self.hparams.n_layers, self.hparams.embedding_dim,
                                self.variant != VARIANT_L, self.variant != VARIANT_L,
                                self.variant == VARIANT_LEF, self.hparams.proj_mlp_units,
                                self.hparams.resnet_version)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(self._sd)

    def load_state_dict(self, state_dict: Dict[str, object], strict: bool = True):
        expected = {n: s for n, s, _ in self._param_shapes()}
        sd = {k: (v.detach().cpu() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v)))
              for k, v in state_dict.items()}
        if strict:
            missing = sorted(set(expected) - set(sd))
            unexpected = sorted(set(sd) - set(expected))
            if missing or unexpected:
                raise RuntimeError(f"Error(s) in loading state_dict for KWSModel: missing {missing[:5]}, "
                                   f"unexpected {unexpected[:5]}")
        for k, shape in expected.items():
            if k in sd and tuple(sd[k].shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(shape)}")
        self._sd = {k: v for k, v in sd.items() if k in expected}
        self._engine = None
        return SimpleNamespace(missing_keys=[], unexpected_keys=[])

    @staticmethod
    def _remap_legacy(state_dict: Dict[str, object]) -> Dict[str, object]:
        """on_load_checkpoint (model.py:931-952): early checkpoints keep `model.resnet.*`."""
        resnet_regex = re.compile("resnet.")
        fe_regex = re.compile("(model.embedder|model.encoder)")
        if not any(resnet_regex.search(k) for k in state_dict):
            return state_dict
        out = {}
        for k, v in state_dict.items():
            nk = resnet_regex.sub("", k)
            if fe_regex.search(nk):
                nk = nk[:6] + "feature_extractor." + nk[6:]
            out[nk] = v
        return out

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path: str, map_location=None, **overrides) -> "KWSModel":
        """Lightning .ckpt: {'state_dict', 'hyper_parameters', ...}; loaded with weights_only=True."""
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        hp = dict(ckpt.get("hyper_parameters", {}))
        hp.update(overrides)
        model = cls(**hp)
        model.load_state_dict(cls._remap_legacy(ckpt["state_dict"]), strict=True)
        return model

    def eval(self):
        self.training = False
        return self

    def to(self, *args, **kwargs):
        return self

    def engine(self) -> KwsEngine:
        if self._engine is None:
            if not self._sd:
                raise RuntimeError("KWSModel has no parameters: call load_state_dict / load_from_checkpoint")
            self._engine = KwsEngine(self._hp, self._sd)
            self._db = None
            self.band_calibration = None
            if not self._engine.has_fp32 and self.exact_band > 0:
                if not self._band_auto:
                    warnings.warn(f"exact_band={self.exact_band} needs the fp32 re-scoring network, which exists for "
                                  f"n_layers <= 4 only (n_layers={self.hparams.n_layers}): decisions are bf16's")
                self.exact_band = 0.0
        return self._engine

    def _band_active(self) -> float:
        return self.exact_band if (self.exact_band > 0 and self.engine().has_fp32) else 0.0

    def _calibrate_band(self, eng, pu, pum, pu32, pk, pkm, pk32) -> None:
        """exact_band="auto" (ADVICE r02): measure the band on these weights (calibrate_band below)."""
        self.band_calibration = calibrate_band(eng, pu, pum, pu32, pk, pkm, pk32)
        self.exact_band = self.band_calibration["band"]

    # ------------------------------------------------------------------ forward
    def forward(self, kwd_features: torch.Tensor, utt_features: torch.Tensor, labels: torch.Tensor = None,
                kwd_mask: Optional[torch.Tensor] = None, utt_mask: Optional[torch.Tensor] = None,
                return_features: bool = True) -> KWSOutput:
        """model.py:129-208.  kwd_features [K, L, Tk, D], utt_features [1 or K, L, Tu, D],
        masks [K|1, L, T] (None = all ones)."""
        eng = self.engine()
        dev = eng.device
        kwd = kwd_features.to(dev, torch.float32)
        utt = utt_features.to(dev, torch.float32)
        K, L, Tk, _ = kwd.shape
        Bu, _, Tu, _ = utt.shape
        if Bu not in (1, K):
            raise ValueError(f"utt batch must be 1 or n_keywords, got {Bu}")
        km = torch.ones((K, L, Tk), device=dev) if kwd_mask is None else kwd_mask.to(dev, torch.float32)
        um = torch.ones((Bu, L, Tu), device=dev) if utt_mask is None else utt_mask.to(dev, torch.float32)
        pk, pkm = self._project(eng, kwd, km)
        pu, pum = self._project(eng, utt, um)
        if Bu == 1:
            out = eng.score(pu[0], pum[0], pk, pkm, features=return_features)
            logits, feats = out if return_features else (out, None)
            if self._band_active() > 0 and K > 0:
                if self._band_auto and self.band_calibration is None:
                    pk32, _ = self._project(eng, kwd, km, f32=True)
                    pu32, _ = self._project(eng, utt, um, f32=True)
                    self._calibrate_band(eng, pu[0], pum[0], pu32[0], pk, pkm, pk32)
                    if self.band_calibration["bias_calibration_pairs"]:
                        logits = eng.score(pu[0], pum[0], pk, pkm)   # the bias-corrected bf16 network
                logits = self._rescore_band(eng, kwd, km, utt, um, pkm, pum, logits)
        else:  # training-style batches: one utterance per keyword
            pair = torch.arange(K, dtype=torch.int32, device=dev)
            if self._band_active() > 0 and K > 0:
                # the exact decisions of the Bu == 1 branch for the identity pair list: every pair in bf16, the
                # band's pairs in fp32 (no compensated tier: the logits equal the K single-pair forwards')
                pk32, _ = self._project(eng, kwd, km, f32=True)
                pu32, _ = self._project(eng, utt, um, f32=True)
                if self._band_auto and self.band_calibration is None:   # scored below by the corrected network
                    self._calibrate_band(eng, pu[0], pum[0], pu32[0], pk, pkm, pk32)
                out = eng.score_pairs_exact(pu, pum, pk, pkm, pu32, pk32, pair, pair, self.hparams.threshold,
                                            self.exact_band, trusted=True, features=return_features)
                logits, feats = (out[0], out[2]) if return_features else (out[0], None)
            else:
                out = eng.score_pairs(pu, pum, pk, pkm, pair, pair, features=return_features, trusted=True)
                logits, feats = out if return_features else (out, None)
        loss = None
        if labels is not None:
            loss = torch.nn.functional.cross_entropy(logits, labels.to(dev).view(-1))
        return KWSOutput(loss=loss, logits=logits, features=feats, logits_alt=None,
                         loss_alt={"loss_diag": None, "loss_resnet": loss})

    @staticmethod
    def _project(eng, x, m, f32: bool = False):
        """Projection of features x [B, L, T, D] with 0/1 masks m [B, L, T] (or masks already at the LEF-pooled
        length, used as given) -> (projected [B, L, T', E] bf16 or f32, pooled masks [B, L, T'])."""
        T = x.shape[2]
        fn = eng.project_f32 if f32 else eng.project
        p, pm = fn(x, m if m.shape[-1] == T else torch.ones(x.shape[:3], device=x.device))
        if m.shape[-1] == p.shape[2] and m.shape[-1] != T:
            pm = m.contiguous()
        return p, pm

    __call__ = forward

    def _rescore_band(self, eng, kwd, km, utt, um, pkm, pum, logits):
        """Pairs with |softmax(logits)[:, 1] - threshold| <= exact_band re-run in fp32 (cbw_kws_band selects
        them on the GPU; only the selected keywords are projected in fp32, then cbw_kws_rescore)."""
        sel, n = eng.band(logits, self.hparams.threshold, self.exact_band)
        if n == 0:
            return logits
        Tk, Tu = kwd.shape[2], utt.shape[2]
        s = sel.long()
        ks, kms = kwd[s], km[s]
        k32, _ = eng.project_f32(ks, kms if kms.shape[-1] == Tk else torch.ones_like(ks[..., 0]))
        u32, _ = eng.project_f32(utt, um if um.shape[-1] == Tu else torch.ones_like(utt[..., 0]))
        sub = logits[s].contiguous()
        eng.rescore(u32[0], pum[0], k32, pkm[s].contiguous(), sub,
                    torch.arange(n, dtype=torch.int32, device=logits.device), trusted=True)
        logits = logits.clone()
        logits[s] = sub
        return logits

    # ------------------------------------------------------------------ evaluation
    def test_step(self, batch: dict, batch_idx: int = 0, dataloader_idx: int = 0) -> dict:
        """model.py:748-802: prob = softmax(logits)[:, 1] * hotword (ghost) mask for every keyword of every group.
        The reference calls forward once per group of ``hotwords_per_group`` keywords and re-projects the groups on
        every utterance; here the projections of the whole keyword database (bf16, and fp32 for the exact band) are
        cached across calls (``kwd_cache``) and all groups are scored in one chunked call -- the per-pair results
        are those of the per-group calls (the scoring is chunk-invariant, tests/test_gpu_kws.py)."""
        kwd_groups = [torch.stack(list(g)) if isinstance(g, (list, tuple)) else g for g in batch["kwd"]]
        kmask_groups = [torch.stack(list(g)) if isinstance(g, (list, tuple)) else g for g in batch["kwd_mask"]]
        eng = self.engine()
        dev = eng.device
        pk, pkm, pk32 = self._keyword_db(eng, kwd_groups, kmask_groups)
        utt = batch["utt"].unsqueeze(0).to(dev, torch.float32)
        um = batch["utt_mask"].unsqueeze(0).to(dev, torch.float32)
        pu, pum = self._project(eng, utt, um)
        hm = batch.get("hotword_mask", None)
        ghost = None
        if hm is not None:
            ghost = torch.cat([torch.as_tensor(hm[i]).reshape(-1).to(dev, torch.float32)
                               for i in range(len(kwd_groups))], 0)
        thr = self.hparams.threshold
        K = pk.shape[0]
        chunk = max(1, min(K, 1112))
        if self._band_active() > 0 and K > 0:
            pu32, _ = self._project(eng, utt, um, f32=True)
            if self._band_auto and self.band_calibration is None:
                self._calibrate_band(eng, pu[0], pum[0], pu32[0], pk, pkm, pk32)
            logits, _ = eng.score_exact(pu[0], pum[0], pk, pkm, pu32[0], pk32, thr, self._band_active(), ghost=ghost,
                                        chunk=chunk, band_x3=X3_BAND if self._band_active() > X3_BAND else None)
        else:
            logits = eng.score(pu[0], pum[0], pk, pkm, chunk=chunk)
        preds, _ = spot(logits, ghost, thr)
        targets = torch.cat(list(batch["hotword_labels"]), 0) if "hotword_labels" in batch else None
        out = {"preds": preds, "targets": targets, "speaker": batch.get("speaker")}
        self.test_step_outputs.append(out)
        return out

    @staticmethod
    def content_key(tensors, device=None) -> tuple:
        """(shape, dtype, 64-bit full-content checksum) of every tensor: cbw_checksum over the tensor's bytes on the
        device, one host sync for all of them.  Tensors that are elsewhere (a DataLoader's CPU batch), not contiguous
        or not 16-byte aligned go through ONE reused device staging buffer, one at a time (stream order keeps each
        copy behind the previous checksum), so the device holds at most the largest of them, not all."""
        from cbw import _lib
        lib = _lib.load()
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        ws = torch.empty(int(lib.cbw_checksum_workspace_bytes()), dtype=torch.uint8, device=dev)
        out = torch.empty(max(1, len(tensors)), dtype=torch.int64, device=dev)
        staged = [t.detach() for t in tensors]
        direct = [x.device == dev and x.is_contiguous() and x.data_ptr() % 16 == 0 for x in staged]
        nstage = max([x.numel() * x.element_size() for x, d in zip(staged, direct) if not d] or [0])
        stage = torch.empty(nstage, dtype=torch.uint8, device=dev) if nstage else None
        with torch.cuda.device(dev):
            for i, (x, d) in enumerate(zip(staged, direct)):
                nb = x.numel() * x.element_size()
                if d:
                    ptr = x.data_ptr()
                else:
                    if nb:
                        stage[:nb].copy_(x.contiguous().reshape(-1).view(torch.uint8))
                    ptr = stage.data_ptr() if stage is not None else ws.data_ptr()
                _lib.check(lib.cbw_checksum(ptr, nb, out[i:i + 1].data_ptr(), ws.data_ptr(), ws.numel(),
                                            _lib.stream_handle()), "cbw_checksum")
            sums = out[:len(tensors)].cpu().tolist()
        return tuple((tuple(t.shape), str(t.dtype), c) for t, c in zip(tensors, sums))

    def _keyword_db(self, eng, kwd_groups, kmask_groups):
        """Projected keyword database (bf16 [K, L, T', E], pooled masks, fp32 [K, L, T', E] when the exact band is
        on) of the concatenated groups; cached: kwd_cache="content" -- a hit when every tensor has the shape,
        dtype and content checksum it had; "identity" -- when the same tensor objects come back at the same
        version counters."""
        tensors = list(kwd_groups) + list(kmask_groups)
        need32 = self._band_active() > 0
        c = self._db
        key = self.content_key(tensors, eng.device) if self.kwd_cache == "content" else None
        if c is not None and self.kwd_cache != "off" and (c["proj"][2] is not None or not need32):
            if self.kwd_cache == "content" and c["key"] == key:
                return c["proj"]
            if self.kwd_cache == "identity" and len(c["refs"]) == len(tensors) and \
                    all(a is b and a._version == v for a, b, v in zip(c["refs"], tensors, c["versions"])):
                return c["proj"]
        dev = eng.device
        pk, pkm, pk32 = [], [], []
        for g, m in zip(kwd_groups, kmask_groups):
            x = g.to(dev, torch.float32)
            mm = m.to(dev, torch.float32)
            p, pm = self._project(eng, x, mm)
            pk.append(p)
            pkm.append(pm)
            if need32:
                pk32.append(self._project(eng, x, mm, f32=True)[0])
        proj = (torch.cat(pk, 0), torch.cat(pkm, 0), torch.cat(pk32, 0) if need32 else None)
        self._db = None if self.kwd_cache == "off" else {
            "refs": tensors if self.kwd_cache == "identity" else None,
            "versions": [t._version for t in tensors], "proj": proj, "key": key}
        return proj

    def on_test_epoch_start(self):
        self.test_step_outputs = []

    def on_test_epoch_end(self, num_bootstraps: int = 1000, alpha: float = 5) -> Dict[str, float]:
        """model.py:804-929: precision / recall / F1 at hparams.threshold on the binary PR curve of
        every (utterance, keyword) probability, with speaker-conditioned bootstrap CIs.  Returns the
        metrics the reference prints (plus the curve under "pr_data"); empties the step outputs."""
        outs = self.test_step_outputs
        samples = torch.cat([o["preds"].detach().float().cpu() for o in outs]).numpy()
        labels = torch.cat([o["targets"].detach().cpu() for o in outs]).numpy()
        speakers = [o["speaker"] for o in outs for _ in range(len(o["preds"]))]
        speaker2id = {s: i for i, s in enumerate(dict.fromkeys(speakers))}
        conditions = [speaker2id[s] for s in speakers]
        thr = self.hparams.threshold

        def at_threshold(which):
            def f(lab, smp, smp2=None):
                return operating_point(*binary_precision_recall_curve(smp, lab), thr)[which]
            return f

        metrics = {}
        for which, name in enumerate(("Precision", "Recall", "F1")):
            c, (lo, hi) = evaluate_with_conf_int(samples, at_threshold(which), labels, conditions,
                                                 num_bootstraps=num_bootstraps, alpha=alpha)
            metrics[name], metrics[name + "_LB"], metrics[name + "_UB"] = c, lo, hi
        p, r, t = binary_precision_recall_curve(samples, labels)
        metrics["pr_data"] = {"precision": p.tolist(), "recall": r.tolist(), "thresholds": t.tolist()}
        self.test_step_outputs = []
        return metrics

    def spot(self, logits: torch.Tensor, ghost_mask: Optional[torch.Tensor] = None,
             threshold: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Operating-point decision of model.py:804-813: prob >= threshold."""
        thr = self.hparams.threshold if threshold is None else threshold
        return spot(logits, ghost_mask, thr)


def calibrate_band(eng, pu, pum, pu32, pk, pkm, pk32) -> dict:
    """The exact-decision band measured on the engine's own weights instead of a number measured on the synthetic
    ones.  With >= 1024 keywords, the bf16 network is first bias-corrected on the first 512 pairs
    (KwsEngine.calibrate_bias: conv-input means of the fp32 network, then the mean logit offset; the compensated /
    fp32 tiers keep the reference biases); the band is then 2x the largest |p_bf16 - p_fp32| over up to 1024
    held-out pairs of this utterance (every pair when there are fewer), floored at 0.005 (at EXACT_BAND with
    fewer than 256 held-out pairs).  An empirical bound like bench.py's.  pu / pum / pu32: the
    projected utterance (bf16, pooled mask, fp32); pk / pkm / pk32: the projected keyword database.
    Returns {"bias_calibration_pairs", "held_out_pairs", "max_bf16_err", "band"}."""
    K = pk.shape[0]
    n_cal = 512 if K >= 1024 else 0
    if n_cal:
        eng.calibrate_bias(pu32, pum, pk32[:n_cal].contiguous(), pkm[:n_cal].contiguous(), utt=pu,
                           kwd=pk[:n_cal].contiguous())
    hold = slice(n_cal, min(K, n_cal + 1024))
    kb, km, k32 = pk[hold].contiguous(), pkm[hold].contiguous(), pk32[hold].contiguous()
    l16 = eng.score(pu, pum, kb, km)
    l32 = torch.empty_like(l16)
    eng.rescore(pu32, pum, k32, km, l32, torch.arange(kb.shape[0], dtype=torch.int32, device=l16.device),
                trusted=True)
    err = float((torch.softmax(l16.double(), -1)[:, 1] - torch.softmax(l32.double(), -1)[:, 1]).abs().max())
    floor = 0.005 if kb.shape[0] >= 256 else EXACT_BAND   # a small sample cannot narrow the default band
    return {"bias_calibration_pairs": n_cal, "held_out_pairs": int(kb.shape[0]), "max_bf16_err": err,
            "band": float(min(0.5, max(floor, 2.0 * err)))}
