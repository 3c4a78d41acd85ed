"""KWS classifier engine over libcbw (LE/LEF projection, similarity maps, ResNet, decision).

Host-side owner of one ``cbw_kws`` handle: loads a reference-format state dict
(``KWSModel.state_dict()`` names, see cbw.synth.kws_param_shapes), lets the
native runtime fold BatchNorm and upload bf16 weights, and runs the hot path on
torch-owned device buffers.  Reference semantics per call are cited in
include/cbw.h.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib

VARIANT_L, VARIANT_LE, VARIANT_LEF = 0, 1, 2
RESNET_DEPTH = {"resnet-50": 50, "resnet-34": 34, "resnet-18": 18}


def variant_of(hp: dict) -> int:
    """efficient_kws/model.py:71-124.  learn_features=False -> L (Resnet on raw-hs
    similarities).  learn_features & proj_mlp -> LE (+frames_conv -> LEF).
    learn_features & !proj_mlp builds no classifier in the reference
    (AttributeError); the build treats it as L."""
    if hp.get("learn_features", False) and hp.get("proj_mlp", False):
        return VARIANT_LEF if hp.get("frames_conv", False) else VARIANT_LE
    return VARIANT_L


def lef_frames(T: int) -> int:
    """MaxPool1d(3, 2, 1) output length (model.py:120-122)."""
    return (T - 1) // 2 + 1


class KwsEngine:
    def __init__(self, hp: dict, state_dict: Dict[str, object], device: Optional[torch.device] = None,
                 classifier_only: bool = False):
        """``classifier_only``: a handle for the ResNet alone (efficient_kws/resnet.py:7-58 as its own module):
        no projector parameters, ``hp['resnet_version']`` honoured; only ``classify`` is usable."""
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.hp = dict(hp)
        self.variant = VARIANT_L if classifier_only else variant_of(hp)
        self.n_layers = int(hp.get("n_layers", 12))
        self.D = int(hp.get("embedding_dim", 1024))
        self.U = int(hp.get("proj_mlp_units", 64))
        version = (hp.get("resnet_version", "resnet-50") if self.variant != VARIANT_L or classifier_only
                   else "resnet-50")
        if version not in RESNET_DEPTH:
            raise ValueError(f"unsupported resnet_version {version}")
        cfg = _lib.KwsConfig(self.n_layers, self.D, self.variant, self.U, RESNET_DEPTH[version])
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cbw_kws_create(ctypes.byref(cfg), ctypes.byref(h)), "cbw_kws_create")
            self.h = h
            for name, v in state_dict.items():
                if name.endswith("num_batches_tracked"):
                    continue
                a = np.ascontiguousarray(v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v),
                                         dtype=np.float32)
                _lib.check(self.lib.cbw_kws_set_param(self.h, name.encode(), a.ctypes.data, a.size),
                           f"cbw_kws_set_param({name})")
            _lib.check(self.lib.cbw_kws_finalize(self.h), "cbw_kws_finalize")
        self._ws = _lib.Workspace()
        self._ws_rescore = _lib.Workspace()   # the re-scoring tiers' own scratch: they may overlap scoring
        self._pws = _lib.Workspace()
        self._exact_built = False

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            try:
                self.lib.cbw_kws_destroy(h)
            except Exception:
                pass

    @property
    def has_fp32(self) -> bool:
        """cbw_kws_finalize built the fp32 / compensated re-scoring networks: it does for n_layers <= 4 (every
        efficient_kws config uses 3), the handles ``rescore`` / ``score_exact`` serve.  CB-Whisper's own 12-channel
        spotter gets the same networks on request (``build_exact``) and reports them as ``has_exact_resized``."""
        return self.n_layers <= 4

    @property
    def has_exact_resized(self) -> bool:
        """The exact tiers of the resized spotter (``rescore_resized`` / ``score_resized_exact``) are available: a
        raw-hs engine whose fp32 and compensated networks exist, from cbw_kws_finalize or ``build_exact``."""
        return self.variant == VARIANT_L and (self.has_fp32 or self._exact_built)

    def build_exact(self) -> "KwsEngine":
        """Build the fp32 and compensated networks of a raw-hs engine with more than 4 layers (cbw_kws_build_exact):
        what cbw_kws_finalize leaves out for the 12-channel CNN, so that an engine that never re-scores pays
        nothing.  Setup-time (synchronises); no work where they exist."""
        if self.variant != VARIANT_L:
            raise ValueError("build_exact serves the resized spotter: build the engine with learn_features=False")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cbw_kws_build_exact(self.h), "cbw_kws_build_exact")
        self._exact_built = True
        return self

    @property
    def feat_dim(self) -> int:
        return self.D if self.variant == VARIANT_L else self.U

    def out_frames(self, T: int) -> int:
        return lef_frames(T) if self.variant == VARIANT_LEF else T

    # ------------------------------------------------------------------ projection
    def project(self, x: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x f32 [B, L, T, D], mask f32 [B, L, T] (device) -> (bf16 [B, L, T', E], f32 [B, L, T'])."""
        x = x.to(self.device, torch.float32).contiguous()
        mask = mask.to(self.device, torch.float32).contiguous()
        B, L, T, D = x.shape
        if L != self.n_layers or D != self.D:
            raise ValueError(f"expected [B, {self.n_layers}, T, {self.D}] features, got {tuple(x.shape)}")
        if tuple(mask.shape) != (B, L, T):
            raise ValueError(f"mask shape {tuple(mask.shape)} != {(B, L, T)}")
        To = self.out_frames(T)
        out = torch.empty((B, L, To, self.feat_dim), dtype=torch.bfloat16, device=self.device)
        mout = torch.empty((B, L, To), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nb = self.lib.cbw_kws_project_workspace_bytes(self.h, B, T)
            ws = self._pws.get(nb, self.device)
            _lib.check(self.lib.cbw_kws_project(self.h, x.data_ptr(), mask.data_ptr(), B, T, out.data_ptr(),
                                                mout.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle()),
                       "cbw_kws_project")
        return out, mout

    def project_f32(self, x: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """fp32 projection (the exact re-scoring path): x f32 [B, L, T, D] -> (f32 [B, L, T', E], f32 [B, L, T'])."""
        x = x.to(self.device, torch.float32).contiguous()
        mask = mask.to(self.device, torch.float32).contiguous()
        B, L, T, D = x.shape
        if L != self.n_layers or D != self.D or tuple(mask.shape) != (B, L, T):
            raise ValueError(f"expected [B, {self.n_layers}, T, {self.D}] features + [B, L, T] mask")
        To = self.out_frames(T)
        out = torch.empty((B, L, To, self.feat_dim), dtype=torch.float32, device=self.device)
        mout = torch.empty((B, L, To), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nb = self.lib.cbw_kws_project_f32_workspace_bytes(self.h, B, T)
            ws = self._pws.get(nb, self.device)
            _lib.check(self.lib.cbw_kws_project_f32(self.h, x.data_ptr(), mask.data_ptr(), B, T, out.data_ptr(),
                                                    mout.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle()),
                       "cbw_kws_project_f32")
        return out, mout

    def rescore(self, utt32: torch.Tensor, utt_mask: torch.Tensor, kwd32: torch.Tensor, kwd_mask: torch.Tensor,
                logits: torch.Tensor, sel: torch.Tensor, trusted: bool = False, tier: str = "fp32") -> torch.Tensor:
        """Re-scored ResNet logits for the keywords ``sel`` (indices into kwd32), written into ``logits`` [K, 2]
        in place.  tier "fp32": fp32-input MFMA (cbw_kws_rescore); "x3": compensated bf16, the 3-term split
        on the bf16 MFMA kernels (cbw_kws_rescore_x3).  utt32 f32 [L, Tu, E], kwd32 f32 [K, L, Tk, E]
        from project_f32."""
        if utt32.dim() == 4:
            utt32, utt_mask = utt32[0], utt_mask.reshape(utt_mask.shape[-2:])
        K, L, Tk, E = kwd32.shape
        Tu = utt32.shape[1]
        if utt32.dtype != torch.float32 or kwd32.dtype != torch.float32 or tuple(utt32.shape) != (L, Tu, E):
            raise ValueError("rescore takes the fp32 projections (KwsEngine.project_f32)")
        if tier not in ("fp32", "x3"):
            raise ValueError(f"unknown re-scoring tier {tier}")
        sel = sel.to(self.device, torch.int32).contiguous()
        n = sel.numel()
        if n == 0:
            return logits
        if tuple(logits.shape) != (K, 2) or tuple(kwd_mask.shape) != (K, L, Tk):
            # sel indexes the logits rows and the keyword rows alike (``trusted`` skips only the sel range check)
            raise ValueError(f"rescore: logits {tuple(logits.shape)} / mask {tuple(kwd_mask.shape)} for {K} keywords")
        if not trusted and (int(sel.min()) < 0 or int(sel.max()) >= K):
            raise ValueError("sel out of range")
        wsq, call = ((self.lib.cbw_kws_rescore_workspace_bytes, self.lib.cbw_kws_rescore) if tier == "fp32" else
                     (self.lib.cbw_kws_rescore_x3_workspace_bytes, self.lib.cbw_kws_rescore_x3))
        with torch.cuda.device(self.device):
            nb = wsq(self.h, Tk, Tu)
            if nb < 0:
                _lib.check(-4, f"cbw_kws_rescore ({tier}) workspace")
            ws = self._ws_rescore.get(nb, self.device)
            _lib.check(call(self.h, utt32.contiguous().data_ptr(), utt_mask.to(torch.float32).contiguous().data_ptr(),
                            kwd32.contiguous().data_ptr(), kwd_mask.to(torch.float32).contiguous().data_ptr(), K, Tk,
                            Tu, sel.data_ptr(), n, logits.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle()),
                       f"cbw_kws_rescore ({tier})")
        return logits

    def rescore_pairs(self, utt32: torch.Tensor, utt_mask: torch.Tensor, kwd32: torch.Tensor, kwd_mask: torch.Tensor,
                      pair_utt, pair_kwd, logits: torch.Tensor, sel, trusted: bool = False,
                      tier: str = "fp32") -> torch.Tensor:
        """The pairs form of ``rescore`` (cbw_kws_rescore_pairs / cbw_kws_rescore_x3_pairs): utt32 f32 [B, L, Tu, E],
        utt_mask f32 [B, L, Tu], kwd32 f32 [K, L, Tk, E] from project_f32; pair p = (pair_utt[p], pair_kwd[p]) as
        ``score_pairs`` takes them, or both None for every utterance against every keyword (p = b * K + k).  ``sel``
        indexes the P pairs, which are the rows of ``logits`` (contiguous f32, 2 P elements: [P, 2] or [B, K, 2]);
        the selected rows are rewritten in place with the tier's logits, bit-identical to what ``rescore`` gives for
        that utterance and keyword alone.  The index ranges are checked before any launch unless ``trusted``."""
        utt32, utt_mask, kwd32, kwd_mask = self._check_batch(utt32, utt_mask, kwd32, kwd_mask, dtype=torch.float32)
        if tier not in ("fp32", "x3"):
            raise ValueError(f"unknown re-scoring tier {tier}")
        K, _, Tk, _ = kwd32.shape
        B, _, Tu, _ = utt32.shape
        pu, pk, P = self._pair_list(pair_utt, pair_kwd, B, K, trusted)
        sel = self._pair_index(sel, P, trusted, "sel")
        n = sel.numel()
        if n == 0:
            return logits
        if n > P:
            raise ValueError(f"sel has {n} entries for {P} pairs")
        if (logits.numel() != 2 * P or logits.shape[-1] != 2 or logits.dtype != torch.float32
                or not logits.is_contiguous() or logits.device != self.device):
            raise ValueError(f"rescore_pairs: logits must be contiguous f32 on {self.device} with one row of 2 per pair "
                             f"({P} pairs), got {tuple(logits.shape)} {logits.dtype}")
        wsq, call = ((self.lib.cbw_kws_rescore_workspace_bytes, self.lib.cbw_kws_rescore_pairs) if tier == "fp32" else
                     (self.lib.cbw_kws_rescore_x3_workspace_bytes, self.lib.cbw_kws_rescore_x3_pairs))
        with torch.cuda.device(self.device):
            nb = wsq(self.h, Tk, Tu)
            if nb < 0:
                _lib.check(-4, f"cbw_kws_rescore_pairs ({tier}) workspace")
            ws = self._ws_rescore.get(nb, self.device)
            _lib.check(call(self.h, utt32.data_ptr(), utt_mask.data_ptr(), B, kwd32.data_ptr(), kwd_mask.data_ptr(), K,
                            Tk, Tu, _lib.ptr(pu), _lib.ptr(pk), P, sel.data_ptr(), n, logits.data_ptr(), ws.data_ptr(),
                            ws.numel(), _lib.stream_handle()), f"cbw_kws_rescore_pairs ({tier})")
        return logits

    def calibrate_bias(self, utt32: Optional[torch.Tensor] = None, utt_mask: Optional[torch.Tensor] = None,
                       kwd32: Optional[torch.Tensor] = None, kwd_mask: Optional[torch.Tensor] = None,
                       sel: Optional[torch.Tensor] = None, utt: Optional[torch.Tensor] = None,
                       kwd: Optional[torch.Tensor] = None) -> Optional[np.ndarray]:
        """Bias correction of the bf16 scoring network (cbw_kws_calibrate_bias): the fp32 network over the
        calibration pairs ``sel`` (default: every keyword of kwd32) gives each conv's mean input per channel,
        and the bf16 convs' biases absorb the mean shift of their rounded weights.  With the bf16 projections of
        the same pairs (``utt`` [L, Tu, E], ``kwd`` [K, L, Tk, E] bf16, masks shared), the mean fp32 - bf16 logit
        difference that remains is then taken out of the bf16 pass's classifier bias (cbw_kws_set_score_offset)
        and returned.  Inputs as rescore; no arguments restores the folded biases and a zero offset.
        Setup-time (synchronises)."""
        if utt32 is None:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.cbw_kws_calibrate_bias(self.h, None, None, None, None, 0, 1, 1, None, 0, None, 0,
                                                           _lib.stream_handle()), "cbw_kws_calibrate_bias")
            return
        utt32, utt_mask, sel, ws = self._calibration_inputs("calibrate_bias", utt32, utt_mask, kwd32, sel)
        K, _, Tk, _ = kwd32.shape
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cbw_kws_calibrate_bias(
                self.h, utt32.contiguous().data_ptr(), utt_mask.to(torch.float32).contiguous().data_ptr(),
                kwd32.contiguous().data_ptr(), kwd_mask.to(torch.float32).contiguous().data_ptr(), K, Tk,
                utt32.shape[1], sel.data_ptr(), sel.numel(), ws.data_ptr(), ws.numel(), _lib.stream_handle()),
                "cbw_kws_calibrate_bias")
        return self._calibrate_offset(self.score, "cbw_kws_set_score_offset", utt32, utt_mask, kwd32, kwd_mask, sel,
                                      utt, kwd)

    def _calibration_inputs(self, what: str, utt32, utt_mask, kwd32, sel):
        """Prologue of calibrate_bias / calibrate_fp8: the utterance without its batch axis of 1, the fp32 check,
        ``sel`` (default: every keyword) on the device and range-checked, the re-scoring workspace."""
        if utt32.dim() == 4:
            utt32, utt_mask = utt32[0], utt_mask.reshape(utt_mask.shape[-2:])
        K, L, Tk, E = kwd32.shape
        Tu = utt32.shape[1]
        if utt32.dtype != torch.float32 or kwd32.dtype != torch.float32 or tuple(utt32.shape) != (L, Tu, E):
            raise ValueError(f"{what} takes the fp32 projections (KwsEngine.project_f32)")
        if sel is None:
            sel = torch.arange(K, dtype=torch.int32, device=self.device)
        sel = sel.to(self.device, torch.int32).contiguous()
        if sel.numel() == 0 or int(sel.min()) < 0 or int(sel.max()) >= K:
            raise ValueError("calibration pairs out of range")
        with torch.cuda.device(self.device):
            nb = self.lib.cbw_kws_rescore_workspace_bytes(self.h, Tk, Tu)
            if nb < 0:
                _lib.check(-4, f"cbw_kws_{what} workspace")
            return utt32, utt_mask, sel, self._ws_rescore.get(nb, self.device)

    def _calibrate_offset(self, score, setter: str, utt32, utt_mask, kwd32, kwd_mask, sel, utt, kwd):
        """Tail of calibrate_bias / calibrate_fp8: with the bf16 projections of the calibration pairs, zero the
        tier's logit offset, score the pairs with ``score``, re-score them in fp32 and set (and return) the mean
        difference as the offset; None without them."""
        if utt is None or kwd is None:
            return None
        set_offset = getattr(self.lib, setter)
        zero = np.zeros(2, np.float32)
        _lib.check(set_offset(self.h, zero.ctypes.data), setter)
        if utt.dim() == 4:
            utt = utt[0]
        s_l = sel.long()
        km = kwd_mask[s_l].contiguous()
        low = score(utt, utt_mask, kwd[s_l].contiguous(), km)
        l32 = torch.empty_like(low)
        self.rescore(utt32, utt_mask, kwd32[s_l].contiguous(), km, l32,
                     torch.arange(sel.numel(), dtype=torch.int32, device=self.device), trusted=True)
        off = (l32.double() - low.double()).mean(0).cpu().numpy().astype(np.float32)
        _lib.check(set_offset(self.h, np.ascontiguousarray(off).ctypes.data), setter)
        return off

    # ------------------------------------------------------------------ fp8 first tier
    def calibrate_fp8(self, utt32: torch.Tensor, utt_mask: torch.Tensor, kwd32: torch.Tensor, kwd_mask: torch.Tensor,
                      sel: Optional[torch.Tensor] = None, margin: float = 1.0, utt: Optional[torch.Tensor] = None,
                      kwd: Optional[torch.Tensor] = None) -> Optional[np.ndarray]:
        """Build the fp8 tier (cbw_kws_calibrate_fp8): the fp32 network over the calibration pairs ``sel``
        (default: every keyword of kwd32) gives each stage-2..4 tensor's absolute maximum, its e4m3 scale is
        amax * margin / 448 and the weights are quantized against it.  With the bf16 projections of the same pairs
        (``utt`` [L, Tu, E], ``kwd`` [K, L, Tk, E]) the mean fp32 - fp8 logit difference is then moved into the fp8
        pass's classifier bias (cbw_kws_set_score_offset_fp8) and returned.  Setup-time (synchronises)."""
        utt32, utt_mask, sel, ws = self._calibration_inputs("calibrate_fp8", utt32, utt_mask, kwd32, sel)
        K, _, Tk, _ = kwd32.shape
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cbw_kws_calibrate_fp8(
                self.h, utt32.contiguous().data_ptr(), utt_mask.to(torch.float32).contiguous().data_ptr(),
                kwd32.contiguous().data_ptr(), kwd_mask.to(torch.float32).contiguous().data_ptr(), K, Tk,
                utt32.shape[1], sel.data_ptr(), sel.numel(), float(margin), ws.data_ptr(), ws.numel(),
                _lib.stream_handle()), "cbw_kws_calibrate_fp8")
        return self._calibrate_offset(self.score_fp8, "cbw_kws_set_score_offset_fp8", utt32, utt_mask, kwd32, kwd_mask,
                                      sel, utt, kwd)

    def fp8_scales(self) -> np.ndarray:
        n = self.lib.cbw_kws_fp8_scales(self.h, None, 0)
        out = np.zeros(max(n, 1), np.float32)
        self.lib.cbw_kws_fp8_scales(self.h, out.ctypes.data, n)
        return out[:n]

    def score_fp8(self, utt: torch.Tensor, utt_mask: torch.Tensor, kwd: torch.Tensor, kwd_mask: torch.Tensor,
                  chunk: Optional[int] = None, logits_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Logits of every pair from the fp8 tier (cbw_kws_score_fp8); inputs as ``score``."""
        utt, utt_mask, kwd, kwd_mask = self._check_single(utt, utt_mask, kwd, kwd_mask)
        K, _, Tk, _ = kwd.shape
        Tu = utt.shape[1]
        chunk = chunk or self.default_chunk(Tk, Tu)
        logits = self._logits(logits_out, (K, 2))
        with torch.cuda.device(self.device):
            ws = self.workspace(Tk, Tu, chunk)
            _lib.check(self.lib.cbw_kws_score_fp8(self.h, utt.data_ptr(), utt_mask.data_ptr(), kwd.data_ptr(),
                                                  kwd_mask.data_ptr(), K, Tk, Tu, logits.data_ptr(), chunk,
                                                  ws.data_ptr(), ws.numel(), _lib.stream_handle()), "cbw_kws_score_fp8")
        return logits

    def band(self, logits: torch.Tensor, threshold: float, band: float, ghost: Optional[torch.Tensor] = None,
             idx_out: Optional[torch.Tensor] = None, n_out: Optional[torch.Tensor] = None,
             scaled: bool = False) -> Tuple[torch.Tensor, int]:
        """Sorted keyword indices whose probability lies within ``band`` of ``threshold`` (cbw_kws_band), or with
        ``scaled`` within ``band`` x max(|l0|, |l1|) of it (cbw_kws_band_scaled): (device int32 [n], n).  Reads the
        count back to the host (one stream sync)."""
        logits = logits.to(torch.float32).contiguous()
        K = logits.shape[0]
        idx = idx_out if idx_out is not None else torch.empty((max(K, 1),), dtype=torch.int32, device=logits.device)
        n = n_out if n_out is not None else torch.zeros((1,), dtype=torch.int32, device=logits.device)
        g = None if ghost is None else ghost.to(logits.device, torch.float32).contiguous()
        if g is not None and g.numel() != K:
            raise ValueError(f"ghost mask of {g.numel()} entries for {K} logits")
        if idx.numel() < max(K, 1) or n.numel() < 1:
            raise ValueError("band output buffers too small")
        with torch.cuda.device(logits.device):
            fn = self.lib.cbw_kws_band_scaled if scaled else self.lib.cbw_kws_band
            _lib.check(fn(logits.data_ptr(), _lib.ptr(g), K, float(threshold), float(band), idx.data_ptr(),
                          n.data_ptr(), _lib.stream_handle()), "cbw_kws_band")
        cnt = int(n.item())
        return idx[:cnt], cnt

    def score_exact(self, utt: torch.Tensor, utt_mask: torch.Tensor, kwd: torch.Tensor, kwd_mask: torch.Tensor,
                    utt32: torch.Tensor, kwd32: torch.Tensor, threshold: float, band: float,
                    ghost: Optional[torch.Tensor] = None, chunk: Optional[int] = None,
                    logits_out: Optional[torch.Tensor] = None, band_x3: Optional[float] = None,
                    band_scaled: bool = False, fp8_band: Optional[float] = None):
        """bf16 scoring of every pair, then the near-threshold pairs re-scored from the cached fp32
        projections ``utt32`` [L, Tu, E] / ``kwd32`` [K, L, Tk, E] (project_f32):

        * ``band_x3`` None: every pair within ``band`` of ``threshold`` in fp32 (cbw_kws_band + cbw_kws_rescore);
        * ``band_x3`` = b2 < band: the pairs within ``band`` on the compensated-bf16 tier (cbw_kws_rescore_x3),
          then those of them still within b2 of the threshold in fp32.  Pairs outside ``band`` cannot enter b2
          (their logits are untouched), so the fp32 decision is reproduced as long as the bf16 error < band
          and the compensated error < b2.

        ``band_scaled``: the first band is ``band`` x max(|l0|, |l1|) per pair (cbw_kws_band_scaled).

        ``fp8_band`` (the fp8 first tier, calibrate_fp8 first): every pair is scored by the fp8 network
        (score_fp8); only the pairs within ``fp8_band`` of the threshold are scored in bf16 (their keywords gathered
        into one batch), then the tiers above.  Pairs outside ``fp8_band`` keep their fp8 logits and cannot enter
        the later bands (fp8_band > band), so the fp32 decision is reproduced as long as the fp8 error < fp8_band.

        Returns (logits f32 [K, 2], {"band": pairs re-scored after bf16, "fp32": pairs re-scored in fp32,
        "bf16": pairs scored in bf16})."""
        stats = {"band": 0, "fp32": 0, "bf16": kwd.shape[0]}
        if fp8_band is not None and kwd.shape[0] > 0:
            if fp8_band <= band:
                raise ValueError("fp8_band must exceed the bf16 band")
            logits = self.score_fp8(utt, utt_mask, kwd, kwd_mask, chunk=chunk, logits_out=logits_out)
            sel8, n8 = self.band(logits, threshold, fp8_band, ghost)
            stats["bf16"] = n8
            if n8:
                s_l = sel8.long()
                sub = self.score(utt, utt_mask, kwd.index_select(0, s_l), kwd_mask.index_select(0, s_l), chunk=chunk)
                logits.index_copy_(0, s_l, sub)
        else:
            logits = self.score(utt, utt_mask, kwd, kwd_mask, chunk=chunk, logits_out=logits_out)
        if band <= 0 or kwd.shape[0] == 0:
            return logits, stats
        sel, n = self.band(logits, threshold, band, ghost, scaled=band_scaled)
        stats["band"] = n
        if n == 0:
            return logits, stats
        um = utt_mask.reshape(utt_mask.shape[-2:]) if utt_mask.dim() == 3 else utt_mask
        if band_x3 is None:
            self.rescore(utt32, um, kwd32, kwd_mask, logits, sel, trusted=True)
            stats["fp32"] = n
            return logits, stats
        self.rescore(utt32, um, kwd32, kwd_mask, logits, sel, trusted=True, tier="x3")
        sel2, n2 = self.band(logits, threshold, band_x3, ghost)
        if n2:
            self.rescore(utt32, um, kwd32, kwd_mask, logits, sel2, trusted=True)
        stats["fp32"] = n2
        return logits, stats

    # ------------------------------------------------------------------ scoring
    def default_chunk(self, Tk: int, Tu: int, budget_bytes: int = 2 << 30) -> int:
        per = self.lib.cbw_kws_workspace_bytes(self.h, Tk, Tu, 1)
        return int(max(1, min(1024, budget_bytes // max(per, 1))))

    def workspace(self, Tk: int, Tu: int, chunk: int) -> torch.Tensor:
        nb = self.lib.cbw_kws_workspace_bytes(self.h, Tk, Tu, chunk)
        if nb < 0:
            raise ValueError("bad workspace query")
        return self._ws.get(nb, self.device)

    def score(self, utt: torch.Tensor, utt_mask: torch.Tensor, kwd: torch.Tensor, kwd_mask: torch.Tensor,
              features: bool = False, chunk: Optional[int] = None, logits_out: Optional[torch.Tensor] = None):
        """utt bf16 [L, Tu, E] (or [1, L, Tu, E]), utt_mask f32 [L, Tu]; kwd bf16 [K, L, Tk, E],
        kwd_mask f32 [K, L, Tk]  ->  logits f32 [K, 2] (+ features f32 [K, L, Tk, Tu])."""
        utt, utt_mask, kwd, kwd_mask = self._check_single(utt, utt_mask, kwd, kwd_mask)
        K, L, Tk, _ = kwd.shape
        Tu = utt.shape[1]
        chunk = chunk or self.default_chunk(Tk, Tu)
        logits = self._logits(logits_out, (K, 2))
        feats = torch.empty((K, L, Tk, Tu), dtype=torch.float32, device=self.device) if features else None
        with torch.cuda.device(self.device):
            ws = self.workspace(Tk, Tu, chunk)
            _lib.check(self.lib.cbw_kws_score(self.h, utt.data_ptr(), utt_mask.data_ptr(), kwd.data_ptr(),
                                              kwd_mask.data_ptr(), K, Tk, Tu, logits.data_ptr(), _lib.ptr(feats), chunk,
                                              ws.data_ptr(), ws.numel(), _lib.stream_handle()), "cbw_kws_score")
        return (logits, feats) if features else logits

    def _check_single(self, utt, utt_mask, kwd, kwd_mask):
        """Shape / dtype checks of ``score`` and ``score_fp8``: utt bf16 [L, Tu, E] or [1, L, Tu, E], a utt_mask of
        L * Tu elements (reshaped to [L, Tu]), kwd bf16 [K, L, Tk, E], kwd_mask [K, L, Tk].  Returns the four
        tensors contiguous, the masks in f32."""
        if utt.dim() == 4:
            utt = utt[0]
        if utt.dim() != 3 or kwd.dim() != 4:
            raise ValueError(f"expected utt [L, Tu, E] and kwd [K, L, Tk, E], got {tuple(utt.shape)} "
                             f"{tuple(kwd.shape)}")
        K, L, Tk, E = kwd.shape
        Tu = utt.shape[1]
        if L != self.n_layers or E != self.feat_dim or tuple(utt.shape) != (L, Tu, E):
            raise ValueError(f"shape mismatch: kwd {tuple(kwd.shape)} utt {tuple(utt.shape)}")
        if utt.dtype != torch.bfloat16 or kwd.dtype != torch.bfloat16:
            raise ValueError("projected features must be bf16 (use KwsEngine.project)")
        if tuple(kwd_mask.shape) != (K, L, Tk) or utt_mask.numel() != L * Tu:
            raise ValueError(f"mask shapes {tuple(kwd_mask.shape)} {tuple(utt_mask.shape)} for kwd {tuple(kwd.shape)} "
                             f"utt {tuple(utt.shape)}")
        return (utt.contiguous(), utt_mask.reshape(L, Tu).to(torch.float32).contiguous(), kwd.contiguous(),
                kwd_mask.to(torch.float32).contiguous())

    def _logits(self, logits_out, shape):
        """The caller's ``logits_out`` if it is a contiguous f32 tensor of ``shape``, a new tensor if None."""
        if logits_out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        if tuple(logits_out.shape) != shape or logits_out.dtype != torch.float32 or not logits_out.is_contiguous():
            raise ValueError(f"logits_out must be contiguous f32 {list(shape)}, got {tuple(logits_out.shape)}")
        return logits_out

    def _check_batch(self, utt, utt_mask, kwd, kwd_mask, dtype=torch.bfloat16):
        """Shape / dtype checks of ``score`` for a batch of utterances: utt bf16 [B, L, Tu, E]; with ``dtype``
        torch.float32 the same checks on the fp32 projections the re-scoring tiers take."""
        if utt.dim() != 4 or kwd.dim() != 4:
            raise ValueError(f"expected utt [B, L, Tu, E] and kwd [K, L, Tk, E], got {tuple(utt.shape)} "
                             f"{tuple(kwd.shape)}")
        K, L, Tk, E = kwd.shape
        B, _, Tu, _ = utt.shape
        if B < 1 or L != self.n_layers or E != self.feat_dim or tuple(utt.shape) != (B, L, Tu, E):
            raise ValueError(f"shape mismatch: kwd {tuple(kwd.shape)} utt {tuple(utt.shape)}")
        if utt.dtype != dtype or kwd.dtype != dtype:
            raise ValueError("projected features must be bf16 (use KwsEngine.project)" if dtype == torch.bfloat16 else
                             "the re-scoring tiers take the fp32 projections (KwsEngine.project_f32)")
        if tuple(kwd_mask.shape) != (K, L, Tk) or tuple(utt_mask.shape) != (B, L, Tu):
            raise ValueError(f"mask shapes {tuple(kwd_mask.shape)} {tuple(utt_mask.shape)} for kwd {tuple(kwd.shape)} "
                             f"utt {tuple(utt.shape)}")
        return (utt.contiguous(), utt_mask.to(torch.float32).contiguous(), kwd.contiguous(),
                kwd_mask.to(torch.float32).contiguous())

    def _pair_index(self, idx, n: int, trusted: bool, what: str) -> torch.Tensor:
        if torch.is_tensor(idx):
            if idx.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{what} must hold integers, got {idx.dtype}")
        else:
            idx = torch.as_tensor(np.asarray(idx, dtype=np.int64).reshape(-1))
        idx = idx.reshape(-1)
        if not trusted and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise ValueError(f"{what} out of range [0, {n})")
        return idx.to(self.device, torch.int32).contiguous()

    def score_pairs(self, utt: torch.Tensor, utt_mask: torch.Tensor, kwd: torch.Tensor, kwd_mask: torch.Tensor,
                    pair_utt, pair_kwd, chunk: Optional[int] = None, features: bool = False,
                    logits_out: Optional[torch.Tensor] = None, trusted: bool = False):
        """A list of (utterance, keyword) pairs in one pass (cbw_kws_score_pairs): utt bf16 [B, L, Tu, E], utt_mask
        f32 [B, L, Tu], kwd / kwd_mask as ``score``; pair p = (pair_utt[p], pair_kwd[p]), host sequences or device
        integer tensors of one length P  ->  logits f32 [P, 2] in pair order (+ features f32 [P, L, Tk, Tu]).
        The index ranges are checked before any launch (one host read-back for device tensors) unless ``trusted``."""
        utt, utt_mask, kwd, kwd_mask = self._check_batch(utt, utt_mask, kwd, kwd_mask)
        K, L, Tk, _ = kwd.shape
        B, _, Tu, _ = utt.shape
        pu = self._pair_index(pair_utt, B, trusted, "pair_utt")
        pk = self._pair_index(pair_kwd, K, trusted, "pair_kwd")
        P = pu.numel()
        if pk.numel() != P:
            raise ValueError(f"pair_utt has {P} entries, pair_kwd {pk.numel()}")
        if P > 0 and K < 1:
            raise ValueError("pairs given but no keywords")
        logits = self._logits(logits_out, (P, 2))
        feats = torch.empty((P, L, Tk, Tu), dtype=torch.float32, device=self.device) if features else None
        self._call_score_pairs(utt, utt_mask, kwd, kwd_mask, pu, pk, P, logits, feats, chunk)
        return (logits, feats) if features else logits

    def _call_score_pairs(self, utt, utt_mask, kwd, kwd_mask, pu, pk, P, logits, feats, chunk):
        """cbw_kws_score_pairs on checked inputs (``_check_batch``); pu / pk None = every utterance x every keyword."""
        if P == 0:
            return
        K, _, Tk, _ = kwd.shape
        B, _, Tu, _ = utt.shape
        chunk = chunk or self.default_chunk(Tk, Tu)
        with torch.cuda.device(self.device):
            ws = self.workspace(Tk, Tu, chunk)
            _lib.check(self.lib.cbw_kws_score_pairs(
                self.h, utt.data_ptr(), utt_mask.data_ptr(), B, kwd.data_ptr(), kwd_mask.data_ptr(), K, Tk, Tu,
                _lib.ptr(pu), _lib.ptr(pk), P, logits.data_ptr(), _lib.ptr(feats), chunk, ws.data_ptr(), ws.numel(),
                _lib.stream_handle()), "cbw_kws_score_pairs")

    def score_batch(self, utt: torch.Tensor, utt_mask: torch.Tensor, kwd: torch.Tensor, kwd_mask: torch.Tensor,
                    chunk: Optional[int] = None, logits_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Every utterance of a batch against every keyword in one pass (cbw_kws_score_pairs without index arrays:
        chunks of pairs may span utterances): utt bf16 [B, L, Tu, E], utt_mask f32 [B, L, Tu]  ->  logits f32
        [B, K, 2], row b what ``score`` gives for utterance b."""
        utt, utt_mask, kwd, kwd_mask = self._check_batch(utt, utt_mask, kwd, kwd_mask)
        B, K = utt.shape[0], kwd.shape[0]
        logits = self._logits(logits_out, (B, K, 2))
        self._call_score_pairs(utt, utt_mask, kwd, kwd_mask, None, None, B * K, logits, None, chunk)
        return logits

    def _pair_list(self, pair_utt, pair_kwd, B: int, K: int, trusted: bool):
        """(pair_utt, pair_kwd, P) as device int32 tensors through ``_pair_index``, or (None, None, B * K) for both
        None: every utterance against every keyword, pair p = b * K + k."""
        if pair_utt is None and pair_kwd is None:
            return None, None, B * K
        if pair_utt is None or pair_kwd is None:
            raise ValueError("pair_utt and pair_kwd must both be given or both be None")
        pu = self._pair_index(pair_utt, B, trusted, "pair_utt")
        pk = self._pair_index(pair_kwd, K, trusted, "pair_kwd")
        if pk.numel() != pu.numel():
            raise ValueError(f"pair_utt has {pu.numel()} entries, pair_kwd {pk.numel()}")
        if pu.numel() > 0 and K < 1:
            raise ValueError("pairs given but no keywords")
        return pu, pk, pu.numel()

    def score_pairs_exact(self, utt: torch.Tensor, utt_mask: torch.Tensor, kwd: torch.Tensor, kwd_mask: torch.Tensor,
                          utt32: torch.Tensor, kwd32: torch.Tensor, pair_utt, pair_kwd, threshold: float, band: float,
                          ghost: Optional[torch.Tensor] = None, chunk: Optional[int] = None,
                          logits_out: Optional[torch.Tensor] = None, band_x3: Optional[float] = None,
                          band_scaled: bool = False, trusted: bool = False, features: bool = False):
        """``score_exact`` for a pair list: every pair scored in bf16 in one pass (``score_pairs``), one band
        selection over the P rows (cbw_kws_band), then the selected pairs re-scored from the fp32 projections
        ``utt32`` [B, L, Tu, E] / ``kwd32`` [K, L, Tk, E] by ``rescore_pairs`` -- in fp32, or with ``band_x3`` on the
        compensated tier and then those still within ``band_x3`` in fp32, sequenced as ``score_exact`` does.  One
        host read-back per band selection and one re-scoring call per tier for the whole list, where P
        ``score_exact`` calls pay both per utterance.  pair_utt / pair_kwd as ``score_pairs``, or both None for the
        cross product p = b * K + k.  ``ghost`` is the per-keyword mask f32 [K] of ``score_exact``, gathered to pair
        order on the device.  The fp8 first tier stays per utterance (``score_exact``'s ``fp8_band``); it has no
        pairs form.

        Returns (logits f32 [P, 2], stats) with ``score_exact``'s stats keys (+ the bf16 pass's features f32
        [P, L, Tk, Tu] as a third element with ``features``)."""
        utt, utt_mask, kwd, kwd_mask = self._check_batch(utt, utt_mask, kwd, kwd_mask)
        K, L, Tk, _ = kwd.shape
        B, _, Tu, _ = utt.shape
        pu, pk, P = self._pair_list(pair_utt, pair_kwd, B, K, trusted)
        logits = self._logits(logits_out, (P, 2))
        feats = torch.empty((P, L, Tk, Tu), dtype=torch.float32, device=self.device) if features else None
        self._call_score_pairs(utt, utt_mask, kwd, kwd_mask, pu, pk, P, logits, feats, chunk)
        stats = {"band": 0, "fp32": 0, "bf16": P}

        def done():
            return (logits, stats, feats) if features else (logits, stats)
        if band <= 0 or P == 0:
            return done()
        g = None
        if ghost is not None:
            g = ghost.to(self.device, torch.float32).reshape(-1)
            if g.numel() != K:
                raise ValueError(f"ghost mask of {g.numel()} entries for {K} keywords")
            g = g.repeat(B) if pk is None else g[pk.long()]
        sel, n = self.band(logits, threshold, band, g, scaled=band_scaled)
        stats["band"] = n
        if n == 0:
            return done()
        if band_x3 is None:
            self.rescore_pairs(utt32, utt_mask, kwd32, kwd_mask, pu, pk, logits, sel, trusted=True)
            stats["fp32"] = n
            return done()
        self.rescore_pairs(utt32, utt_mask, kwd32, kwd_mask, pu, pk, logits, sel, trusted=True, tier="x3")
        sel2, n2 = self.band(logits, threshold, band_x3, g)
        if n2:
            self.rescore_pairs(utt32, utt_mask, kwd32, kwd_mask, pu, pk, logits, sel2, trusted=True)
        stats["fp32"] = n2
        return done()

    def score_batch_exact(self, utt: torch.Tensor, utt_mask: torch.Tensor, kwd: torch.Tensor, kwd_mask: torch.Tensor,
                          utt32: torch.Tensor, kwd32: torch.Tensor, threshold: float, band: float,
                          ghost: Optional[torch.Tensor] = None, chunk: Optional[int] = None,
                          logits_out: Optional[torch.Tensor] = None, band_x3: Optional[float] = None,
                          band_scaled: bool = False):
        """``score_exact`` for every utterance of a batch against every keyword: ``score_pairs_exact`` over the cross
        product without index arrays, the per-keyword ``ghost`` tiled over the B utterances -- one band selection
        and one re-scoring call per tier for the whole batch.  Returns (logits f32 [B, K, 2], stats): row b is what
        ``score_exact`` gives for utterance b, the stats are the sums over b.  No fp8 first tier (per utterance
        only)."""
        utt, utt_mask, kwd, kwd_mask = self._check_batch(utt, utt_mask, kwd, kwd_mask)
        B, K = utt.shape[0], kwd.shape[0]
        out = self._logits(logits_out, (B, K, 2))
        _, stats = self.score_pairs_exact(utt, utt_mask, kwd, kwd_mask, utt32, kwd32, None, None, threshold, band,
                                          ghost=ghost, chunk=chunk, logits_out=out.view(B * K, 2), band_x3=band_x3,
                                          band_scaled=band_scaled, trusted=True)
        return out, stats

    def classify(self, maps: torch.Tensor, chunk: Optional[int] = None) -> torch.Tensor:
        """Resnet.forward (resnet.py:51-58) on NCHW f32 maps [K, L, H, W] -> logits [K, 2]."""
        maps = maps.to(self.device, torch.float32).contiguous()
        K, L, Tk, Tu = maps.shape
        if L != self.n_layers:
            raise ValueError("Make sure that the channel dimension of the pixel values match with the one set in the "
                             "configuration.")
        chunk = chunk or self.default_chunk(Tk, Tu)
        logits = torch.empty((K, 2), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            ws = self.workspace(Tk, Tu, chunk)
            _lib.check(self.lib.cbw_kws_classify(self.h, maps.data_ptr(), K, Tk, Tu, logits.data_ptr(), chunk,
                                                 ws.data_ptr(), ws.numel(), _lib.stream_handle()), "cbw_kws_classify")
        return logits

    def score_resized(self, utt_hs: torch.Tensor, kwd_hs, out_size: Tuple[int, int] = (150, 750),
                      chunk: Optional[int] = None) -> torch.Tensor:
        """CB-Whisper's own spotter (model/cb_whisper.py:110-126, :189-210; model/model.py:78-93):
        utt_hs [L, Tu, D] and keyword hs (a list of [L, Tk_k, D], ragged) per-frame L2-normalised ->
        similarity matrices -> bilinear resize to ``out_size`` -> ResNet -> logits f32 [K, 2].
        ``kwd_hs`` may also be a packed ``(bf16 [L, R, D], int32 offsets [K + 1])`` pair
        (see ``pack_keywords``)."""
        if self.variant != VARIANT_L:
            raise ValueError("score_resized takes raw hs: build the engine with learn_features=False")
        rows, off = kwd_hs if isinstance(kwd_hs, tuple) else pack_keywords(kwd_hs, self.device)
        rows = rows.to(self.device, torch.bfloat16).contiguous()
        off_host = off.to("cpu", torch.int32).contiguous()
        off_dev = off_host.to(self.device)
        utt = utt_hs.to(self.device, torch.bfloat16).contiguous()
        L, Tu, D = utt.shape
        if L != self.n_layers or rows.shape[0] != L or rows.shape[2] != D:
            raise ValueError(f"shape mismatch: utt {tuple(utt.shape)} keyword rows {tuple(rows.shape)}")
        K = off_host.numel() - 1
        Ho, Wo = out_size
        chunk = chunk or self.default_chunk(Ho, Wo, budget_bytes=1 << 30)
        logits = torch.empty((K, 2), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nb = self.lib.cbw_kws_score_resized_workspace_bytes(self.h, off_host.data_ptr(), K, Tu, D, Ho, Wo, chunk)
            if nb < 0:
                _lib.check(-1, "cbw_kws_score_resized_workspace_bytes")
            ws = self._ws.get(nb, self.device)
            _lib.check(self.lib.cbw_kws_score_resized(self.h, utt.data_ptr(), Tu, rows.data_ptr(), rows.shape[1], D,
                                                      off_dev.data_ptr(), off_host.data_ptr(), K, Ho, Wo,
                                                      logits.data_ptr(), chunk, ws.data_ptr(), ws.numel(),
                                                      _lib.stream_handle()), "cbw_kws_score_resized")
        return logits

    def _packed_f32(self, kwd32_packed):
        """A ``pack_keywords(..., dtype=torch.float32)`` pair as (rows f32 [L, R, D] on the device, host offsets,
        device offsets, K)."""
        rows, off = kwd32_packed
        if rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[0] != self.n_layers:
            raise ValueError(f"the exact tiers take fp32 keyword rows [L, R, D] (pack_keywords(dtype=torch.float32)), "
                             f"got {tuple(rows.shape)} {rows.dtype}")
        off_host = off.to("cpu", torch.int32).contiguous()
        return rows.to(self.device).contiguous(), off_host, off_host.to(self.device), off_host.numel() - 1

    def rescore_resized(self, utt32: torch.Tensor, kwd32_packed, out_size: Tuple[int, int], logits: torch.Tensor,
                        sel: torch.Tensor, tier: str = "f32", trusted: bool = False) -> torch.Tensor:
        """The exact tiers of CB-Whisper's own spotter (cbw_kws_rescore_resized / cbw_kws_rescore_resized_x3;
        cb_whisper.py:110-128 as the reference runs it, in fp32 from fp32 hidden states): the logits of the keywords
        ``sel`` (int indices, any order) written into ``logits`` [K, 2] in place, every other row untouched.  utt32
        f32 [L, Tu, D] and kwd32_packed = pack_keywords(..., dtype=torch.float32), both L2-normalised per frame.
        tier "f32": fp32-input MFMA throughout; "x3": the compensated bf16 network.  ``build_exact`` first."""
        if tier not in ("f32", "x3"):
            raise ValueError(f"unknown re-scoring tier {tier}")
        if not self.has_exact_resized:
            raise _lib.CbwError("rescore_resized needs the fp32 networks: call KwsEngine.build_exact() first")
        rows, off_host, off_dev, K = self._packed_f32(kwd32_packed)
        utt = utt32.to(self.device).contiguous()
        L, Tu, D = utt.shape
        if utt.dtype != torch.float32 or L != self.n_layers or rows.shape[2] != D:
            raise ValueError(f"shape mismatch: utt {tuple(utt.shape)} {utt.dtype} keyword rows {tuple(rows.shape)}")
        sel = self._pair_index(sel, K, trusted, "sel")
        n = sel.numel()
        if n == 0:
            return logits
        if (tuple(logits.shape) != (K, 2) or logits.dtype != torch.float32 or not logits.is_contiguous()
                or logits.device != self.device):
            raise ValueError(f"rescore_resized: logits must be contiguous f32 [{K}, 2] on {self.device}, got "
                             f"{tuple(logits.shape)} {logits.dtype}")
        Ho, Wo = out_size
        wsq, call = ((self.lib.cbw_kws_rescore_resized_workspace_bytes, self.lib.cbw_kws_rescore_resized)
                     if tier == "f32" else
                     (self.lib.cbw_kws_rescore_resized_x3_workspace_bytes, self.lib.cbw_kws_rescore_resized_x3))
        with torch.cuda.device(self.device):
            nb = wsq(self.h, off_host.data_ptr(), K, Tu, D, Ho, Wo)
            if nb < 0:
                raise ValueError(f"cbw_kws_rescore_resized ({tier}) workspace: bad arguments "
                                 f"(K {K}, Tu {Tu}, D {D}, out {Ho} x {Wo})")
            ws = self._ws_rescore.get(nb, self.device)
            _lib.check(call(self.h, utt.data_ptr(), Tu, rows.data_ptr(), rows.shape[1], D, off_dev.data_ptr(),
                            off_host.data_ptr(), K, Ho, Wo, sel.data_ptr(), n, logits.data_ptr(), ws.data_ptr(),
                            ws.numel(), _lib.stream_handle()), f"cbw_kws_rescore_resized ({tier})")
        return logits

    def score_resized_exact(self, utt_hs: torch.Tensor, kwd_packed_bf16, kwd_packed_f32,
                            out_size: Tuple[int, int] = (150, 750), band: float = 0.0,
                            band_x3: Optional[float] = 1e-4, chunk: Optional[int] = None):
        """``score_exact`` for CB-Whisper's own spotter, decision argmax(logits) == 1 <=> p > 0.5 (cb_whisper.py:128):
        every keyword scored in bf16 (``score_resized``), the keywords within ``band`` of p = 0.5 re-scored from the
        fp32 hidden states ``utt_hs`` [L, Tu, D] and the fp32 keyword rows ``kwd_packed_f32`` -- on the compensated
        tier and then those still within ``band_x3`` in fp32, or with ``band_x3`` None all of them in fp32.  Keywords
        outside ``band`` keep their bf16 logits, so the fp32 decision is reproduced as long as the bf16 error < band
        and the compensated error < band_x3.

        Returns (logits f32 [K, 2], stats) with ``score_exact``'s stats keys."""
        logits = self.score_resized(utt_hs, kwd_packed_bf16, out_size, chunk=chunk)
        K = logits.shape[0]
        stats = {"band": 0, "fp32": 0, "bf16": K}
        if band <= 0 or K == 0:
            return logits, stats
        sel, n = self.band(logits, 0.5, band)
        stats["band"] = n
        if n == 0:
            return logits, stats
        utt32 = utt_hs.to(self.device, torch.float32)
        if band_x3 is None:
            self.rescore_resized(utt32, kwd_packed_f32, out_size, logits, sel, trusted=True)
            stats["fp32"] = n
            return logits, stats
        self.rescore_resized(utt32, kwd_packed_f32, out_size, logits, sel, tier="x3", trusted=True)
        sel2, n2 = self.band(logits, 0.5, band_x3)
        if n2:
            self.rescore_resized(utt32, kwd_packed_f32, out_size, logits, sel2, trusted=True)
        stats["fp32"] = n2
        return logits, stats

    def score_resized_batch(self, utt_hs: torch.Tensor, kwd_hs, out_size: Tuple[int, int] = (150, 750),
                            chunk: Optional[int] = None) -> torch.Tensor:
        """``score_resized`` for a batch of segments in one pass (cbw_kws_score_resized_batch; cb_whisper.py:87-129,
        where keyword_spotting scores every segment against every keyword): utt_hs [B, L, Tu, D] -> logits f32
        [B, K, 2].  Row b carries the bits ``score_resized(utt_hs[b], ...)`` gives, whatever ``chunk`` (which counts
        (segment, keyword) pairs here) and whatever else the batch holds."""
        if self.variant != VARIANT_L:
            raise ValueError("score_resized_batch takes raw hs: build the engine with learn_features=False")
        rows, off = kwd_hs if isinstance(kwd_hs, tuple) else pack_keywords(kwd_hs, self.device)
        rows = rows.to(self.device, torch.bfloat16).contiguous()
        off_host = off.to("cpu", torch.int32).contiguous()
        off_dev = off_host.to(self.device)
        utt = utt_hs.to(self.device, torch.bfloat16).contiguous()
        if utt.dim() != 4:
            raise ValueError(f"score_resized_batch takes utt_hs [B, L, Tu, D], got {tuple(utt.shape)}")
        B, L, Tu, D = utt.shape
        if L != self.n_layers or rows.shape[0] != L or rows.shape[2] != D:
            raise ValueError(f"shape mismatch: utt {tuple(utt.shape)} keyword rows {tuple(rows.shape)}")
        K = off_host.numel() - 1
        Ho, Wo = out_size
        chunk = chunk or self.default_chunk(Ho, Wo, budget_bytes=1 << 30)
        logits = torch.empty((B, K, 2), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nb = self.lib.cbw_kws_score_resized_batch_workspace_bytes(self.h, off_host.data_ptr(), K, B, Tu, D, Ho, Wo,
                                                                      chunk)
            if nb < 0:
                _lib.check(-1, "cbw_kws_score_resized_batch_workspace_bytes")
            ws = self._ws.get(nb, self.device)
            _lib.check(self.lib.cbw_kws_score_resized_batch(self.h, utt.data_ptr(), B, Tu, rows.data_ptr(),
                                                            rows.shape[1], D, off_dev.data_ptr(), off_host.data_ptr(),
                                                            K, Ho, Wo, logits.data_ptr(), chunk, ws.data_ptr(),
                                                            ws.numel(), _lib.stream_handle()),
                       "cbw_kws_score_resized_batch")
        return logits

    def rescore_resized_batch(self, utt32: torch.Tensor, kwd32_packed, out_size: Tuple[int, int], logits: torch.Tensor,
                              sel: torch.Tensor, tier: str = "f32", trusted: bool = False) -> torch.Tensor:
        """``rescore_resized`` for a batch of segments (cbw_kws_rescore_resized_batch / _x3_batch): utt32 f32
        [B, L, Tu, D]; ``sel`` indexes the B * K pairs p = b * K + k, the rows of ``logits`` [B, K, 2], which are
        rewritten in place, every other row untouched.  A pair's logits carry the bits ``rescore_resized`` gives for
        that utterance and keyword."""
        if tier not in ("f32", "x3"):
            raise ValueError(f"unknown re-scoring tier {tier}")
        if not self.has_exact_resized:
            raise _lib.CbwError("rescore_resized_batch needs the fp32 networks: call KwsEngine.build_exact() first")
        rows, off_host, off_dev, K = self._packed_f32(kwd32_packed)
        utt = utt32.to(self.device).contiguous()
        if utt.dim() != 4:
            raise ValueError(f"rescore_resized_batch takes utt32 [B, L, Tu, D], got {tuple(utt.shape)}")
        B, L, Tu, D = utt.shape
        if utt.dtype != torch.float32 or L != self.n_layers or rows.shape[2] != D:
            raise ValueError(f"shape mismatch: utt {tuple(utt.shape)} {utt.dtype} keyword rows {tuple(rows.shape)}")
        if (tuple(logits.shape) != (B, K, 2) or logits.dtype != torch.float32 or not logits.is_contiguous()
                or logits.device != self.device):
            raise ValueError(f"rescore_resized_batch: logits must be contiguous f32 [{B}, {K}, 2] on {self.device}, "
                             f"got {tuple(logits.shape)} {logits.dtype}")
        sel = self._pair_index(sel, B * K, trusted, "sel")
        n = sel.numel()
        if n == 0:
            return logits
        Ho, Wo = out_size
        wsq, call = ((self.lib.cbw_kws_rescore_resized_workspace_bytes, self.lib.cbw_kws_rescore_resized_batch)
                     if tier == "f32" else
                     (self.lib.cbw_kws_rescore_resized_x3_workspace_bytes, self.lib.cbw_kws_rescore_resized_x3_batch))
        with torch.cuda.device(self.device):
            nb = wsq(self.h, off_host.data_ptr(), K, Tu, D, Ho, Wo)   # a pass's size does not depend on B
            if nb < 0:
                raise ValueError(f"cbw_kws_rescore_resized_batch ({tier}) workspace: bad arguments "
                                 f"(K {K}, Tu {Tu}, D {D}, out {Ho} x {Wo})")
            ws = self._ws_rescore.get(nb, self.device)
            _lib.check(call(self.h, utt.data_ptr(), B, Tu, rows.data_ptr(), rows.shape[1], D, off_dev.data_ptr(),
                            off_host.data_ptr(), K, Ho, Wo, sel.data_ptr(), n, logits.data_ptr(), ws.data_ptr(),
                            ws.numel(), _lib.stream_handle()), f"cbw_kws_rescore_resized_batch ({tier})")
        return logits

    def score_resized_batch_exact(self, utt_hs: torch.Tensor, kwd_packed_bf16, kwd_packed_f32,
                                  out_size: Tuple[int, int] = (150, 750), band: float = 0.0,
                                  band_x3: Optional[float] = 1e-4, chunk: Optional[int] = None):
        """``score_resized_exact`` for a batch of segments utt_hs [B, L, Tu, D]: one bf16 pass
        (``score_resized_batch``), one band selection over the B * K rows and one re-scoring call per tier for the
        whole batch.  Returns (logits f32 [B, K, 2], stats): row b is what ``score_resized_exact`` gives for
        utterance b, the stats are the sums over b."""
        logits = self.score_resized_batch(utt_hs, kwd_packed_bf16, out_size, chunk=chunk)
        B, K = logits.shape[0], logits.shape[1]
        stats = {"band": 0, "fp32": 0, "bf16": B * K}
        if band <= 0 or B * K == 0:
            return logits, stats
        flat = logits.view(B * K, 2)
        sel, n = self.band(flat, 0.5, band)
        stats["band"] = n
        if n == 0:
            return logits, stats
        utt32 = utt_hs.to(self.device, torch.float32)
        if band_x3 is None:
            self.rescore_resized_batch(utt32, kwd_packed_f32, out_size, logits, sel, trusted=True)
            stats["fp32"] = n
            return logits, stats
        self.rescore_resized_batch(utt32, kwd_packed_f32, out_size, logits, sel, tier="x3", trusted=True)
        sel2, n2 = self.band(flat, 0.5, band_x3)
        if n2:
            self.rescore_resized_batch(utt32, kwd_packed_f32, out_size, logits, sel2, trusted=True)
        stats["fp32"] = n2
        return logits, stats

    # ------------------------------------------------------------------ decision
    def spot(self, logits: torch.Tensor, ghost: Optional[torch.Tensor] = None, threshold: float = 0.5,
             mode: str = "threshold") -> Tuple[torch.Tensor, torch.Tensor]:
        """(prob f32 [K], sorted int64 indices) — model.py:782-813 (mode 'threshold') or
        cb_whisper.py:128 (mode 'argmax')."""
        return spot(logits, ghost, threshold, mode)


def pack_keywords(kwd_hs, device=None, dtype: torch.dtype = torch.bfloat16) -> Tuple[torch.Tensor, torch.Tensor]:
    """Ragged keyword hs (list of [L, Tk_k, D]) -> (``dtype`` [L, sum Tk, D] rows, int32 offsets [K + 1]):
    keyword k is rows off[k] .. off[k + 1] - 1 of every layer.  bf16 for ``score_resized``, torch.float32 for the
    exact tiers (``rescore_resized``)."""
    if len(kwd_hs) == 0:
        raise ValueError("no keywords")
    t = [torch.as_tensor(k) for k in kwd_hs]
    lens = torch.tensor([0] + [k.shape[1] for k in t], dtype=torch.int64)
    rows = torch.cat([k.to(device, dtype) for k in t], dim=1)
    return rows, torch.cumsum(lens, 0).to(torch.int32)


def spot(logits: torch.Tensor, ghost: Optional[torch.Tensor] = None, threshold: float = 0.5,
         mode: str = "threshold") -> Tuple[torch.Tensor, torch.Tensor]:
    lib = _lib.load()
    logits = logits.to(torch.float32).contiguous()
    K = logits.shape[0]
    dev = logits.device
    prob = torch.empty((K,), dtype=torch.float32, device=dev)
    idx = torch.empty((max(K, 1),), dtype=torch.int32, device=dev)
    n = torch.zeros((1,), dtype=torch.int32, device=dev)
    g = None if ghost is None else ghost.to(dev, torch.float32).contiguous()
    if g is not None and g.numel() != K:
        raise ValueError(f"ghost mask of {g.numel()} entries for {K} logits")
    with torch.cuda.device(dev):
        _lib.check(lib.cbw_kws_spot(logits.data_ptr(), _lib.ptr(g), K, float(threshold), 1 if mode == "argmax" else 0,
                                    prob.data_ptr(), idx.data_ptr(), n.data_ptr(), _lib.stream_handle()),
                   "cbw_kws_spot")
    return prob, idx[: int(n.item())].to(torch.int64)
