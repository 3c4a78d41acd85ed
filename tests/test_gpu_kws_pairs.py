"""Pair lists and utterance batches in one pass (cbw_kws_score_pairs, KwsEngine.score_pairs / score_batch, the
paired batch of KWSModel.forward) against the single-utterance path (cbw_kws_score) and the numpy oracle.

Shapes: L = 3, B = 3 utterances of 100 feature frames, K = 5 keywords of 30 feature frames, D = 128.  Through the
LEF projector Tu = 50 and Tk = 15: neither a multiple of the 16-frame tile, both above the ABI minimum of 7; the
LE and L engines keep 100 x 30 (7 and 2 tiles, both with a tail).  chunk = 4, so a chunk boundary falls inside an
utterance.  Utterance 1 has its last 13 frames masked and keyword 2 its last 4.
"""
import ctypes

import numpy as np
import pytest
import torch

from cbw import synth

pytestmark = pytest.mark.gpu

LOGIT_RTOL = 2e-2   # tests/test_gpu_kws.py:21, used as atol = LOGIT_RTOL * max|ref| by its LEF parity test (:107)

L, B, K, D, T_UTT, T_KWD, CHUNK = 3, 3, 5, 128, 100, 30, 4
# 11 pairs, unsorted, (2, 4) twice, every utterance used, keyword 4 with all three utterances;
# chunks of 4: [0:4] and [4:8] mix utterances, the tail chunk holds 3 pairs
PAIRS = [(2, 4), (0, 1), (1, 4), (0, 4), (1, 2), (2, 0), (2, 4), (0, 3), (1, 0), (2, 2), (1, 1)]
PAIR_UTT = [u for u, _ in PAIRS]
PAIR_KWD = [k for _, k in PAIRS]

ENGINES = {
    "LEF64-r18": dict(n_layers=L, embedding_dim=D, learn_features=True, proj_mlp=True, frames_conv=True,
                      proj_mlp_units=64, resnet_version="resnet-18"),
    "LE64-r18": dict(n_layers=L, embedding_dim=D, learn_features=True, proj_mlp=True, frames_conv=False,
                     proj_mlp_units=64, resnet_version="resnet-18"),
    # E = 32, the row-strip kernel's other instantiation: cbw_kws_create accepts proj_mlp_units = 64 only, so the
    # width is reached with raw 32-wide hs (the first 32 dims of the features, renormalised; ResNet-50)
    "L32": dict(n_layers=L, embedding_dim=32, learn_features=False, proj_mlp=False),
    "L128": dict(n_layers=L, embedding_dim=D, learn_features=False, proj_mlp=False),   # generic kernel, ResNet-50
    "LEF64-r50": dict(n_layers=L, embedding_dim=D, learn_features=True, proj_mlp=True, frames_conv=True,
                      proj_mlp_units=64, resnet_version="resnet-50"),
}


@pytest.fixture(scope="module")
def batch():
    """Seeded features in the dataset contract (L2-normalised frames, 0/1 masks), shared and never modified."""
    g = np.random.Generator(np.random.PCG64(77))
    utt = synth.l2n(g.standard_normal((B, L, T_UTT, D)).astype(np.float32))
    kwd = synth.l2n(g.standard_normal((K, L, T_KWD, D)).astype(np.float32))
    # keyword 4 also sits in utterance 0 (with noise), so one pair carries a diagonal
    utt[0, :, 20:20 + T_KWD] = synth.l2n(kwd[4] + 0.3 * g.standard_normal((L, T_KWD, D)).astype(np.float32))
    utt_mask = np.ones((B, L, T_UTT), np.float32)
    kwd_mask = np.ones((K, L, T_KWD), np.float32)
    utt_mask[1, :, -13:] = 0.0
    utt[1, :, -13:] = 0.0
    kwd_mask[2, :, -4:] = 0.0
    kwd[2, :, -4:] = 0.0
    return dict(utt=utt, utt_mask=utt_mask, kwd=kwd, kwd_mask=kwd_mask)


_cache = {}


def engine(name, batch):
    """(engine, projected utt [B, L, Tu, E], utt mask, projected kwd, kwd mask), built once per variant."""
    if name not in _cache:
        from cbw.kws import KwsEngine
        hp = ENGINES[name]
        eng = KwsEngine(hp, synth.synth_kws_state_dict(seed=3, **hp))
        d = eng.device
        kwd, utt = batch["kwd"], batch["utt"]
        if hp["embedding_dim"] != D:
            kwd, utt = (np.ascontiguousarray(synth.l2n(x[..., :hp["embedding_dim"]])) for x in (kwd, utt))
        pk, pkm = eng.project(torch.from_numpy(kwd).to(d), torch.from_numpy(batch["kwd_mask"]).to(d))
        pu, pum = eng.project(torch.from_numpy(utt).to(d), torch.from_numpy(batch["utt_mask"]).to(d))
        _cache[name] = (eng, pu, pum, pk, pkm)
    return _cache[name]


@pytest.mark.parametrize("name", list(ENGINES))
def test_pair_list_bit_identical_to_single_utterance_path(name, batch):
    """Every pair's logits and similarity maps equal what ``score`` gives for that utterance and that keyword alone,
    bit for bit: row-strip kernel at E = 64 and E = 32, generic kernel at E = 128."""
    eng, pu, pum, pk, pkm = engine(name, batch)
    if name.startswith("LEF"):
        assert tuple(pu.shape) == (B, L, 50, 64) and tuple(pk.shape) == (K, L, 15, 64)
    logits, feats = eng.score_pairs(pu, pum, pk, pkm, PAIR_UTT, PAIR_KWD, chunk=CHUNK, features=True)
    assert tuple(logits.shape) == (len(PAIRS), 2) and tuple(feats.shape) == (len(PAIRS), L) + (pk.shape[2], pu.shape[2])
    # device int32 index tensors give the same result as host sequences
    lg2 = eng.score_pairs(pu, pum, pk, pkm, torch.tensor(PAIR_UTT, dtype=torch.int32, device=eng.device),
                          torch.tensor(PAIR_KWD, dtype=torch.int32, device=eng.device), chunk=CHUNK)
    assert torch.equal(lg2, logits)
    refs = [eng.score(pu[u], pum[u], pk[k:k + 1], pkm[k:k + 1], features=True, chunk=CHUNK) for u, k in PAIRS]
    ref_l = torch.cat([r[0] for r in refs])
    ref_f = torch.cat([r[1] for r in refs])
    print(f"{name}: largest |score_pairs - score|: logits {float((logits - ref_l).abs().max()):.3g}, "
          f"maps {float((feats - ref_f).abs().max()):.3g}")
    for p, (u, k) in enumerate(PAIRS):
        assert torch.equal(feats[p], ref_f[p]), f"pair {p} = ({u}, {k}): similarity maps differ"
        assert torch.equal(logits[p], ref_l[p]), f"pair {p} = ({u}, {k}): logits differ"
    assert torch.equal(logits[0], logits[6])   # the repeated pair
    assert torch.isfinite(logits).all()
    # the masked frames are zero in the maps: utterance 1's last 13 feature frames, keyword 2's last 4
    p12 = PAIRS.index((1, 2))
    tu0 = feats.shape[3] - (6 if name.startswith("LEF") else 13)
    tk0 = feats.shape[2] - (1 if name.startswith("LEF") else 4)
    assert float(feats[p12, :, :, tu0:].abs().max()) == 0.0 and float(feats[p12, :, tk0:, :].abs().max()) == 0.0
    assert float(feats[p12, :, :tk0, :tu0].abs().max()) > 0.0


@pytest.mark.parametrize("name", ["LEF64-r18", "L128"])
def test_batch_form_equals_stacked_score_calls(name, batch):
    eng, pu, pum, pk, pkm = engine(name, batch)
    out = eng.score_batch(pu, pum, pk, pkm, chunk=CHUNK)
    assert tuple(out.shape) == (B, K, 2)
    ref = torch.stack([eng.score(pu[b], pum[b], pk, pkm, chunk=CHUNK) for b in range(B)])
    assert torch.equal(out, ref)
    buf = torch.full((B, K, 2), float("nan"), device=eng.device)
    assert eng.score_batch(pu, pum, pk, pkm, chunk=CHUNK, logits_out=buf) is buf and torch.equal(buf, ref)


def test_pair_list_against_numpy_oracle(batch):
    """Guards against the pair path and ``score`` being wrong together: each pair against oracle.kws's forward of
    that pair's utterance and keyword alone.  Tolerance: that of the LEF parity test of tests/test_gpu_kws.py
    (:107), atol = LOGIT_RTOL * max|ref| with the maximum over the logits the test checks (there the K keywords'
    of one call, here the 11 pairs'): the bf16 error scales with the network's activations, not with one pair's
    logit, which may lie near zero."""
    import oracle.kws as okws
    name = "LEF64-r18"
    hp = ENGINES[name]
    sd = synth.synth_kws_state_dict(seed=3, **hp)
    eng, pu, pum, pk, pkm = engine(name, batch)
    logits = eng.score_pairs(pu, pum, pk, pkm, PAIR_UTT, PAIR_KWD, chunk=CHUNK).cpu().numpy()
    ref = np.concatenate([okws.kws_forward(sd, hp, batch["kwd"][k:k + 1], batch["utt"][u:u + 1],
                                           batch["kwd_mask"][k:k + 1], batch["utt_mask"][u:u + 1],
                                           return_features=False)[0] for u, k in PAIRS])
    print(f"max |gpu - oracle| = {np.abs(logits - ref).max():.3g}, bound {LOGIT_RTOL * np.abs(ref).max():.3g}")
    np.testing.assert_allclose(logits, ref, atol=LOGIT_RTOL * np.abs(ref).max(), rtol=0)


def test_kwsmodel_forward_paired_batch(batch):
    """utt batch == n_keywords (model.py:171-184): pair i = (utterance i, keyword i) in one call equals the K
    single-pair forwards.  exact_band = 0: the fp32 re-scoring of near-threshold pairs exists for the
    one-utterance shape only, and this test compares the bf16 passes."""
    from efficient_kws.model import KWSModel
    hp = ENGINES["LEF64-r18"]
    m = KWSModel(features_size=(T_KWD, T_UTT), exact_band=0.0, **hp)
    m.load_state_dict(synth.synth_kws_state_dict(seed=3, **hp))
    sel = [0, 1, 2, 1, 0]
    kwd, km = torch.from_numpy(batch["kwd"]), torch.from_numpy(batch["kwd_mask"])
    utt, um = torch.from_numpy(batch["utt"][sel]), torch.from_numpy(batch["utt_mask"][sel])
    labels = torch.tensor([1, 0, 0, 1, 0])
    out = m.forward(kwd_features=kwd, utt_features=utt, labels=labels, kwd_mask=km, utt_mask=um, return_features=True)
    assert tuple(out.logits.shape) == (K, 2) and tuple(out.features.shape) == (K, L, 15, 50)
    singles = [m.forward(kwd_features=kwd[i:i + 1], utt_features=utt[i:i + 1], kwd_mask=km[i:i + 1],
                         utt_mask=um[i:i + 1], return_features=True) for i in range(K)]
    ref_l = torch.cat([s.logits for s in singles])
    assert torch.equal(out.logits, ref_l)
    assert torch.equal(out.features, torch.cat([s.features for s in singles]))
    assert torch.equal(out.loss, torch.nn.functional.cross_entropy(ref_l, labels.to(ref_l.device)))
    assert out.loss_alt["loss_resnet"] is out.loss
    out2 = m.forward(kwd_features=kwd, utt_features=utt, kwd_mask=km, utt_mask=um, return_features=False)
    assert out2.features is None and out2.loss is None and torch.equal(out2.logits, ref_l)
    with pytest.raises(ValueError):
        m.forward(kwd_features=kwd, utt_features=utt[:2], kwd_mask=km, utt_mask=um[:2])


def test_score_checks_mask_shapes(batch):
    """``score`` refuses a mask that does not cover its features before anything is launched (the kernel would read
    past its end), and takes the utterance with or without the batch axis of 1."""
    eng, pu, pum, pk, pkm = engine("LEF64-r18", batch)
    Tk, Tu = pk.shape[2], pu.shape[2]
    sentinel = 123.0
    buf = torch.full((K, 2), sentinel, device=eng.device)
    with pytest.raises(ValueError):   # kwd_mask [K, L, Tk - 1]
        eng.score(pu[0], pum[0], pk, pkm[:, :, :Tk - 1], chunk=CHUNK, logits_out=buf)
    for bad in (pum[0][:, :Tu - 1], pum[:2], pum[0].reshape(-1)[:L * Tu - 1]):   # not L * Tu elements
        with pytest.raises(ValueError):
            eng.score(pu[0], bad, pk, pkm, chunk=CHUNK, logits_out=buf)
    torch.cuda.synchronize()
    assert bool((buf == sentinel).all())
    ref = eng.score(pu[0], pum[0], pk, pkm, chunk=CHUNK)
    assert tuple(pu[:1].shape) == (1, L, Tu, 64) and tuple(pum[:1].shape) == (1, L, Tu)
    assert torch.equal(eng.score(pu[:1], pum[:1], pk, pkm, chunk=CHUNK), ref)
    assert torch.equal(eng.score(pu[0], pum[0].reshape(-1), pk, pkm, chunk=CHUNK), ref)   # L * Tu elements: reshaped
    assert torch.isfinite(ref).all()


def test_argument_handling(batch):
    from cbw import _lib
    eng, pu, pum, pk, pkm = engine("LEF64-r18", batch)
    lib = eng.lib
    # index ranges are checked on the host before any launch (the device clamp is never exercised here)
    for bad_u, bad_k in (([0, B], [0, 1]), ([0, 1], [K, 0]), ([-1, 0], [0, 1]), ([0, 1], [0, -1])):
        with pytest.raises(ValueError):
            eng.score_pairs(pu, pum, pk, pkm, bad_u, bad_k, chunk=CHUNK)
    with pytest.raises(ValueError):
        eng.score_pairs(pu, pum, pk, pkm, torch.tensor([0, B], dtype=torch.int32, device=eng.device),
                        torch.tensor([0, 1], dtype=torch.int32, device=eng.device), chunk=CHUNK)
    with pytest.raises(ValueError):   # lengths differ
        eng.score_pairs(pu, pum, pk, pkm, [0, 1], [0], chunk=CHUNK)
    with pytest.raises(ValueError):   # one utterance without the batch axis
        eng.score_pairs(pu[0], pum[0], pk, pkm, [0], [0], chunk=CHUNK)
    with pytest.raises(ValueError):   # fp32 features
        eng.score_batch(pu.float(), pum, pk, pkm, chunk=CHUNK)
    # an empty pair list: empty logits, no launch
    out = eng.score_pairs(pu, pum, pk, pkm, [], [], chunk=CHUNK)
    assert tuple(out.shape) == (0, 2)

    # the C ABI's own checks
    Tk, Tu = pk.shape[2], pu.shape[2]
    idx = torch.zeros(4, dtype=torch.int32, device=eng.device)
    sentinel = 123.0
    logits = torch.full((B * K, 2), sentinel, device=eng.device)
    ws = eng.workspace(Tk, Tu, CHUNK)

    def call(pair_u, pair_k, P, b=B):
        return lib.cbw_kws_score_pairs(eng.h, pu.data_ptr(), pum.data_ptr(), b, pk.data_ptr(), pkm.data_ptr(), K, Tk,
                                       Tu, pair_u, pair_k, P, logits.data_ptr(), None, CHUNK, ws.data_ptr(),
                                       ws.numel(), _lib.stream_handle())

    for pair_u, pair_k in ((idx.data_ptr(), None), (None, idx.data_ptr())):   # exactly one index array
        assert call(pair_u, pair_k, 4) == -1
        assert b"pair_utt and pair_kwd" in lib.cbw_last_error()
    assert call(None, None, B * K - 1) == -1                                  # cross product of the wrong size
    assert b"B * K" in lib.cbw_last_error()
    assert call(idx.data_ptr(), idx.data_ptr(), -1) == -1 and lib.cbw_last_error()
    assert call(idx.data_ptr(), idx.data_ptr(), 4, b=0) == -1 and lib.cbw_last_error()
    assert call(idx.data_ptr(), idx.data_ptr(), 0) == 0                       # P = 0: CBW_OK, nothing written
    assert call(None, None, 0) == 0
    torch.cuda.synchronize()
    assert bool((logits == sentinel).all())
    assert ctypes.c_int(call(None, None, B * K)).value == 0                   # and the valid call still runs
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all() and not bool((logits == sentinel).any())
