"""Exact decisions for pair lists and utterance batches: the pairs form of the two re-scoring tiers
(cbw_kws_rescore_pairs / cbw_kws_rescore_x3_pairs, KwsEngine.rescore_pairs), the band pipeline over pair lists
(KwsEngine.score_pairs_exact / score_batch_exact) and the paired batch of KWSModel.forward with the exact band on,
against the per-utterance tiers (cbw_kws_rescore / cbw_kws_rescore_x3, KwsEngine.score_exact) and the numpy oracle.

Shapes, seeded batch, PAIRS and CHUNK are those of tests/test_gpu_kws_pairs.py, restated: L = 3, B = 3 utterances of
100 feature frames, K = 5 keywords of 30 feature frames, D = 128.  Through the LEF projector Tu = 50 and Tk = 15,
neither a multiple of 16; the L engine keeps 100 x 30.  Utterance 1 has its last 13 frames masked and keyword 2 its
last 4.  The 11 pairs are unsorted and hold (2, 4) twice.  A pass of the fp32 tier holds 32 pairs, so one case runs
the list four times over (44 pairs: a full pass and a partial one starting at p0 = 32).
"""
import numpy as np
import pytest
import torch

from cbw import synth

pytestmark = pytest.mark.gpu

EXACT_RTOL = 1e-4   # tests/test_gpu_kws.py:555, the bound of test_exact_rescore_matches_reference_fp32

L, B, K, D, T_UTT, T_KWD, CHUNK = 3, 3, 5, 128, 100, 30, 4
PAIRS = [(2, 4), (0, 1), (1, 4), (0, 4), (1, 2), (2, 0), (2, 4), (0, 3), (1, 0), (2, 2), (1, 1)]
PAIR_UTT = [u for u, _ in PAIRS]
PAIR_KWD = [k for _, k in PAIRS]
P = len(PAIRS)
SUBSET = [1, 4, 6, 9]
THR = 0.5

ENGINES = {
    "LEF64-r18": dict(n_layers=L, embedding_dim=D, learn_features=True, proj_mlp=True, frames_conv=True,
                      proj_mlp_units=64, resnet_version="resnet-18"),                  # the E = 64 kernel
    "L128": dict(n_layers=L, embedding_dim=D, learn_features=False, proj_mlp=False),   # generic kernel, ResNet-50
    "LEF64-r50": dict(n_layers=L, embedding_dim=D, learn_features=True, proj_mlp=True, frames_conv=True,
                      proj_mlp_units=64, resnet_version="resnet-50"),
}
# the fp32 tier on both similarity kernels; the compensated tier on every engine, each test asking the runtime
# (cbw_kws_rescore_x3_workspace_bytes) whether it supports the engine: an unsupported one must refuse the call
TIERS = [("LEF64-r18", "fp32"), ("L128", "fp32"), ("LEF64-r50", "x3"), ("LEF64-r18", "x3"), ("L128", "x3")]


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
    """Per variant, built once and never modified: the engine, the bf16 and fp32 projections with their masks, and the
    bf16 logits of the 11 pairs."""
    if name not in _cache:
        from cbw.kws import KwsEngine
        from types import SimpleNamespace
        hp = ENGINES[name]
        eng = KwsEngine(hp, synth.synth_kws_state_dict(seed=3, **hp))
        d = eng.device
        kwd, km = torch.from_numpy(batch["kwd"]).to(d), torch.from_numpy(batch["kwd_mask"]).to(d)
        utt, um = torch.from_numpy(batch["utt"]).to(d), torch.from_numpy(batch["utt_mask"]).to(d)
        pk, pkm = eng.project(kwd, km)
        pu, pum = eng.project(utt, um)
        pk32, _ = eng.project_f32(kwd, km)
        pu32, _ = eng.project_f32(utt, um)
        if name.startswith("LEF"):
            assert tuple(pu32.shape) == (B, L, 50, 64) and tuple(pk32.shape) == (K, L, 15, 64)
        l16 = eng.score_pairs(pu, pum, pk, pkm, PAIR_UTT, PAIR_KWD, chunk=CHUNK)
        _cache[name] = SimpleNamespace(eng=eng, pu=pu, pum=pum, pk=pk, pkm=pkm, pu32=pu32, pk32=pk32, l16=l16)
    return _cache[name]


def x3_supported(s):
    return s.eng.lib.cbw_kws_rescore_x3_workspace_bytes(s.eng.h, s.pk.shape[2], s.pu.shape[2]) >= 0


def single_rows(name, tier, batch):
    """[P, 2]: row p = what the per-utterance tier (``rescore``) writes for pair p's utterance and keyword alone."""
    key = (name, tier)
    if key not in _cache:
        s = engine(name, batch)
        zero = torch.zeros(1, dtype=torch.int32, device=s.eng.device)
        rows = {}
        for u, k in set(PAIRS):
            one = torch.full((1, 2), float("nan"), device=s.eng.device)
            s.eng.rescore(s.pu32[u], s.pum[u], s.pk32[k:k + 1], s.pkm[k:k + 1], one, zero, tier=tier)
            rows[(u, k)] = one[0]
        _cache[key] = torch.stack([rows[p] for p in PAIRS])
        assert torch.isfinite(_cache[key]).all()
    return _cache[key]


def rescore_pairs(s, sel, tier="fp32", pair_utt=PAIR_UTT, pair_kwd=PAIR_KWD, start=None):
    lg = (s.l16 if start is None else start).clone()
    return s.eng.rescore_pairs(s.pu32, s.pum, s.pk32, s.pkm, pair_utt, pair_kwd, lg, sel, tier=tier)


def prob(lg):
    return torch.softmax(lg.double(), -1)[:, 1].cpu().numpy()


def split_band(p, lo, hi):
    """A band halfway between two adjacent distinct distances |p - THR|, at the widest such gap that leaves between
    lo and hi rows inside: (band, rows inside)."""
    d = np.abs(p - THR)
    ds = np.sort(d)
    gaps = [(ds[i + 1] - ds[i], i) for i in range(len(ds) - 1) if lo <= i + 1 <= hi and ds[i + 1] > ds[i]]
    assert gaps, f"no two distinct distances leave {lo}..{hi} rows inside: {ds}"
    _, i = max(gaps)
    band = 0.5 * (ds[i] + ds[i + 1])
    inside = np.nonzero(d <= band)[0]
    assert len(inside) == i + 1
    return float(band), inside


# ---------------------------------------------------------------- 1. bit identity with the per-utterance tiers
@pytest.mark.parametrize("name,tier", TIERS)
def test_rescore_pairs_bit_identical_to_per_utterance_tier(name, tier, batch):
    s = engine(name, batch)
    if tier == "x3" and not x3_supported(s):
        with pytest.raises(Exception):
            rescore_pairs(s, list(range(P)), tier)
        return
    ref = single_rows(name, tier, batch)
    dev = s.eng.device
    for sel in (list(range(P)), SUBSET):
        got = rescore_pairs(s, sel, tier)
        for p in range(P):
            if p in sel:
                assert torch.equal(got[p], ref[p]), f"{tier} pair {p} = {PAIRS[p]}: differs from the per-utterance tier"
            else:
                assert torch.equal(got[p], s.l16[p]), f"{tier} pair {p}: an unselected row was written"
        # device int32 tensors give the same result as host sequences
        dev_got = rescore_pairs(s, torch.tensor(sel, dtype=torch.int32, device=dev), tier,
                                torch.tensor(PAIR_UTT, dtype=torch.int32, device=dev),
                                torch.tensor(PAIR_KWD, dtype=torch.int32, device=dev))
        assert torch.equal(dev_got, got)
    full = rescore_pairs(s, list(range(P)), tier)
    assert torch.equal(full[0], full[6])   # the repeated pair
    assert not torch.equal(full, s.l16)    # the tier's logits are not the bf16 pass's
    print(f"{name} {tier}: largest |tier - bf16| logit {float((full - s.l16).abs().max()):.3g}")
    # an unsorted selection with the rows out of order writes the same rows
    assert torch.equal(rescore_pairs(s, SUBSET[::-1], tier), rescore_pairs(s, SUBSET, tier))


@pytest.mark.parametrize("name,tier", TIERS)
def test_cross_product_without_index_arrays(name, tier, batch):
    """None / None over the B * K pairs equals the explicit list p = b * K + k, for all pairs and for a subset, on a
    [B * K, 2] and on a [B, K, 2] logits buffer."""
    s = engine(name, batch)
    if tier == "x3" and not x3_supported(s):
        with pytest.raises(Exception):
            rescore_pairs(s, [0], tier, None, None, start=torch.zeros((B * K, 2), device=s.eng.device))
        return
    cu = [b for b in range(B) for _ in range(K)]
    ck = [k for _ in range(B) for k in range(K)]
    start = s.eng.score_batch(s.pu, s.pum, s.pk, s.pkm, chunk=CHUNK)
    for sel in (list(range(B * K)), [14, 3, 7, 8]):
        explicit = rescore_pairs(s, sel, tier, cu, ck, start=start.view(B * K, 2))
        implicit = rescore_pairs(s, sel, tier, None, None, start=start.view(B * K, 2))
        cube = rescore_pairs(s, sel, tier, None, None, start=start)
        assert torch.equal(implicit, explicit) and torch.equal(cube.view(B * K, 2), explicit)
        assert not torch.equal(explicit, start.view(B * K, 2))
    ref = single_rows(name, tier, batch)
    all_rows = rescore_pairs(s, list(range(B * K)), tier, None, None, start=start)
    for p, (u, k) in enumerate(PAIRS):
        assert torch.equal(all_rows[u, k], ref[p]), f"cross product ({u}, {k})"


@pytest.mark.parametrize("name", ["LEF64-r18", "L128"])
def test_rescore_pairs_across_a_pass_boundary(name, batch):
    """44 pairs (the list four times): the fp32 tier runs a pass of 32 and a pass of 12 from p0 = 32; a selection of
    36 of them still crosses the boundary."""
    s = engine(name, batch)
    ref = single_rows(name, "fp32", batch)
    start = s.l16.repeat(4, 1)
    for sel in (list(range(4 * P)), [i for i in range(4 * P) if i % 11 not in (3, 8)][::-1]):
        got = rescore_pairs(s, sel, "fp32", PAIR_UTT * 4, PAIR_KWD * 4, start=start)
        assert len(sel) > 32
        for i in range(4 * P):
            assert torch.equal(got[i], ref[i % P] if i in sel else start[i]), f"row {i}"


# ---------------------------------------------------------------- 2. against the oracle
@pytest.mark.parametrize("name", ["LEF64-r18", "L128"])
def test_rescore_pairs_against_numpy_oracle(name, batch):
    """Guards against the pairs form and the per-utterance tier being wrong together: every pair re-scored in fp32
    against oracle.kws's forward of that pair's utterance and keyword alone.  Measure and bound of
    tests/test_gpu_kws.py::test_exact_rescore_matches_reference_fp32: max |dlogit| / max |ref| < EXACT_RTOL."""
    import oracle.kws as okws
    hp = ENGINES[name]
    sd = synth.synth_kws_state_dict(seed=3, **hp)
    s = engine(name, batch)
    got = rescore_pairs(s, list(range(P))).cpu().numpy()
    one = {(u, k): okws.kws_forward(sd, hp, batch["kwd"][k:k + 1], batch["utt"][u:u + 1], batch["kwd_mask"][k:k + 1],
                                    batch["utt_mask"][u:u + 1], return_features=False)[0] for u, k in set(PAIRS)}
    ref = np.concatenate([one[p] for p in PAIRS])
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{name}: fp32 rescore_pairs max|dlogit|/max|logit| = {err:.2e} (bound {EXACT_RTOL:.0e})")
    assert err < EXACT_RTOL, f"fp32 rescore_pairs deviates {err:.2e}"


# ---------------------------------------------------------------- 3. band semantics
@pytest.mark.parametrize("name", ["LEF64-r18", "L128", "LEF64-r50"])
def test_score_pairs_exact_band(name, batch):
    s = engine(name, batch)
    band, inside = split_band(prob(s.l16), 1, P - 1)
    n_in = len(inside)
    assert 0 < n_in < P
    print(f"{name}: band {band:.6g} holds {n_in} of {P} pairs: {inside.tolist()}")
    want = rescore_pairs(s, inside.tolist())
    got, stats = s.eng.score_pairs_exact(s.pu, s.pum, s.pk, s.pkm, s.pu32, s.pk32, PAIR_UTT, PAIR_KWD, THR, band,
                                         chunk=CHUNK)
    assert stats == {"band": n_in, "fp32": n_in, "bf16": P}
    for p in range(P):
        if p in inside:
            assert torch.equal(got[p], want[p]) and torch.equal(got[p], single_rows(name, "fp32", batch)[p])
        else:
            assert torch.equal(got[p], s.l16[p]), f"pair {p} outside the band must keep its bf16 logits"
    # band 0: the bf16 pass alone; logits_out and features are honoured
    buf = torch.full((P, 2), float("nan"), device=s.eng.device)
    out, st0, feats = s.eng.score_pairs_exact(s.pu, s.pum, s.pk, s.pkm, s.pu32, s.pk32, PAIR_UTT, PAIR_KWD, THR, 0.0,
                                              chunk=CHUNK, logits_out=buf, features=True)
    assert out is buf and torch.equal(buf, s.l16) and st0 == {"band": 0, "fp32": 0, "bf16": P}
    assert torch.equal(feats, s.eng.score_pairs(s.pu, s.pum, s.pk, s.pkm, PAIR_UTT, PAIR_KWD, chunk=CHUNK,
                                                features=True)[1])


@pytest.mark.parametrize("name", list(ENGINES))
def test_score_pairs_exact_two_tiers(name, batch):
    """With band_x3 the band's pairs go to the compensated tier, and stats["fp32"] counts only those still inside
    band_x3, which end with the fp32 tier's logits."""
    s = engine(name, batch)
    if not x3_supported(s):
        with pytest.raises(Exception):
            s.eng.score_pairs_exact(s.pu, s.pum, s.pk, s.pkm, s.pu32, s.pk32, PAIR_UTT, PAIR_KWD, THR, 1.0,
                                    chunk=CHUNK, band_x3=1e-4)
        return
    band, inside = split_band(prob(s.l16), 3, P - 1)   # >= 3 rows: at least two distinct pairs (rows 0 and 6 are one)
    x3 = rescore_pairs(s, inside.tolist(), "x3")
    band_x3, in3 = split_band(prob(x3)[inside], 1, len(inside) - 1)
    in3 = inside[in3]
    assert 0 < len(in3) < len(inside) < P
    print(f"{name}: band {band:.6g} holds {inside.tolist()}, band_x3 {band_x3:.6g} holds {in3.tolist()}")
    want = rescore_pairs(s, in3.tolist(), "fp32", start=x3)
    got, stats = s.eng.score_pairs_exact(s.pu, s.pum, s.pk, s.pkm, s.pu32, s.pk32, PAIR_UTT, PAIR_KWD, THR, band,
                                         chunk=CHUNK, band_x3=band_x3)
    assert stats == {"band": len(inside), "fp32": len(in3), "bf16": P}
    assert torch.equal(got, want)
    f32, x3_rows = single_rows(name, "fp32", batch), single_rows(name, "x3", batch)
    for p in range(P):
        assert torch.equal(got[p], f32[p] if p in in3 else x3_rows[p] if p in inside else s.l16[p]), f"pair {p}"


def test_score_pairs_exact_ghost_mask(batch):
    """A per-keyword ghost mask: a pair is selected exactly when ``band`` selects its keyword in the single-utterance
    call of its utterance; none of the zeroed keyword's pairs is."""
    name = "LEF64-r18"
    s = engine(name, batch)
    ghost = torch.ones(K, device=s.eng.device)
    ghost[4] = 0.0
    band = 0.49   # the zeroed keyword's probability is 0: |0 - 0.5| > band
    chosen = []
    for u in range(B):
        idx, _ = s.eng.band(s.eng.score(s.pu[u], s.pum[u], s.pk, s.pkm, chunk=CHUNK), THR, band, ghost)
        chosen.append(set(idx.cpu().tolist()))
    inside = [p for p, (u, k) in enumerate(PAIRS) if k in chosen[u]]
    assert 0 < len(inside) < P and all(PAIR_KWD[p] != 4 for p in inside)
    got, stats = s.eng.score_pairs_exact(s.pu, s.pum, s.pk, s.pkm, s.pu32, s.pk32, PAIR_UTT, PAIR_KWD, THR, band,
                                         ghost=ghost, chunk=CHUNK)
    assert stats["band"] == len(inside) and stats["fp32"] == len(inside)
    assert torch.equal(got, rescore_pairs(s, inside))
    for p in range(P):
        if PAIR_KWD[p] == 4:
            assert torch.equal(got[p], s.l16[p])
    with pytest.raises(ValueError):   # the ghost mask is per keyword
        s.eng.score_pairs_exact(s.pu, s.pum, s.pk, s.pkm, s.pu32, s.pk32, PAIR_UTT, PAIR_KWD, THR, band,
                                ghost=torch.ones(P, device=s.eng.device), chunk=CHUNK)


# ---------------------------------------------------------------- 4. batch form
@pytest.mark.parametrize("name,two_tiers", [("LEF64-r18", False), ("L128", False), ("LEF64-r50", True),
                                            ("LEF64-r18", True)])
def test_score_batch_exact_equals_stacked_score_exact(name, two_tiers, batch):
    s = engine(name, batch)
    if two_tiers and not x3_supported(s):
        with pytest.raises(Exception):
            s.eng.score_batch_exact(s.pu, s.pum, s.pk, s.pkm, s.pu32, s.pk32, THR, 1.0, chunk=CHUNK, band_x3=1e-4)
        return
    l16 = s.eng.score_batch(s.pu, s.pum, s.pk, s.pkm, chunk=CHUNK).view(B * K, 2)
    band, inside = split_band(prob(l16), 4, B * K - 1)   # >= 4 pairs: more than the ghosted keyword's B = 3
    band_x3 = None
    if two_tiers:
        x3 = rescore_pairs(s, inside.tolist(), "x3", None, None, start=l16)
        band_x3, in3 = split_band(prob(x3)[inside], 1, len(inside) - 1)
    ghost = torch.ones(K, device=s.eng.device)
    ghost[1] = 0.0
    for g in (None, ghost):
        singles = [s.eng.score_exact(s.pu[b], s.pum[b], s.pk, s.pkm, s.pu32[b], s.pk32, THR, band, ghost=g,
                                     chunk=CHUNK, band_x3=band_x3) for b in range(B)]
        ref = torch.stack([lg for lg, _ in singles])
        ref_stats = {key: sum(st[key] for _, st in singles) for key in ("band", "fp32", "bf16")}
        got, stats = s.eng.score_batch_exact(s.pu, s.pum, s.pk, s.pkm, s.pu32, s.pk32, THR, band, ghost=g, chunk=CHUNK,
                                             band_x3=band_x3)
        print(f"{name} two_tiers={two_tiers} ghost={g is not None}: band {band:.6g}, band_x3 {band_x3}, {stats}")
        assert tuple(got.shape) == (B, K, 2) and torch.equal(got, ref)
        assert stats == ref_stats and 0 < stats["band"] < B * K and stats["bf16"] == B * K
        if g is None:
            assert stats["band"] == len(inside)
            if two_tiers:
                assert stats["fp32"] == len(in3) and 0 < len(in3) < len(inside)
        buf = torch.full((B, K, 2), float("nan"), device=s.eng.device)
        out, _ = s.eng.score_batch_exact(s.pu, s.pum, s.pk, s.pkm, s.pu32, s.pk32, THR, band, ghost=g, chunk=CHUNK,
                                         band_x3=band_x3, logits_out=buf)
        assert out is buf and torch.equal(buf, ref)
    assert not torch.equal(ref.view(B * K, 2), l16)


# ---------------------------------------------------------------- 5. model
def test_kwsmodel_forward_paired_batch_exact(batch):
    """utt batch == n_keywords with the exact band on: pair i = (utterance i, keyword i) in one call equals the K
    single-pair forwards bit for bit -- fp32-tier logits, where the paired branch returned the bf16 pass's."""
    from efficient_kws.model import KWSModel
    hp = ENGINES["LEF64-r18"]
    sd = synth.synth_kws_state_dict(seed=3, **hp)
    m = KWSModel(features_size=(T_KWD, T_UTT), exact_band=1.0, **hp)
    m.load_state_dict(sd)
    sel = [0, 1, 2, 1, 0]
    kwd, km = torch.from_numpy(batch["kwd"]), torch.from_numpy(batch["kwd_mask"])
    utt, um = torch.from_numpy(batch["utt"][sel]), torch.from_numpy(batch["utt_mask"][sel])
    labels = torch.tensor([1, 0, 0, 1, 0])
    out = m.forward(kwd_features=kwd, utt_features=utt, labels=labels, kwd_mask=km, utt_mask=um, return_features=True)
    assert tuple(out.logits.shape) == (K, 2) and tuple(out.features.shape) == (K, L, 15, 50)
    singles = [m.forward(kwd_features=kwd[i:i + 1], utt_features=utt[i:i + 1], kwd_mask=km[i:i + 1],
                         utt_mask=um[i:i + 1], return_features=True) for i in range(K)]
    ref_l = torch.cat([x.logits for x in singles])
    assert torch.equal(out.logits, ref_l)
    assert torch.equal(out.features, torch.cat([x.features for x in singles]))   # the bf16 pass's maps
    assert torch.equal(out.loss, torch.nn.functional.cross_entropy(ref_l, labels.to(ref_l.device)))
    assert out.loss_alt["loss_resnet"] is out.loss
    m0 = KWSModel(features_size=(T_KWD, T_UTT), exact_band=0.0, **hp)
    m0.load_state_dict(sd)
    out0 = m0.forward(kwd_features=kwd, utt_features=utt, kwd_mask=km, utt_mask=um, return_features=True)
    assert not torch.equal(out.logits, out0.logits)
    assert torch.equal(out.features, out0.features)
    print(f"largest |exact - bf16| paired logit: {float((out.logits - out0.logits).abs().max()):.3g}")
    out2 = m.forward(kwd_features=kwd, utt_features=utt, kwd_mask=km, utt_mask=um, return_features=False)
    assert out2.features is None and out2.loss is None and torch.equal(out2.logits, ref_l)


def test_kwsmodel_forward_paired_batch_auto_band(batch):
    """exact_band="auto": the paired branch calibrates on the first utterance of the batch as the one-utterance
    branch does, and the K single-pair forwards on the calibrated model then give the same logits."""
    from efficient_kws.model import KWSModel
    hp = ENGINES["LEF64-r18"]
    m = KWSModel(features_size=(T_KWD, T_UTT), **hp)
    m.load_state_dict(synth.synth_kws_state_dict(seed=3, **hp))
    sel = [0, 1, 2, 1, 0]
    kwd, km = torch.from_numpy(batch["kwd"]), torch.from_numpy(batch["kwd_mask"])
    utt, um = torch.from_numpy(batch["utt"][sel]), torch.from_numpy(batch["utt_mask"][sel])
    assert m.band_calibration is None
    out = m.forward(kwd_features=kwd, utt_features=utt, kwd_mask=km, utt_mask=um, return_features=False)
    assert m.band_calibration is not None and m.band_calibration["held_out_pairs"] == K
    assert m.exact_band == m.band_calibration["band"] > 0
    singles = [m.forward(kwd_features=kwd[i:i + 1], utt_features=utt[i:i + 1], kwd_mask=km[i:i + 1],
                         utt_mask=um[i:i + 1], return_features=False) for i in range(K)]
    assert torch.equal(out.logits, torch.cat([x.logits for x in singles]))


# ---------------------------------------------------------------- 6. arguments
def test_argument_handling(batch):
    """Host checks only: nothing here reaches a kernel with a bad index."""
    from cbw import _lib
    s = engine("LEF64-r18", batch)
    eng, lib = s.eng, s.eng.lib
    dev = eng.device
    sentinel = 123.0
    logits = torch.full((P, 2), sentinel, device=dev)

    def rp(pair_utt=PAIR_UTT, pair_kwd=PAIR_KWD, sel=(0, 1), lg=logits, utt32=s.pu32, kwd32=s.pk32, **kw):
        return eng.rescore_pairs(utt32, s.pum, kwd32, s.pkm, pair_utt, pair_kwd, lg, list(sel), **kw)

    bad_u, bad_k = list(PAIR_UTT), list(PAIR_KWD)
    bad_u[3], bad_k[5] = B, -1
    for kw in (dict(pair_utt=bad_u), dict(pair_kwd=bad_k), dict(sel=(0, P)), dict(sel=(-1,)),
               dict(pair_utt=PAIR_UTT[:-1]),                       # index lengths differ
               dict(pair_utt=None), dict(pair_kwd=None),           # exactly one index array
               dict(pair_utt=None, pair_kwd=None),                 # cross product: logits of P != B * K rows
               dict(sel=list(range(P)) + [0]),                     # more selections than pairs
               dict(utt32=s.pu, kwd32=s.pk),                       # bf16 where the fp32 projections are expected
               dict(utt32=s.pu32[0]),                              # one utterance without the batch axis
               dict(lg=logits[:P - 1]), dict(lg=logits.double()),  # logits rows / dtype
               dict(tier="fp16")):
        with pytest.raises(ValueError):
            rp(**kw)
    with pytest.raises(ValueError):
        rp(pair_utt=torch.tensor(bad_u, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        eng.score_pairs_exact(s.pu, s.pum, s.pk, s.pkm, s.pu32, s.pk32, bad_u, PAIR_KWD, THR, 1.0, chunk=CHUNK)
    with pytest.raises(ValueError):   # bf16 where the fp32 projections are expected, found by the re-scoring step
        eng.score_pairs_exact(s.pu, s.pum, s.pk, s.pkm, s.pu, s.pk, PAIR_UTT, PAIR_KWD, THR, 1.0, chunk=CHUNK)
    with pytest.raises(ValueError):
        eng.score_batch_exact(s.pu32, s.pum, s.pk32, s.pkm, s.pu32, s.pk32, THR, 1.0, chunk=CHUNK)
    # nothing to do: untouched or empty results, no launch
    assert rp(sel=()) is logits
    assert tuple(rp(pair_utt=[], pair_kwd=[], sel=(), lg=logits[:0]).shape) == (0, 2)
    out, stats = eng.score_pairs_exact(s.pu, s.pum, s.pk, s.pkm, s.pu32, s.pk32, [], [], THR, 1.0, chunk=CHUNK)
    assert tuple(out.shape) == (0, 2) and stats == {"band": 0, "fp32": 0, "bf16": 0}
    torch.cuda.synchronize()
    assert bool((logits == sentinel).all())

    # the C ABI's own checks, both tiers
    Tk, Tu = s.pk32.shape[2], s.pu32.shape[2]
    idx = torch.zeros(P, dtype=torch.int32, device=dev)
    for fn, wsq in ((lib.cbw_kws_rescore_pairs, lib.cbw_kws_rescore_workspace_bytes),
                    (lib.cbw_kws_rescore_x3_pairs, lib.cbw_kws_rescore_x3_workspace_bytes)):
        nb = wsq(eng.h, Tk, Tu)
        assert nb > 0
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        big = torch.full((B * K, 2), sentinel, device=dev)

        def call(pair_u, pair_k, n_pairs, n_sel, b=B, lg=logits):
            return fn(eng.h, s.pu32.data_ptr(), s.pum.data_ptr(), b, s.pk32.data_ptr(), s.pkm.data_ptr(), K, Tk, Tu,
                      pair_u, pair_k, n_pairs, idx.data_ptr(), n_sel, lg.data_ptr(), ws.data_ptr(), ws.numel(),
                      _lib.stream_handle())

        assert call(idx.data_ptr(), idx.data_ptr(), 4, 5) == -1                   # n_sel > P
        assert b"n_sel" in lib.cbw_last_error()
        for pair_u, pair_k in ((idx.data_ptr(), None), (None, idx.data_ptr())):   # exactly one index array
            assert call(pair_u, pair_k, 4, 2) == -1
            assert b"pair_utt and pair_kwd" in lib.cbw_last_error()
        assert call(None, None, B * K - 1, 2, lg=big) == -1                       # cross product of the wrong size
        assert b"B * K" in lib.cbw_last_error()
        assert call(idx.data_ptr(), idx.data_ptr(), 4, 2, b=0) == -1 and lib.cbw_last_error()
        assert call(idx.data_ptr(), idx.data_ptr(), 4, 0) == 0                    # n_sel = 0: CBW_OK, nothing written
        assert call(idx.data_ptr(), idx.data_ptr(), 0, 0) == 0                    # P = 0
        assert call(None, None, 0, 0) == 0
        torch.cuda.synchronize()
        assert bool((logits == sentinel).all()) and bool((big == sentinel).all())
        assert call(None, None, B * K, 1, lg=big) == 0                            # and a valid call still runs: pair 0
        torch.cuda.synchronize()
        assert torch.isfinite(big).all() and not bool((big[0] == sentinel).any()) and bool((big[1:] == sentinel).all())
