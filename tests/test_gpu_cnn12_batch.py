"""A batch of segments on CB-Whisper's own 12-channel spotter in one pass (model/cb_whisper.py:87-129: keyword_spotting
receives [S, n_mel, 3000] and scores every segment against every keyword): the bf16 similarity-rows kernel
(sim_rows_bf16_kernel) against float64, the bit-identity of cbw_kws_score_resized_batch and of the two exact tiers'
batch entry points with the per-utterance calls, the cascade (KwsEngine.score_resized_batch_exact,
KWSModel.spot_keywords_batch) and CBWhisper's cnn path with two segments in one call.

Tolerance of the rows kernel, ROWS_TOL(D) = 1.01 (D + 8) 2^-24 against float64 on the bf16-rounded inputs: bf16
products are exact in fp32; frames are unit vectors up to bf16 rounding, so sum |a_i b_i| <= (1 + 2^-8)^2 = 1.0078;
fp32 summation in any order errs by at most (D - 1) 2^-24 times that: tests/test_gpu_cnn12_exact.py's sim_tol(D) with
the rounding of the norms added.  Everything else here is equality of bits.

Measured on MI355X (this file's prints): see docs/MEASUREMENT_LOG.md, "A batch of segments on the 12-channel spotter".
"""
import numpy as np
import pytest
import torch

from cbw import synth
from test_gpu_cnn12_exact import BAND48, BAND_X3, D48, K48, SIZE48, TU48, L, build, cnn12_engine, cnn12_sd
from test_gpu_cnn12_exact import case48, planted  # noqa: F401  (fixtures: inputs48()'s keywords, weights, bias shift)

pytestmark = pytest.mark.gpu

TK = [1, 9, 65, 171, 130]          # a sub-tile run, two-tile runs, runs that end mid-tile (K = 5, 376 rows)
B = 3
RANGES = [(0, 15), (3, 4), (4, 7), (14, 1)]   # the whole batch, across a boundary, splitting two, the last pair


def rows_tol(D):
    return 1.01 * (D + 8) * 2.0 ** -24


def bf16_round(x):
    return torch.from_numpy(x).to(torch.bfloat16)


def batch_inputs(D, Tu, seed):
    """B unit-norm utterances and the TK keywords, rounded to bf16 (torch tensors), keyword 2 planted in utterance 1."""
    g = np.random.default_rng(seed)
    utt = synth.l2n(g.standard_normal((B, L, Tu, D)).astype(np.float32))
    kwd = [synth.l2n(g.standard_normal((L, T, D)).astype(np.float32)) for T in TK]
    kwd[2][:, 5:35] = utt[1][:, 60:90]          # a planted match: similarities up to 1
    return bf16_round(utt), [bf16_round(k) for k in kwd]


@pytest.mark.parametrize("D,Tu", [(64, 130), (128, 300), (1280, 130)])
def test_similarity_rows_bf16_vs_float64(D, Tu):
    """cbw_kws_sim_rows_bf16 for four pair ranges against oracle.cnn12.sim_matrices in float64 on the same bf16-rounded
    values; everything outside a pair's [Tk][Tu] block, columns >= Tu included, stays unwritten."""
    import oracle.cnn12 as oc
    from cbw import _lib
    from cbw.kws import pack_keywords
    lib = _lib.load()
    d = torch.device("cuda:0")
    utt, kwd = batch_inputs(D, Tu, 100 * D + Tu)
    sims = [oc.sim_matrices([k.float().numpy() for k in kwd], utt[b].float().numpy()) for b in range(B)]
    rows_k, off = pack_keywords(kwd, d)
    off_dev = off.to(d)
    u = utt.to(d).contiguous()
    K = len(TK)
    ld = (Tu + 127) // 128 * 128
    tol = rows_tol(D)
    for p0, pc in RANGES:
        n_rows = sum(TK[p % K] for p in range(p0, p0 + pc))
        rows = torch.full((L, n_rows, ld), float("nan"), dtype=torch.float32, device=d)
        _lib.check(lib.cbw_kws_sim_rows_bf16(u.data_ptr(), B, Tu, rows_k.data_ptr(), rows_k.shape[1], D, L,
                                             off_dev.data_ptr(), K, p0, pc, ld, rows.data_ptr(), _lib.stream_handle()),
                   "cbw_kws_sim_rows_bf16")
        got = rows.cpu().numpy()
        assert np.isnan(got[:, :, Tu:]).all(), "a column >= Tu was written"
        r0, worst = 0, 0.0
        for p in range(p0, p0 + pc):
            b, k = divmod(p, K)
            blk = got[:, r0:r0 + TK[k], :Tu].astype(np.float64)
            assert np.isfinite(blk).all(), f"pair {p} (rows {r0}..{r0 + TK[k] - 1}) not fully written"
            worst = max(worst, np.abs(blk - sims[b][k]).max())
            r0 += TK[k]
        assert r0 == n_rows
        print(f"D {D} Tu {Tu} pairs [{p0}, {p0 + pc}): {n_rows} rows, max |err| {worst:.3e} (tolerance {tol:.3e})")
        assert worst <= tol


@pytest.fixture(scope="module")
def small():
    """D = 128, Tu = 300, B = 3 utterances, the K = 5 keywords above, one planted match; the engine on synth weights."""
    from cbw.kws import pack_keywords
    utt, kwd = batch_inputs(128, 300, 7)
    m, eng = cnn12_engine(cnn12_sd(128), 128)
    d = eng.device
    return dict(eng=eng, model=m, utt=utt.to(d), p16=pack_keywords(kwd, d))


@pytest.mark.parametrize("size", [(38, 150), (7, 97)])
def test_bf16_pass_bit_identical_to_per_utterance_calls(small, size):
    """score_resized_batch carries the bits of score_resized(utt[b]) for every pair chunk size (below K, equal, not
    dividing K, above B * K) and under a permutation of the batch."""
    eng, utt, p16 = small["eng"], small["utt"], small["p16"]
    want = torch.stack([eng.score_resized(utt[b], p16, size) for b in range(B)])
    assert torch.isfinite(want).all() and want.shape == (B, len(TK), 2)
    for chunk in ((4, 5, 7, 64) if size == (38, 150) else (7,)):
        got = eng.score_resized_batch(utt, p16, size, chunk=chunk)
        assert torch.equal(got, want), f"chunk {chunk}: max |diff| {(got - want).abs().max().item():.3e}"
    assert torch.equal(eng.score_resized_batch(utt, p16, size), want)            # the default chunk
    perm = [2, 0, 1]
    got = eng.score_resized_batch(utt[perm].contiguous(), p16, size, chunk=7)
    assert torch.equal(got, want[perm])
    assert torch.equal(eng.score_resized_batch(utt[1:2], p16, size), want[1:2])   # alone


@pytest.fixture(scope="module")
def batch48(case48):
    """[u0, u1, u0] on case48's weights: u0 is inputs48()'s utterance, u1 a fresh unit-norm one.  144 pairs: across the
    32-map fp32 pass boundary and the 64-map compensated one."""
    g = np.random.default_rng(4848)
    u1 = torch.from_numpy(synth.l2n(g.standard_normal((L, TU48, D48)).astype(np.float32))).to(case48["utt"].device)
    u0 = case48["utt"]
    return torch.stack([u0, u1, u0]).contiguous()


@pytest.mark.parametrize("tier", ["f32", "x3"])
def test_exact_tiers_scatter_and_independence(case48, batch48, tier):
    """rescore_resized_batch over all pairs equals the per-utterance rescore_resized results bit for bit; the two copies
    of u0 carry equal bits; rows outside sel keep theirs; sel's order does not matter."""
    eng, p32 = case48["eng"], case48["p32"]
    d = eng.device
    P = 3 * K48
    every = torch.arange(K48, dtype=torch.int32, device=d)
    nan = torch.full((K48, 2), float("nan"), device=d)
    want = torch.stack([eng.rescore_resized(batch48[b], p32, SIZE48, nan.clone(), every, tier=tier) for b in range(3)])
    assert torch.isfinite(want).all()

    def run(sel, base=None):
        lg = torch.full((3, K48, 2), float("nan"), dtype=torch.float32, device=d) if base is None else base.clone()
        return eng.rescore_resized_batch(batch48, p32, SIZE48, lg, torch.tensor(sel, dtype=torch.int32, device=d),
                                         tier=tier)
    full = run(list(range(P)))
    assert torch.equal(full, want)
    assert torch.equal(full[0], full[2]), "pairs (0, k) and (2, k) of the same utterance differ"
    assert not torch.equal(full[0], full[1])
    base = torch.randn((3, K48, 2), dtype=torch.float32, device=d)
    sel = [130, 3, 77, 3]
    got = run(sel, base).view(P, 2)
    keep = torch.ones(P, dtype=torch.bool, device=d)
    keep[sel] = False
    assert torch.equal(got[keep], base.view(P, 2)[keep]), "a row outside sel was written"
    assert torch.equal(got[~keep], full.view(P, 2)[~keep])
    assert torch.equal(run(sel[::-1], base).view(P, 2), got)


def test_cascade_equals_per_utterance_cascade(case48, batch48):
    """score_resized_batch_exact = the stack of score_resized_exact, stats = their sums; spot_keywords_batch = the
    spot_keywords lists, with and without exact_band."""
    eng, m, p16, p32 = case48["eng"], case48["model"], case48["p16"], case48["p32"]
    for band_x3 in (BAND_X3, None):
        per = [eng.score_resized_exact(batch48[b], p16, p32, SIZE48, BAND48, band_x3=band_x3) for b in range(3)]
        got, stats = eng.score_resized_batch_exact(batch48, p16, p32, SIZE48, BAND48, band_x3=band_x3)
        assert torch.equal(got, torch.stack([lg for lg, _ in per]))
        assert stats == {k: sum(s[k] for _, s in per) for k in ("band", "fp32", "bf16")}
        print(f"band_x3 {band_x3}: batch cascade stats {stats}, per utterance {[s for _, s in per]}")
        assert stats["band"] >= 2 * 4 and stats["bf16"] == 3 * K48
    want = [m.spot_keywords(batch48[b], p16, SIZE48) for b in range(3)]
    assert m.spot_keywords_batch(batch48, p16, SIZE48) == want
    assert m.last_exact_stats is None
    want = [m.spot_keywords(batch48[b], p16, SIZE48, exact_band=BAND48, kwd_hs32=p32) for b in range(3)]
    assert m.spot_keywords_batch(batch48, p16, SIZE48, exact_band=BAND48, kwd_hs32=p32) == want
    assert m.last_exact_stats["bf16"] == 3 * K48 and any(want)


@pytest.mark.parametrize("exact_band", [0, 0.05])
def test_cbwhisper_two_segments_in_one_call(planted, exact_band):
    """keyword_spotting on two segments: the keyword lists and prompt ids of two single-segment calls, from exactly one
    score_resized_batch call and no score_resized call."""
    import oracle.mel as omel
    paths, _, mel = planted
    mel2 = omel.log_mel(synth.synth_clip(1), 80)
    feats = torch.from_numpy(np.stack([mel, mel2])).cuda()
    single = build(paths, exact_band=exact_band)
    ids, spotted = [], []
    for s in range(2):
        ids += single.keyword_spotting(feats[s:s + 1], start_of_prev=True)
        spotted += single.last_spotted
    assert spotted[0], "test setup: the planted keywords must be spotted in segment 0"

    both = build(paths, exact_band=exact_band)
    both.segment_keywords = "per_segment"
    eng = both.cnn.engine(128)
    calls = {"batch": 0, "single": 0}
    batch_fn, single_fn = eng.score_resized_batch, eng.score_resized

    def spy_batch(*a, **kw):
        calls["batch"] += 1
        return batch_fn(*a, **kw)

    def spy_single(*a, **kw):
        calls["single"] += 1
        return single_fn(*a, **kw)
    eng.score_resized_batch, eng.score_resized = spy_batch, spy_single
    try:
        got = both.keyword_spotting(feats, start_of_prev=True)
    finally:
        del eng.score_resized_batch, eng.score_resized
    assert both.cnn.engine(128) is eng
    assert calls == {"batch": 1, "single": 0}
    assert both.last_spotted == spotted and got == ids
    if exact_band:
        assert both.cnn.last_exact_stats["bf16"] == 2 * len(both.keywords)


def test_argument_errors(case48, batch48, small):
    """The checks that need a handle: B = 0, a workspace one byte short, a projector (variant 1) handle, the tiers
    before build_exact, n_sel > B * K, logits of the wrong shape."""
    from cbw import _lib
    from cbw.kws import KwsEngine
    eng, p16, p32 = case48["eng"], case48["p16"], case48["p32"]
    lib, d = eng.lib, eng.device
    rows, off = p16
    off_h = off.to("cpu", torch.int32).contiguous()
    off_d = off_h.to(d)
    u16 = batch48.to(torch.bfloat16).contiguous()
    Ho, Wo = SIZE48
    chunk = 64
    nb = lib.cbw_kws_score_resized_batch_workspace_bytes(eng.h, off_h.data_ptr(), K48, 3, TU48, D48, Ho, Wo, chunk)
    assert nb > 0
    wsq = lib.cbw_kws_score_resized_batch_workspace_bytes
    assert wsq(eng.h, off_h.data_ptr(), K48, 0, TU48, D48, Ho, Wo, chunk) == -1
    ws = torch.empty(nb, dtype=torch.uint8, device=d)
    lg = torch.zeros((3, K48, 2), dtype=torch.float32, device=d)

    def score(h=eng.h, B_=3, K=K48, ws_bytes=nb, D=D48):
        return lib.cbw_kws_score_resized_batch(h, u16.data_ptr(), B_, TU48, rows.data_ptr(), rows.shape[1], D,
                                               off_d.data_ptr(), off_h.data_ptr(), K, Ho, Wo, lg.data_ptr(), chunk,
                                               ws.data_ptr(), ws_bytes, _lib.stream_handle())
    assert score(B_=0) == -1 and score(B_=-2) == -1
    assert score(K=0) == 0                                              # no keywords: returns at once
    assert score(ws_bytes=nb - 1) == -3                                 # CBW_ERR_OOM
    assert score(D=D48 + 32) == -1                                      # D % 64
    hp = dict(n_layers=3, embedding_dim=128, learn_features=True, proj_mlp=True, frames_conv=False, proj_mlp_units=64)
    le = KwsEngine(hp, synth.synth_kws_state_dict(seed=0, **hp))
    assert score(h=le.h) == -1 and b"variant" in lib.cbw_last_error()
    with pytest.raises(ValueError):
        le.score_resized_batch(batch48[:, :3], p16, SIZE48)
    torch.cuda.synchronize()
    assert torch.count_nonzero(lg).item() == 0                          # no call above wrote a logit

    fresh = small["eng"]                                                # never called build_exact
    assert not fresh.has_exact_resized
    with pytest.raises(_lib.CbwError):
        fresh.rescore_resized_batch(small["utt"].float(), p32, SIZE48, torch.zeros((3, 5, 2), device=d), [0])
    u32 = batch48
    r32, _ = p32
    sel = torch.zeros(3 * K48 + 1, dtype=torch.int32, device=d)
    wsr = torch.empty(1 << 20, dtype=torch.uint8, device=d)

    def tier(fn, B_=3, n_sel=1, h=eng.h):
        return fn(h, u32.data_ptr(), B_, TU48, r32.data_ptr(), r32.shape[1], D48, off_d.data_ptr(), off_h.data_ptr(),
                  K48, Ho, Wo, sel.data_ptr(), n_sel, lg.data_ptr(), wsr.data_ptr(), wsr.numel(), _lib.stream_handle())
    for fn in (lib.cbw_kws_rescore_resized_batch, lib.cbw_kws_rescore_resized_x3_batch):
        assert tier(fn, n_sel=3 * K48 + 1) == -1                        # more pairs selected than there are
        assert tier(fn, B_=0) == -1
        assert tier(fn, n_sel=0) == 0
        assert tier(fn) == -3                                           # 1 MB of workspace is too small
        assert tier(fn, h=fresh.h) == -4                                # CBW_ERR_STATE without cbw_kws_build_exact
    for shape in ((3 * K48, 2), (3, K48), (2, K48, 2)):
        with pytest.raises(ValueError):
            eng.rescore_resized_batch(batch48, p32, SIZE48, torch.zeros(shape, device=d), [0])
    with pytest.raises(ValueError):
        eng.rescore_resized_batch(batch48, p32, SIZE48, lg, [3 * K48])   # an index past the last pair
    torch.cuda.synchronize()
    assert torch.count_nonzero(lg).item() == 0
