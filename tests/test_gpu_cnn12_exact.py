"""Exact fp32 decisions for CB-Whisper's own 12-channel spotter (model/cb_whisper.py:110-128 as the reference runs it:
fp32 inner products of fp32 hidden states, bilinear resize, Resnet(num_channels=12), argmax): the fp32 front of the
re-scoring tiers (similarity rows on the fp32-input MFMA, resize to fp32 NHWC maps), the two tiers over it
(cbw_kws_rescore_resized / _x3), the cascade (KwsEngine.score_resized_exact) and CBWhisper's cnn path.

Tolerances.  Frames are unit vectors, so a D-term fp32 dot product errs by at most D 2^-24 to first order
(Cauchy-Schwarz) and the resize, a convex combination, adds a few ulps: SIM_TOL(D) = (D + 8) 2^-24 against float64,
twice that per element against the golden's fp32 maps (torch's own fp32 sums err as much).  Logits: RESCORE_RTOL = 1e-4
of max |logit| (tests/test_gpu_kws.py, tests/test_gpu_kws_tiers.py).  BAND_X3 = 1e-4: the compensated tier's distance
from the fp32 tier that the cascade's second band relies on.

Measured on MI355X (this file's prints): see docs/MEASUREMENT_LOG.md, "Exact fp32 decisions for CB-Whisper's own
12-channel spotter".
"""
import os
import sys

import numpy as np
import pytest
import torch

from cbw import synth

pytestmark = pytest.mark.gpu

L = 12
RESCORE_RTOL = 1e-4
BAND_X3 = 1e-4
SIZES = [(150, 750), (7, 97), (38, 150)]   # up- and down-scaling on both axes, a non-integer ratio, the exact ratio 2
TK = [1, 9, 65, 171]
SEL = [3, 0, 2, 3, 1]                      # out of order, one repeat


def sim_tol(D):
    return (D + 8) * 2.0 ** -24


def cnn12_sd(D=128):
    return synth.synth_kws_state_dict(seed=3, n_layers=L, embedding_dim=D, learn_features=False, proj_mlp=False)


def cnn12_engine(sd, D=128):
    from model.model import KWSModel
    m = KWSModel()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m, m.engine(D)


def golden_inputs():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import cnn12_inputs
    return cnn12_inputs()


def prob1(logits):
    return torch.softmax(torch.as_tensor(logits).double(), -1)[:, 1].cpu().numpy()


def front(utt, kwd, sel, sizes):
    """The two kernels one by one on the GPU: (rows f32 [n][L][tk_max][ld] as numpy, {size: maps [n][Ho][Wo][L]})."""
    from cbw import _lib
    from cbw.kws import pack_keywords
    lib = _lib.load()
    d = torch.device("cuda:0")
    rows_k, off = pack_keywords([torch.from_numpy(k) for k in kwd], d, dtype=torch.float32)
    off_dev = off.to(d)
    u = torch.from_numpy(utt).to(d).contiguous()
    _, Tu, D = u.shape
    K, n = len(kwd), len(sel)
    tk_max, ld = max(k.shape[1] for k in kwd), (Tu + 63) // 64 * 64
    sel_d = torch.tensor(sel, dtype=torch.int32, device=d)
    rows = torch.full((n, L, tk_max, ld), float("nan"), dtype=torch.float32, device=d)
    _lib.check(lib.cbw_kws_sim_rows_f32(u.data_ptr(), Tu, rows_k.data_ptr(), rows_k.shape[1], D, L, off_dev.data_ptr(), K,
                                        sel_d.data_ptr(), n, tk_max, ld, rows.data_ptr(), _lib.stream_handle()),
               "cbw_kws_sim_rows_f32")
    maps = {}
    for Ho, Wo in sizes:
        m = torch.full((n, Ho, Wo, L), float("nan"), dtype=torch.float32, device=d)
        _lib.check(lib.cbw_kws_sim_resize_f32(rows.data_ptr(), Tu, rows_k.shape[1], L, off_dev.data_ptr(), K,
                                              sel_d.data_ptr(), n, tk_max, ld, Ho, Wo, m.data_ptr(),
                                              _lib.stream_handle()), "cbw_kws_sim_resize_f32")
        maps[(Ho, Wo)] = m.cpu().numpy()
    return rows.cpu().numpy(), maps


@pytest.mark.parametrize("D,Tu", [(64, 130), (64, 1500), (1280, 130), (1280, 1500)])
def test_similarity_rows_and_resize_vs_float64(D, Tu):
    """sim_rows_f32 and sim_resize_f32 against oracle.cnn12.sim_matrices / resize_bilinear in float64: ragged keywords of
    1, 9, 65 and 171 frames (one tile row, a partial one, two, three), a masked tail tile (Tu = 130) and the reference's
    1500 frames, sel out of order with a repeat; every element outside a keyword's [Tk][Tu] block stays unwritten."""
    import oracle.cnn12 as oc
    g = np.random.default_rng(100 * D + Tu)
    utt = synth.l2n(g.standard_normal((L, Tu, D)).astype(np.float32))
    kwd = [synth.l2n(g.standard_normal((L, T, D)).astype(np.float32)) for T in TK]
    kwd[2][:, 5:35] = utt[:, 60:90]          # a planted match: similarities up to 1
    rows, maps = front(utt, kwd, SEL, SIZES)
    sims = oc.sim_matrices(kwd, utt)         # float64 [L][Tk][Tu] per keyword
    tol = sim_tol(D)
    worst = 0.0
    for i, k in enumerate(SEL):
        T = TK[k]
        err = np.abs(rows[i, :, :T, :Tu].astype(np.float64) - sims[k]).max()
        worst = max(worst, err)
        assert err <= tol, f"similarity rows of keyword {k} (map {i}): {err:.3e} > {tol:.3e}"
        assert np.isnan(rows[i, :, T:, :]).all() and np.isnan(rows[i, :, :, Tu:]).all(), "write outside the keyword's block"
    print(f"D {D} Tu {Tu}: similarity rows max |err| {worst:.3e} (tolerance {tol:.3e})")
    for size in SIZES:
        worst = 0.0
        for i, k in enumerate(SEL):
            ref = oc.resize_bilinear(sims[k], size)                      # [L][Ho][Wo]
            err = np.abs(maps[size][i].transpose(2, 0, 1).astype(np.float64) - ref).max()
            worst = max(worst, err)
            assert err <= tol, f"resized map of keyword {k} at {size}: {err:.3e} > {tol:.3e}"
        print(f"D {D} Tu {Tu}: resize to {size} max |err| {worst:.3e}")


def test_resized_maps_vs_reference_golden(golden_dir):
    """The fp32 maps of cnn12_inputs() against what the reference's torch ops gave (tests/golden/cnn12.npz: keyword 1's
    map subsampled, and every map's per-channel sum): twice SIM_TOL per element."""
    g = np.load(os.path.join(golden_dir, "cnn12.npz"))
    utt, kwd = golden_inputs()
    _, maps = front(utt, kwd, list(range(len(kwd))), [(150, 750)])
    m = maps[(150, 750)].transpose(0, 3, 1, 2)                           # [K][L][150][750]
    tol = 2 * sim_tol(utt.shape[-1])
    err = np.abs(m[1][:, ::7, ::11].astype(np.float64) - g["maps_k1_sub"]).max()
    serr = np.abs(m.astype(np.float64).sum(axis=(2, 3)) - g["maps_sum"]).max()
    print(f"golden maps: max |err| {err:.3e} (tolerance {tol:.3e}); per-channel sums max |err| {serr:.3e}")
    assert err <= tol
    assert serr <= tol * 150 * 750


@pytest.fixture(scope="module")
def golden_tiers(golden_dir):
    """cnn12_inputs() through the bf16 pass and both exact tiers, all five keywords, once."""
    from cbw.kws import pack_keywords
    utt, kwd = golden_inputs()
    m, eng = cnn12_engine(cnn12_sd())
    d = eng.device
    u = torch.from_numpy(utt).to(d)
    kt = [torch.from_numpy(k) for k in kwd]
    p16, p32 = pack_keywords(kt, d), pack_keywords(kt, d, dtype=torch.float32)
    bf16 = eng.score_resized(u, p16)
    assert not eng.has_exact_resized and not eng.has_fp32
    with pytest.raises(Exception):
        eng.rescore_resized(u, p32, (150, 750), torch.empty_like(bf16), torch.arange(5))
    eng.build_exact()
    assert eng.has_exact_resized and not eng.has_fp32
    out = {"bf16": bf16.cpu().numpy()}
    for tier in ("f32", "x3"):
        lg = torch.full((len(kwd), 2), float("nan"), dtype=torch.float32, device=d)
        eng.rescore_resized(u, p32, (150, 750), lg, torch.arange(len(kwd), dtype=torch.int32, device=d), tier=tier)
        out[tier] = lg.cpu().numpy()
    torch.cuda.synchronize()
    return np.load(os.path.join(golden_dir, "cnn12.npz")), out, (eng, u, p16, p32)


def test_fp32_tier_matches_reference_fp32(golden_tiers):
    """Every keyword re-scored in fp32: logits within RESCORE_RTOL of max |logit| of the reference's fp32 forward
    (cnn12.npz) and the same argmax list.  The bf16 pass alone misses this bound (1.4-5.5e-3 observed), so the test
    fails without the fp32 front."""
    g, out, _ = golden_tiers
    ref = g["logits"]
    scale = np.abs(ref).max()
    e32 = np.abs(out["f32"] - ref).max() / scale
    e16 = np.abs(out["bf16"] - ref).max() / scale
    print(f"12-channel spotter vs reference fp32 logits, relative to max |logit| {scale:.4f}: fp32 tier {e32:.3e}, "
          f"bf16 pass {e16:.3e}")
    assert np.isfinite(out["f32"]).all()
    assert e32 <= RESCORE_RTOL
    assert np.flatnonzero(out["f32"].argmax(1) == 1).tolist() == g["argmax_idx"].tolist()


def test_compensated_tier_within_band_x3_of_fp32_tier(golden_tiers):
    """|p_x3 - p_f32| < BAND_X3 on the same five keywords: the condition under which the keywords the compensated tier
    leaves outside the second band need no fp32 pass."""
    _, out, _ = golden_tiers
    dp = np.abs(prob1(out["x3"]) - prob1(out["f32"])).max()
    dl = np.abs(out["x3"] - out["f32"]).max() / np.abs(out["f32"]).max()
    print(f"12-channel compensated tier vs fp32 tier: max |p_x3 - p_f32| {dp:.3e}, logits {dl:.3e} of max |logit|")
    assert np.isfinite(out["x3"]).all()
    assert dp < BAND_X3


def test_argument_errors(golden_tiers):
    """The checks of cbw_kws_rescore_resized on a built handle, and CBW_ERR_STATE on one that never called
    cbw_kws_build_exact."""
    from cbw import _lib
    _, _, (eng, u, p16, p32) = golden_tiers
    lib, d = eng.lib, eng.device
    rows, off = p32
    off_h = off.to("cpu", torch.int32).contiguous()
    off_d = off_h.to(d)
    K, R, D, Tu = off_h.numel() - 1, rows.shape[1], rows.shape[2], u.shape[1]
    sel = torch.arange(K, dtype=torch.int32, device=d)
    lg = torch.zeros((K, 2), dtype=torch.float32, device=d)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=d)

    def call(h=eng.h, D=D, off_host=off_h, Ho=150, Wo=750, n_sel=K, fn=lib.cbw_kws_rescore_resized, R=R):
        return fn(h, u.data_ptr(), Tu, rows.data_ptr(), R, D, off_d.data_ptr(), off_host.data_ptr(), K, Ho, Wo,
                  sel.data_ptr(), n_sel, lg.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle())
    for fn in (lib.cbw_kws_rescore_resized, lib.cbw_kws_rescore_resized_x3):
        assert call(fn=fn, D=D + 8) == -1                                # D % 16
        bad = off_h.clone()
        bad[2] = bad[1]
        assert call(fn=fn, off_host=bad) == -1                           # an empty keyword: offsets not increasing
        assert call(fn=fn, R=R - 1) == -1                                # offsets beyond the rows
        assert call(fn=fn, Ho=6) == -1 and call(fn=fn, Wo=6) == -1       # smaller than the stem's kernel
        assert call(fn=fn, n_sel=0) == 0                                 # nothing selected: returns at once
        assert call(fn=fn) == -3                                         # 1 MB of workspace is too small
    assert lib.cbw_kws_rescore_resized_workspace_bytes(eng.h, off_h.data_ptr(), K, Tu, D, 6, 750) == -1
    assert lib.cbw_kws_build_exact(eng.h) == 0                           # a second call: no-op success
    _, fresh = cnn12_engine(cnn12_sd())
    assert call(h=fresh.h) == -4 and call(h=fresh.h, n_sel=0) == -4      # CBW_ERR_STATE without cbw_kws_build_exact
    assert lib.cbw_kws_rescore_resized_workspace_bytes(fresh.h, off_h.data_ptr(), K, Tu, D, 150, 750) == -1
    assert torch.count_nonzero(lg).item() == 0                           # no call above wrote a logit


# ---- K = 48 ragged keywords at D = 128, Tu = 300, maps (38, 150): crosses the fp32 tier's 32-map pass boundary
SEED48 = 2          # picked on the CPU with oracle.cnn12.keyword_spotting_logits: 22 keywords within BAND48 of p = 0.5
                    # after the bias shift, 26 outside, the nearest 7.8e-4 from the boundary (no near-tie)
K48, D48, TU48, SIZE48 = 48, 128, 300, (38, 150)
BAND48 = 0.0075     # the bf16 pass is held to LOGIT_RTOL = 2e-2 of max |logit| (tests/test_gpu_kws.py; max |logit| is
                    # 0.65 here): 1.3e-2 on each logit, twice that on the margin l1 - l0, and p moves by at most a
                    # quarter of the margin's error: 6.5e-3 < BAND48
NEAR_TIE = 1e-4     # |p_oracle - 0.5| below which fp32 and float64 may decide differently: the fp32 tier's
                    # RESCORE_RTOL x max |logit| on both logits moves p by at most 2 x 1e-4 x 0.65 / 4 = 3.3e-5


def inputs48():
    g = np.random.default_rng(SEED48)
    utt = synth.l2n(g.standard_normal((L, TU48, D48)).astype(np.float32))
    lens = g.integers(3, 70, K48)
    kwd = [synth.l2n(g.standard_normal((L, int(T), D48)).astype(np.float32)) for T in lens]
    for k in range(0, K48, 3):   # every third keyword shares frames with the utterance, mixed with noise
        T = kwd[k].shape[1]
        s = int(g.integers(0, TU48 - T))
        a = g.uniform(0.2, 1.0)
        kwd[k] = synth.l2n(a * utt[:, s:s + T] + (1 - a) * kwd[k])
    return utt, kwd


@pytest.fixture(scope="module")
def case48():
    """The float64 oracle's logits of the 48 keywords (computed once), the class-1 bias lowered by their median margin so
    that the probabilities straddle 0.5 (bench.py's operating points do the same), and the engine on those weights."""
    import oracle.cnn12 as oc
    from cbw.kws import pack_keywords
    utt, kwd = inputs48()
    sd = cnn12_sd(D48)
    lg = oc.keyword_spotting_logits(sd, kwd, utt, SIZE48)
    shift = -float(np.median(lg[:, 1] - lg[:, 0]))
    sd = dict(sd)
    sd["model.classifier.1.bias"] = np.asarray(sd["model.classifier.1.bias"]).copy()
    sd["model.classifier.1.bias"][1] += shift
    lg = lg.copy()
    lg[:, 1] += shift
    m, eng = cnn12_engine(sd, D48)
    eng.build_exact()
    d = eng.device
    kt = [torch.from_numpy(k) for k in kwd]
    return dict(oracle=lg, eng=eng, utt=torch.from_numpy(utt).to(d), p16=pack_keywords(kt, d),
                p32=pack_keywords(kt, d, dtype=torch.float32), model=m)


@pytest.mark.parametrize("tier", ["f32", "x3"])
def test_scatter_and_pass_independence(case48, tier):
    """Rows outside sel keep their bits; a keyword's logits are the same bits alone, inside a pass of many, in another
    position of sel and on the far side of a pass boundary (32 maps in fp32; 64 in the compensated tier, crossed with
    repeats in sel)."""
    eng, u, p32 = case48["eng"], case48["utt"], case48["p32"]
    d = eng.device

    def run(sel, base=None):
        lg = torch.full((K48, 2), float("nan"), dtype=torch.float32, device=d) if base is None else base.clone()
        return eng.rescore_resized(u, p32, SIZE48, lg, torch.tensor(sel, dtype=torch.int32, device=d), tier=tier)
    full = run(list(range(K48)))                                   # passes [0, 32) and [32, 48) in fp32
    assert torch.isfinite(full).all()
    for k in (0, 31, 32, 47):
        alone = run([k])
        assert torch.equal(alone[k], full[k]), f"keyword {k} alone differs from keyword {k} in a pass of many"
        assert torch.isnan(alone[torch.arange(K48, device=d) != k]).all()
    assert torch.equal(run(list(range(K48))[::-1]), full)          # every keyword in another slot and pass
    assert torch.equal(run(list(range(K48)) + list(range(22))), full)   # 70 maps: across the x3 pass boundary too
    base = torch.randn((K48, 2), dtype=torch.float32, device=d)
    sub = [40, 3, 17]
    got = run(sub, base)
    keep = torch.ones(K48, dtype=torch.bool, device=d)
    keep[sub] = False
    assert torch.equal(got[keep], base[keep]), "a row outside sel was written"
    assert torch.equal(got[~keep], full[~keep])


def test_cascade_decisions(case48):
    """score_resized_exact spots exactly what all-keywords fp32 re-scoring spots, both equal the float64 oracle outside
    an oracle-confirmed near-tie, keywords outside the band keep their bf16 logits bit for bit, and the counts add up."""
    eng, u, p16, p32, want = case48["eng"], case48["utt"], case48["p16"], case48["p32"], case48["oracle"]
    d = eng.device
    bf16 = eng.score_resized(u, p16, SIZE48)
    all32 = eng.rescore_resized(u, p32, SIZE48, torch.empty_like(bf16), torch.arange(K48, dtype=torch.int32, device=d))
    p16v, p32v, pw = prob1(bf16), prob1(all32), prob1(want)
    inside = np.abs(p16v.astype(np.float32) - np.float32(0.5)) <= np.float32(BAND48)
    print(f"K = 48: bf16 max |p - p_f32| {np.abs(p16v - p32v).max():.3e}, fp32 tier max |p - p_oracle| "
          f"{np.abs(p32v - pw).max():.3e}, logits {np.abs(all32.cpu().numpy() - want).max() / np.abs(want).max():.3e} of "
          f"max |logit|; {int(inside.sum())} keywords inside the band {BAND48}, nearest oracle |p - 0.5| "
          f"{np.abs(pw - 0.5).min():.3e}")
    assert inside.sum() >= 4 and (~inside).sum() >= 4, "test setup: the band must split the keywords"
    assert np.abs(p16v - p32v).max() < BAND48, "test setup: the bf16 error must stay inside the band"
    spot32 = set(np.flatnonzero(all32.cpu().numpy().argmax(1) == 1).tolist())
    sure = np.abs(pw - 0.5) >= NEAR_TIE
    spot_w = set(np.flatnonzero(want.argmax(1) == 1).tolist())
    for band_x3 in (BAND_X3, None):
        lg, stats = eng.score_resized_exact(u, p16, p32, SIZE48, BAND48, band_x3=band_x3)
        got = set(np.flatnonzero(lg.cpu().numpy().argmax(1) == 1).tolist())
        assert got == spot32
        assert {k for k in got if sure[k]} == {k for k in spot_w if sure[k]}
        out_idx = torch.from_numpy(np.flatnonzero(~inside)).to(d)
        assert torch.equal(lg[out_idx], bf16[out_idx]), "a keyword outside the band lost its bf16 logits"
        assert stats["bf16"] == K48 and stats["band"] == int(inside.sum())
        changed = int((lg != bf16).any(1).sum())
        assert changed <= stats["band"]
        if band_x3 is None:
            assert stats["fp32"] == stats["band"]
            in_idx = torch.from_numpy(np.flatnonzero(inside)).to(d)
            assert torch.equal(lg[in_idx], all32[in_idx])
        else:
            assert 0 <= stats["fp32"] <= stats["band"]
            px = prob1(lg)
            second = np.abs(px.astype(np.float32) - np.float32(0.5)) <= np.float32(band_x3)
            # whoever is still inside the second band after the cascade carries fp32-tier logits
            idx2 = torch.from_numpy(np.flatnonzero(second & inside)).to(d)
            assert torch.equal(lg[idx2], all32[idx2])
    # the model-level entry: same decisions, bf16 by default
    m = case48["model"]
    assert m.spot_keywords(u, p16, SIZE48) == sorted(np.flatnonzero(bf16.cpu().numpy().argmax(1) == 1).tolist())
    assert m.last_exact_stats is None
    assert set(m.spot_keywords(u, p16, SIZE48, exact_band=BAND48, kwd_hs32=p32)) == spot32
    assert m.last_exact_stats["band"] == int(inside.sum())


# ---- CBWhisper, cnn path: the fixture shapes of tests/test_gpu_cbwhisper.py
PROMPT = dict(keyword_prompt_prepend="The topic of today's speech is, ah, ",
              keyword_prompt_append=". Okay, then I'll continue.", keyword_separator=", ")


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    import oracle.cbwhisper as ocb
    import oracle.mel as omel
    enc_sd = synth.synth_whisper_encoder_state_dict("micro-deep", 0)
    mel = omel.log_mel(synth.synth_clip(0), 80)
    u = ocb.utterance_hs(enc_sd, mel, synth.WHISPER_CONFIGS["micro-deep"][3])
    khs = {0: u[:, 100:140], 2: u[:, 700:725], 4: u[:, 1200:1260]}
    paths = synth.write_cbwhisper_fixture(str(tmp_path_factory.mktemp("cbwexact")), keyword_hs=khs,
                                          cnn_class1_shift=-2.5)
    return paths, enc_sd, mel


def build(paths, **kw):
    from model.cb_whisper import CBWhisper
    args = dict(dataset="acl", split="test", root=paths["acl"], kw_type="tts", encoder_ckpt=paths["encoder"],
                whisper_ckpt=paths["whisper"], kws_ckpt=paths["kws_ckpt"], language="English", prompt=True,
                oracle="kws", kws_features_size=(150, 750), keywords_per_group=100, **PROMPT)
    args.update(kw)
    return CBWhisper(**args)


def test_cbwhisper_cnn_path_honours_exact_band(planted):
    """exact_band = 1.0 (every keyword re-scored in fp32): the oracle's keyword list; exact_band = 0 and the default:
    today's bf16 output, no fp32 network built; "auto": a band measured at the first segment and kept."""
    import oracle.cbwhisper as ocb
    paths, enc_sd, mel = planted
    feats = torch.from_numpy(mel[None]).cuda()
    default = build(paths)
    ids0 = default.keyword_spotting(feats, start_of_prev=True)
    assert default.exact_band == 0 and not default.cnn.engine(128).has_exact_resized and default._packed32 is None
    zero = build(paths, exact_band=0)
    assert zero.keyword_spotting(feats, start_of_prev=True) == ids0 and zero.last_spotted == default.last_spotted
    assert not zero.cnn.engine(128).has_exact_resized

    ck = torch.load(paths["kws_ckpt"], map_location="cpu", weights_only=True)["state_dict"]
    ksd = {k: v.numpy() for k, v in ck.items()}
    exact = build(paths, exact_band=1.0)
    ids1 = exact.keyword_spotting(feats, start_of_prev=True)
    khs = [h.numpy() for h in exact.kw_database.db.hidden_states]
    want, want_ids, lgs = ocb.keyword_spotting(enc_sd, synth.WHISPER_CONFIGS["micro-deep"][3], mel[None], ksd, khs,
                                               exact.keywords, exact.get_prompt_ids, 100, (150, 750), exact.prepend,
                                               exact.append, exact.sep, start_of_prev=True)
    assert exact.last_spotted == want and ids1 == want_ids
    assert exact.cnn.last_exact_stats == {"band": len(khs), "fp32": exact.cnn.last_exact_stats["fp32"],
                                          "bf16": len(khs)}
    assert exact.cnn.engine(128).has_exact_resized and exact._packed32 is not None

    auto = build(paths, exact_band="auto")
    assert auto.band_calibration is None
    assert auto.keyword_spotting(feats, start_of_prev=True) == want_ids
    cal = auto.band_calibration
    print("CBWhisper cnn path, exact_band='auto':", cal)
    assert cal["held_out_pairs"] == len(khs) and cal["bias_calibration_pairs"] == 0
    assert cal["band"] == auto.exact_band and 0.03 <= cal["band"] <= 0.5 and cal["band"] >= 2 * cal["max_bf16_err"]
    # the group-size resize (kws_features_size=None) runs the same cascade per group
    grp = build(paths, exact_band=1.0, kws_features_size=None)
    grp0 = build(paths, kws_features_size=None)
    grp.spot_keywords(feats)
    assert grp.cnn.last_exact_stats["band"] == len(khs)
    assert grp0.spot_keywords(feats) is not None and grp0.cnn.last_exact_stats is None
