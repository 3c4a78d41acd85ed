"""The chained stage-2 junction (conv_stream.hip conv_stream_chain_kernel): block b's identity expand 128 -> 512 +
residual + ReLU and block b + 1's 1x1 reduce 512 -> 128 + ReLU in one launch, the reduce fed from the expand's
registers.  It does nothing numerically new -- the same MFMA, the same k order into one fp32 accumulator, bias after,
ReLU, RNE to bf16 as the two streaming launches it replaces -- so every check against them is bit for bit."""
import functools

import numpy as np
import pytest
import torch

from cbw import _lib, synth

pytestmark = pytest.mark.gpu

# (N, H, W): 91 px (a partial 64-pixel unit, most waves idle); the real stage-2 map (every wave at most one unit);
# 67 680 px = 1058 units of 64 > 256 CUs x 4 waves (some waves walk two units: the unit loop, accumulators
# re-initialised)
SHAPES = [(1, 7, 13), (3, 10, 94), (72, 10, 94)]


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded inputs, the two-launch reference (cbw_conv2d twice) and the chained launch's outputs, computed once."""
    N, H, W = shape
    lib = _lib.load()
    d = torch.device("cuda:0")
    g = torch.Generator(device=d)
    g.manual_seed(1000 + N * H * W)
    x = torch.randn((N, H, W, 128), generator=g, device=d).to(torch.bfloat16)
    res = torch.randn((N, H, W, 512), generator=g, device=d).relu().to(torch.bfloat16)
    we = (torch.randn((512, 128), generator=g, device=d) / 128 ** 0.5).to(torch.bfloat16)
    be = torch.randn(512, generator=g, device=d)
    wr = (torch.randn((128, 512), generator=g, device=d) / 512 ** 0.5).to(torch.bfloat16)
    br = torch.randn(128, generator=g, device=d)
    nan = float("nan")
    y2 = torch.full((N, H, W, 512), nan, device=d, dtype=torch.bfloat16)
    t2 = torch.full((N, H, W, 128), nan, device=d, dtype=torch.bfloat16)
    s = _lib.stream_handle()
    _lib.check(lib.cbw_conv2d(x.data_ptr(), we.data_ptr(), be.data_ptr(), res.data_ptr(), y2.data_ptr(), N, H, W, 128,
                              512, 1, 1, 1, 1, 0, 0, 1, s), "cbw_conv2d expand")
    _lib.check(lib.cbw_conv2d(y2.data_ptr(), wr.data_ptr(), br.data_ptr(), None, t2.data_ptr(), N, H, W, 512, 128, 1,
                              1, 1, 1, 0, 0, 1, s), "cbw_conv2d reduce")
    y = torch.full((N, H, W, 512), nan, device=d, dtype=torch.bfloat16)
    t1 = torch.full((N, H, W, 128), nan, device=d, dtype=torch.bfloat16)
    _lib.check(lib.cbw_conv1x1_chain(x.data_ptr(), we.data_ptr(), be.data_ptr(), res.data_ptr(), wr.data_ptr(),
                                     br.data_ptr(), y.data_ptr(), t1.data_ptr(), N, H, W, s), "cbw_conv1x1_chain")
    torch.cuda.synchronize()
    return dict(x=x, res=res, we=we, be=be, wr=wr, br=br, y2=y2, t2=t2, y=y, t1=t1)


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_equals_two_launches(shape):
    c = _case(shape)
    assert torch.isfinite(c["y2"].float()).all() and torch.isfinite(c["t2"].float()).all()
    assert torch.isfinite(c["y"].float()).all() and torch.isfinite(c["t1"].float()).all()
    assert torch.equal(c["y"], c["y2"]), (c["y"].float() - c["y2"].float()).abs().max().item()
    assert torch.equal(c["t1"], c["t2"]), (c["t1"].float() - c["t2"].float()).abs().max().item()


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_chain_vs_float64(shape):
    """Guards the reference of the test above: y and t1 against float64 over the same bf16 inputs, the intermediate Y
    rounded to bf16 as the network stores it; one conv's tolerance (test_conv_igemm_vs_torch): 1e-2 x max|ref|."""
    c = _case(shape)
    f = lambda t: t.double().reshape(-1, t.shape[-1])   # noqa: E731
    yr = (f(c["x"]) @ c["we"].double().t() + c["be"].double() + f(c["res"])).relu()
    tr = (yr.to(torch.bfloat16).double() @ c["wr"].double().t() + c["br"].double()).relu()
    ey = (f(c["y"]) - yr).abs().max().item()
    et = (f(c["t1"]) - tr).abs().max().item()
    print(f"chain vs float64 {shape}: y err {ey:.3e} (max|ref| {yr.abs().max().item():.3f}), "
          f"t1 err {et:.3e} (max|ref| {tr.abs().max().item():.3f})")
    assert ey <= 1e-2 * yr.abs().max().item()
    assert et <= 1e-2 * tr.abs().max().item()


HP = dict(n_layers=3, embedding_dim=1280, learn_features=True, proj_mlp=True, frames_conv=True, proj_mlp_units=64,
          resnet_version="resnet-50", threshold=0.5)


@functools.lru_cache(maxsize=None)
def _engine(version):
    """large-v3 LEF widths, small maps (keywords of 64 frames against an utterance of 400: stage-2 map 4 x 25)."""
    from cbw.kws import KwsEngine
    hp = dict(HP, resnet_version=version)
    eng = KwsEngine(hp, synth.synth_kws_state_dict(seed=4, **hp))
    d = eng.device
    g = torch.Generator(device=d)
    g.manual_seed(31)
    kwd = torch.randn((40, 3, 64, 1280), generator=g, device=d)
    km = torch.ones((40, 3, 64), device=d)
    km[::5, :, 40:] = 0
    utt = torch.randn((1, 3, 400, 1280), generator=g, device=d)
    um = torch.ones((1, 3, 400), device=d)
    pk, pkm = eng.project(kwd, km)
    pu, pum = eng.project(utt, um)
    return dict(eng=eng, pk=pk, pkm=pkm, pu=pu[0], pum=pum[0], kwd=kwd, km=km, utt=utt, um=um)


@pytest.mark.parametrize("K,chunk", [(3, 3), (40, 20)])
def test_score_bit_identical_with_and_without_chain(monkeypatch, K, chunk):
    """KwsEngine.score with the junctions chained (default) and as separate launches (CBW_CS_CHAIN=0): one chunk on the
    whole grid, and two chunks on two streams (the shared grid)."""
    s = _engine("resnet-50")
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("CBW_CS_CHAIN", mode)
        out[mode] = s["eng"].score(s["pu"], s["pum"], s["pk"][:K].contiguous(), s["pkm"][:K].contiguous(), chunk=chunk)
    monkeypatch.delenv("CBW_CS_CHAIN")
    out["default"] = s["eng"].score(s["pu"], s["pum"], s["pk"][:K].contiguous(), s["pkm"][:K].contiguous(), chunk=chunk)
    torch.cuda.synchronize()
    assert torch.isfinite(out["default"]).all()
    assert torch.equal(out["0"], out["default"]), (out["0"] - out["default"]).abs().max().item()
    assert torch.equal(out["1"], out["default"])


def test_profile_records_of_a_chained_chunk(monkeypatch):
    """One scoring chunk with the launch profile on: the chained run makes 2 launches fewer (s2b1 -> s2b2, s2b2 -> s2b3)
    with the same summed algorithmic FLOPs, each chained launch one record under the chained kernel's name."""
    import ctypes
    s = _engine("resnet-50")
    eng, lib = s["eng"], _lib.load()
    got = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("CBW_CS_CHAIN", mode)
        _lib.check(lib.cbw_kws_profile(eng.h, 64), "cbw_kws_profile")
        eng.score(s["pu"], s["pum"], s["pk"][:3].contiguous(), s["pkm"][:3].contiguous(), chunk=3)
        torch.cuda.synchronize()
        st, en, fl = (np.zeros(64) for _ in range(3))
        n = lib.cbw_kws_profile_records(eng.h, st.ctypes.data, en.ctypes.data, fl.ctypes.data, 64)
        names = (ctypes.c_char_p * 64)()
        lib.cbw_kws_profile_kernels(eng.h, names, 64)
        lib.cbw_kws_profile(eng.h, 0)
        got[mode] = (n, fl[:n].sum(), [(names[i] or b"").decode() for i in range(n)])
    assert 0 < got["1"][0] < 64
    assert got["0"][0] - got["1"][0] == 2
    assert got["0"][1] == got["1"][1]
    assert sum(k.startswith("conv_stream_chain_kernel") for k in got["1"][2]) == 2
    assert not any(k.startswith("conv_stream_chain_kernel") for k in got["0"][2])


def test_profile_records_across_entry_points():
    """One profile session over four calls on the same 3 keywords in one chunk: cbw_kws_score, cbw_kws_score_pairs
    (B = 1, pair p = (0, p)), cbw_kws_score_fp8, cbw_kws_score again.  The pair call runs the same network launches as
    the single-utterance call, so its records match in count, kernel names and FLOPs; the fp8 call's records all carry
    tier 2, and the bf16 call after it tier 0 again (cbw_kws_profile starts the session at tier 0)."""
    import ctypes
    s = _engine("resnet-50")
    eng, lib = s["eng"], _lib.load()
    K, CAP = 3, 256
    pk, pkm = s["pk"][:K].contiguous(), s["pkm"][:K].contiguous()
    pk32, _ = eng.project_f32(s["kwd"][:K], s["km"][:K])
    pu32, _ = eng.project_f32(s["utt"], s["um"])
    eng.calibrate_fp8(pu32[0], s["pum"], pk32, pkm, margin=1.0, utt=s["pu"], kwd=pk)
    _lib.check(lib.cbw_kws_profile(eng.h, CAP), "cbw_kws_profile")
    calls = [lambda: eng.score(s["pu"], s["pum"], pk, pkm, chunk=K),
             lambda: eng.score_pairs(s["pu"][None], s["pum"][None], pk, pkm, [0] * K, list(range(K)), chunk=K),
             lambda: eng.score_fp8(s["pu"], s["pum"], pk, pkm, chunk=K),
             lambda: eng.score(s["pu"], s["pum"], pk, pkm, chunk=K)]
    marks = [0]
    for call in calls:
        call()
        marks.append(lib.cbw_kws_profile_tiers(eng.h, None, 0))
    torch.cuda.synchronize()
    st, en, fl = (np.zeros(CAP) for _ in range(3))
    tiers = np.full(CAP, -1, np.int32)
    names = (ctypes.c_char_p * CAP)()
    n = lib.cbw_kws_profile_records(eng.h, st.ctypes.data, en.ctypes.data, fl.ctypes.data, CAP)
    lib.cbw_kws_profile_tiers(eng.h, tiers.ctypes.data, CAP)
    lib.cbw_kws_profile_kernels(eng.h, names, CAP)
    lib.cbw_kws_profile(eng.h, 0)
    assert marks[-1] == n < CAP   # nothing dropped for want of room
    rec = [([(names[i] or b"").decode() for i in range(a, b)], fl[a:b].tolist(), tiers[a:b].tolist())
           for a, b in zip(marks[:-1], marks[1:])]
    score, pairs, fp8, again = rec
    assert len(score[0]) > 0 and all(f > 0 for f in score[1])
    assert len(pairs[0]) == len(score[0]) and pairs[0] == score[0] and pairs[1] == score[1]
    assert set(score[2]) == {0} and set(pairs[2]) == {0}
    assert len(fp8[0]) > 0 and set(fp8[2]) == {2}
    assert again[0] == score[0] and again[1] == score[1] and set(again[2]) == {0}


def test_untouched_paths_still_run():
    """ResNet-34 (basic blocks: nothing to chain) and the fp8 tier (its stage-2 blocks are e4m3 convs) with the
    default settings."""
    s34 = _engine("resnet-34")
    l34 = s34["eng"].score(s34["pu"], s34["pum"], s34["pk"][:3].contiguous(), s34["pkm"][:3].contiguous(), chunk=3)
    s = _engine("resnet-50")
    eng = s["eng"]
    pk32, _ = eng.project_f32(s["kwd"][:8], s["km"][:8])
    pu32, _ = eng.project_f32(s["utt"], s["um"])
    eng.calibrate_fp8(pu32[0], s["pum"], pk32, s["pkm"][:8].contiguous(), margin=1.0, utt=s["pu"],
                      kwd=s["pk"][:8].contiguous())
    l8 = eng.score_fp8(s["pu"], s["pum"], s["pk"][:8].contiguous(), s["pkm"][:8].contiguous(), chunk=8)
    torch.cuda.synchronize()
    assert torch.isfinite(l34).all() and torch.isfinite(l8).all()
