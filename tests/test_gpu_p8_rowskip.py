"""conv_igemm_p8's 3x3 tiles in row order without their all-padding kernel rows (CBW_P8_ROWSKIP, csrc/p8_rowmap.h):
the dropped K-tiles added exact zeros to the fp32 accumulators and the remaining ones keep their order, so every output
is bit-identical with the switch on and off -- single convs at the smallest shapes conv_igemm_p8 still takes (>= 256
tiles), group sizes that make every tile mix image rows / straddle / end in a short group / flat, one conv of the
compensated tier, and the whole classifier.  Outputs start NaN-filled: a row the map loses shows."""
import pytest
import torch

from cbw import synth

pytestmark = pytest.mark.gpu

CASES = [
    # N, H, W, Cin, Cout, k, stride
    (460, 3, 24, 512, 512, 3, 1),     # Ho 3: top, middle and bottom tiles; two channel tiles; M tail
    (460, 5, 47, 512, 512, 3, 2),     # odd H at stride 2: both ends skip
    (280, 10, 94, 256, 256, 3, 2),    # even H at stride 2: only the top skips
    (300, 5, 47, 256, 256, 3, 1),     # stage-3 3x3
    (150, 10, 94, 128, 128, 3, 1),    # 512 x 128 tiles
    (150, 19, 188, 128, 128, 3, 2),   # 512 x 128 tiles, stride 2
    (2800, 1, 24, 256, 256, 3, 1),    # Ho 1: kernel rows 0 and 2 both dropped in every tile
    (1400, 2, 24, 256, 256, 3, 1),    # Ho 2: no middle row
]
# the group sizes cases 1 and 4 also run at: 1 = every tile mixes image rows (the conservative rule skips almost
# nothing), 7 = straddling tiles and a short last group, above N = the flat order
GROUPED = {CASES[0]: (1, 7, 461), CASES[3]: (1, 7, 100000)}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_rowskip_bit_identical(monkeypatch, case):
    """cbw_conv2d with CBW_P8_ROWSKIP=0 and =1 (default group size, and the GROUPED ones): torch.equal, and the
    tolerance of test_p8_lef_shapes_deterministic_vs_fp32 against an fp32 conv2d + bias + ReLU (1 % of its largest
    value: bf16 output rounding)."""
    from cbw import _lib
    N, H, W, Cin, Cout, K, s = case
    lib = _lib.load()
    d = torch.device("cuda:0")
    g = torch.Generator(device=d)
    g.manual_seed(31)
    x = torch.randn((N, H, W, Cin), generator=g, device=d).to(torch.bfloat16)
    w = (torch.randn((Cout, K, K, Cin), generator=g, device=d) / (Cin * K * K) ** 0.5).to(torch.bfloat16)
    b = torch.randn((Cout,), generator=g, device=d)
    p = K // 2
    Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1

    def run(skip, group):
        monkeypatch.setenv("CBW_P8_ROWSKIP", skip)
        monkeypatch.setenv("CBW_P8_ROWGROUP", str(group))
        y = torch.full((N, Ho, Wo, Cout), float("nan"), dtype=torch.bfloat16, device=d)
        _lib.check(lib.cbw_conv2d(x.data_ptr(), w.data_ptr(), b.data_ptr(), None, y.data_ptr(), N, H, W, Cin, Cout,
                                  K, K, s, s, p, p, 1, _lib.stream_handle()), "cbw_conv2d")
        return y

    off = run("0", 0)
    on = {G: run("1", G) for G in (0,) + GROUPED.get(case, ())}
    torch.cuda.synchronize()
    ref = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), b, stride=s,
                                     padding=p).clamp_min(0).permute(0, 2, 3, 1)
    atol = 1e-2 * ref.abs().max().item()
    torch.testing.assert_close(off.float(), ref, rtol=0, atol=atol)
    for G, y in on.items():
        assert torch.isfinite(y.float()).all(), G
        assert torch.equal(off, y), G
        torch.testing.assert_close(y.float(), ref, rtol=0, atol=atol)


def test_rowskip_compensated_tier_conv(monkeypatch):
    """One 3x3 conv of the compensated tier through cbw_conv2d_x3 ([hi | lo] input read as [hi | hi | lo], split
    output): both output halves bit-identical with the switch on and off.  139 pairs of 5 x 47 x 256 are the fewest
    the dispatcher sends to conv_igemm_p8: K = 9 * 768 >= 4096, so half a round of 256 x 256 tiles suffices, 128 of
    them = 32 513 pixels or more."""
    from cbw import _lib
    N, H, W, C, Cout = 139, 5, 47, 256, 256
    lib = _lib.load()
    d = torch.device("cuda:0")
    g = torch.Generator(device=d)
    g.manual_seed(32)
    x32 = torch.randn((N, H, W, C), generator=g, device=d)
    w32 = torch.randn((Cout, 3, 3, C), generator=g, device=d) / (9 * C) ** 0.5
    xh, wh = x32.to(torch.bfloat16), w32.to(torch.bfloat16)
    xl, wl = (x32 - xh.float()).to(torch.bfloat16), (w32 - wh.float()).to(torch.bfloat16)
    x = torch.cat([xh, xl], -1).contiguous()
    w = torch.cat([wh, wl, wh], -1).contiguous()
    b = torch.randn((Cout,), generator=g, device=d)
    M = N * H * W
    outs = []
    for mode in ("0", "1"):
        monkeypatch.setenv("CBW_P8_ROWSKIP", mode)
        y = torch.full((M, 2 * Cout), float("nan"), dtype=torch.bfloat16, device=d)
        y32 = torch.full((M, Cout), float("nan"), dtype=torch.float32, device=d)
        _lib.check(lib.cbw_conv2d_x3(x.data_ptr(), w.data_ptr(), b.data_ptr(), None, 0, y.data_ptr(), y32.data_ptr(), 1,
                                     N, H, W, C, Cout, 3, 1, 1, _lib.stream_handle()), "cbw_conv2d_x3")
        outs.append((y, y32))
    torch.cuda.synchronize()
    (y0, f0), (y1, f1) = outs
    assert torch.isfinite(y1.float()).all() and torch.isfinite(f1).all()
    assert torch.equal(y0[:, :Cout], y1[:, :Cout]) and torch.equal(y0[:, Cout:], y1[:, Cout:])
    assert torch.equal(f0, f1)
    ref = torch.nn.functional.conv2d(x32.permute(0, 3, 1, 2), w32.permute(0, 3, 1, 2), b, padding=1
                                     ).clamp_min(0).permute(0, 2, 3, 1).reshape(M, Cout)
    torch.testing.assert_close(f1, ref, rtol=0, atol=1e-2 * ref.abs().max().item())


def test_rowskip_classifier_bit_identical(monkeypatch):
    """The whole bf16 network: KwsEngine.classify on one 300-pair LEF chunk, logits bit-identical with the switch on
    and off."""
    from cbw.kws import KwsEngine
    hp = dict(n_layers=3, embedding_dim=128, learn_features=True, proj_mlp=True, frames_conv=True)
    eng = KwsEngine(hp, synth.synth_kws_state_dict(seed=4, **hp))
    g = torch.Generator(device=eng.device)
    g.manual_seed(33)
    maps = torch.rand((300, 3, 75, 750), generator=g, device=eng.device) * 2 - 1
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("CBW_P8_ROWSKIP", mode)
        out[mode] = eng.classify(maps, chunk=300)
    torch.cuda.synchronize()
    assert torch.isfinite(out["1"]).all()
    assert torch.equal(out["0"], out["1"]), (out["0"] - out["1"]).abs().max().item()
