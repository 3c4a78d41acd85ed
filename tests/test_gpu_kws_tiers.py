"""The basic-block networks (ResNet-18 / 34) through the re-scoring and calibration paths, and the workspace sizes of
all three depths: every tier's network, the bias restore and the planners are built from one topology
(resnet_topology in csrc/runtime.cpp), and the other GPU tests reach calibrate_bias and the compensated tier on
ResNet-50 only.

Shapes: LEF, proj_mlp_units 64, embedding_dim 128, L = 3, K = 5 keywords of 30 feature frames against one utterance of
100 (Tk = 15, Tu = 50 after the frame pooling: neither a multiple of the 16-frame tile), chunk = 4 (one full chunk and
one partial).  The features are those tools/kws_dump.py writes its byte-comparison files from.
"""
import numpy as np
import pytest
import torch

from cbw import synth

pytestmark = pytest.mark.gpu

L, K, D, T_UTT, T_KWD, CHUNK = 3, 5, 128, 100, 30, 4
BAND_X3 = 1e-4   # tests/test_gpu_exact.py:26, the width bench.py's second band assumes.  Largest |p_x3 - p_fp32| of the
                 # build before the shared topology at these shapes: ResNet-18 1.3e-6, ResNet-34 1.6e-6
                 # (docs/MEASUREMENT_LOG.md)
RESCORE_RTOL = 1e-4   # tests/test_gpu_exact.py:106: re-scored pairs within 1e-4 of max |logit| of the float64 oracle

# bytes of [cbw_kws_workspace_bytes chunk 4, chunk 1112, cbw_kws_rescore_workspace_bytes,
# cbw_kws_rescore_x3_workspace_bytes] per (Tk, Tu), from the build before the two planners were merged
# (tools/kws_dump.py, default CBW_KWS_STREAMS and CBW_X3_CHUNK)
WORKSPACE = {
    "resnet-18": {(15, 50): [1153536, 320630016, 4056320, 71716864],
                  (30, 100): [4358400, 1211635200, 15488000, 274022400],
                  (150, 1500): [324576000, 90232128000, 1130880000, 19961856000]},
    "resnet-34": {(15, 50): [1153536, 320630016, 4056320, 71716864],
                  (30, 100): [4358400, 1211635200, 15488000, 274022400],
                  (150, 1500): [324576000, 90232128000, 1130880000, 19961856000]},
    "resnet-50": {(15, 50): [1350144, 375287040, 8742144, 167137280],
                  (30, 100): [5203200, 1446489600, 33510400, 641024000],
                  (150, 1500): [371808000, 103362624000, 2414976000, 46110720000]},
}


def _hp(version):
    return dict(n_layers=L, embedding_dim=D, learn_features=True, proj_mlp=True, frames_conv=True, proj_mlp_units=64,
                resnet_version=version)


@pytest.fixture(scope="module")
def batch():
    """Seeded features in the dataset contract (L2-normalised frames, all frames valid), keyword 4 planted in the
    utterance; shared and never modified."""
    g = np.random.Generator(np.random.PCG64(77))
    utt = synth.l2n(g.standard_normal((1, L, T_UTT, D)).astype(np.float32))
    kwd = synth.l2n(g.standard_normal((K, L, T_KWD, D)).astype(np.float32))
    utt[0, :, 20:20 + T_KWD] = synth.l2n(kwd[4] + 0.3 * g.standard_normal((L, T_KWD, D)).astype(np.float32))
    return dict(utt=utt, kwd=kwd, utt_mask=np.ones((1, L, T_UTT), np.float32),
                kwd_mask=np.ones((K, L, T_KWD), np.float32))


_cache = {}


def engine(version):
    if version not in _cache:
        from cbw.kws import KwsEngine
        hp = _hp(version)
        _cache[version] = KwsEngine(hp, synth.synth_kws_state_dict(seed=3, **hp))
    return _cache[version]


def projections(eng, batch):
    d = eng.device
    utt, um = torch.from_numpy(batch["utt"]).to(d), torch.from_numpy(batch["utt_mask"]).to(d)
    kwd, km = torch.from_numpy(batch["kwd"]).to(d), torch.from_numpy(batch["kwd_mask"]).to(d)
    pu, pum = eng.project(utt, um)
    pk, pkm = eng.project(kwd, km)
    pu32, _ = eng.project_f32(utt, um)
    pk32, _ = eng.project_f32(kwd, km)
    assert tuple(pk.shape) == (K, L, 15, 64) and tuple(pu.shape) == (1, L, 50, 64)
    return pu[0], pum[0], pk, pkm, pu32[0], pk32


def _prob(lg):
    return torch.softmax(lg.double(), -1)[:, 1].cpu().numpy()


@pytest.mark.parametrize("version", ["resnet-18", "resnet-34"])
def test_basic_block_networks_rescore_and_calibrate(version, batch):
    import oracle.kws as okws
    eng = engine(version)
    pu, pum, pk, pkm, pu32, pk32 = projections(eng, batch)
    everyone = torch.arange(K, dtype=torch.int32, device=eng.device)

    before = eng.score(pu, pum, pk, pkm, chunk=CHUNK)
    assert torch.isfinite(before).all()

    # fp32 re-scoring of all five pairs against the float64 oracle
    hp = _hp(version)
    ref, _ = okws.kws_forward(synth.synth_kws_state_dict(seed=3, **hp), hp, batch["kwd"], batch["utt"],
                              batch["kwd_mask"], batch["utt_mask"], return_features=False)
    full = eng.rescore(pu32, pum, pk32, pkm, before.clone(), everyone)
    err32 = np.abs(full.cpu().numpy() - ref).max()
    print(f"{version}: max |fp32 rescore - oracle| = {err32:.3g}, bound {RESCORE_RTOL * np.abs(ref).max():.3g}")
    assert err32 < RESCORE_RTOL * np.abs(ref).max()

    # the compensated tier against the fp32 tier, in probabilities
    x3 = eng.rescore(pu32, pum, pk32, pkm, before.clone(), everyone, tier="x3")
    err3 = np.abs(_prob(x3) - _prob(full)).max()
    print(f"{version}: max |p_x3 - p_fp32| = {err3:.3g}, max |dlogit| = {float((x3 - full).abs().max()):.3g}")
    assert err3 < BAND_X3

    # bias calibration over all five pairs moves the biases; the no-argument form puts back exactly finalize's
    off = eng.calibrate_bias(pu32, pum, pk32, pkm, sel=everyone, utt=pu, kwd=pk)
    calibrated = eng.score(pu, pum, pk, pkm, chunk=CHUNK)
    eng.calibrate_bias()
    restored = eng.score(pu, pum, pk, pkm, chunk=CHUNK)
    print(f"{version}: offset {off.tolist()}, max |calibrated - before| = "
          f"{float((calibrated - before).abs().max()):.3g}, max |restored - before| = "
          f"{float((restored - before).abs().max()):.3g}")
    assert off.shape == (2,) and np.isfinite(off).all() and not torch.equal(calibrated, before)
    np.testing.assert_allclose(restored.cpu().numpy(), before.cpu().numpy(), rtol=0, atol=0)


@pytest.mark.parametrize("version", list(WORKSPACE))
def test_workspace_bytes_table(version, monkeypatch):
    monkeypatch.delenv("CBW_KWS_STREAMS", raising=False)
    eng = engine(version)
    lib = eng.lib
    for (tk, tu), want in WORKSPACE[version].items():
        got = [lib.cbw_kws_workspace_bytes(eng.h, tk, tu, 4), lib.cbw_kws_workspace_bytes(eng.h, tk, tu, 1112),
               lib.cbw_kws_rescore_workspace_bytes(eng.h, tk, tu),
               lib.cbw_kws_rescore_x3_workspace_bytes(eng.h, tk, tu)]
        print(f"{version} ({tk}, {tu}): {got}")
        assert got == want, f"{version} at ({tk}, {tu})"
