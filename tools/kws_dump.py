"""Dump what the KWS host code decides, for a byte comparison of two builds of libcbw.so.

    CBW_LIB=/path/to/libcbw.so python tools/kws_dump.py OUT_DIR

Run it once per library, each in a fresh process (CBW_LIB is read when cbw._lib is imported), then `diff -r` the two
directories: a refactor of the runtime's host side must leave every file byte-equal.  Per configuration it writes, as
.npy files under OUT_DIR/<configuration>/:

  score, rescore_fp32, rescore_x3      logits of the 5 keywords against utterance 0 (chunk = 4: one full chunk and one
                                       partial), and both re-scoring tiers over all five
  bias_offset, score_calibrated        calibrate_bias over all five pairs: the returned offset, the logits after it
  score_restored                       the logits after the no-argument calibrate_bias()
  fp8_scales, fp8_offset, score_fp8    ResNet-50 only: calibrate_fp8(margin = 1.0)
  profile_score_*, profile_x3_*        ResNet-50 only: kernel names, FLOPs and tiers of the launch-profile records of
                                       one score call and one x3 rescore call
  workspace                            int64 [3][4]: at (Tk, Tu) = (15, 50), (30, 100) and (150, 1500) the bytes of
                                       cbw_kws_workspace_bytes with chunk 4 and 1112, cbw_kws_rescore_workspace_bytes
                                       and cbw_kws_rescore_x3_workspace_bytes

Configurations: LEF (proj_mlp_units 64, embedding_dim 128, 3 layers) on ResNet-18 / 34 / 50 at Tk = 15, Tu = 50 after
the frame pooling (30 and 100 feature frames in), and the L variant (raw 32-wide features) on ResNet-18 at the same
Tk, Tu: the shapes of tests/test_gpu_kws_pairs.py and tests/test_gpu_kws_tiers.py, which every conv shape class of the
three depths and both block kinds pass through in seconds.
"""
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
from cbw import _lib, synth  # noqa: E402
from cbw.kws import KwsEngine  # noqa: E402

L, K, D, CHUNK, CAP = 3, 5, 128, 4, 256
LEF = dict(n_layers=L, embedding_dim=D, learn_features=True, proj_mlp=True, frames_conv=True, proj_mlp_units=64)
# name: (hparams, classifier_only, utterance frames, keyword frames)
CONFIGS = {
    "LEF64-r18": (dict(LEF, resnet_version="resnet-18"), False, 100, 30),
    "LEF64-r34": (dict(LEF, resnet_version="resnet-34"), False, 100, 30),
    "LEF64-r50": (dict(LEF, resnet_version="resnet-50"), False, 100, 30),
    # the state dict is a LEF one (its projector goes unused): only that form names a ResNet-18
    "L32-r18": (dict(LEF, embedding_dim=32, resnet_version="resnet-18"), True, 50, 15),
}


def features():
    """The seeded batch of tests/test_gpu_kws_tiers.py: one utterance, five keywords, keyword 4 planted in it."""
    g = np.random.Generator(np.random.PCG64(77))
    utt = synth.l2n(g.standard_normal((1, L, 100, D)).astype(np.float32))
    kwd = synth.l2n(g.standard_normal((K, L, 30, D)).astype(np.float32))
    utt[0, :, 20:50] = synth.l2n(kwd[4] + 0.3 * g.standard_normal((L, 30, D)).astype(np.float32))
    return utt, kwd


def profile(eng, call):
    """(kernel names, FLOPs, tiers) of the launch-profile records of one call."""
    lib = eng.lib
    _lib.check(lib.cbw_kws_profile(eng.h, CAP), "cbw_kws_profile")
    call()
    torch.cuda.synchronize()
    st, en, fl = (np.zeros(CAP) for _ in range(3))
    tiers = np.full(CAP, -1, np.int32)
    names = (ctypes.c_char_p * CAP)()
    n = lib.cbw_kws_profile_records(eng.h, st.ctypes.data, en.ctypes.data, fl.ctypes.data, CAP)
    lib.cbw_kws_profile_tiers(eng.h, tiers.ctypes.data, CAP)
    lib.cbw_kws_profile_kernels(eng.h, names, CAP)
    lib.cbw_kws_profile(eng.h, 0)
    assert 0 < n < CAP
    return np.array([names[i] or b"" for i in range(n)], dtype="S96"), fl[:n].copy(), tiers[:n].copy()


def dump(name, out_dir):
    hp, classifier_only, t_utt, t_kwd = CONFIGS[name]
    os.makedirs(out_dir, exist_ok=True)

    def save(what, a):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        np.save(os.path.join(out_dir, what + ".npy"), np.ascontiguousarray(a))

    eng = KwsEngine(hp, synth.synth_kws_state_dict(seed=3, **hp), classifier_only=classifier_only)
    d = eng.device
    utt, kwd = features()
    E = hp["embedding_dim"]
    utt = torch.from_numpy(np.ascontiguousarray(synth.l2n(utt[:, :, :t_utt, :E]))).to(d)
    kwd = torch.from_numpy(np.ascontiguousarray(synth.l2n(kwd[:, :, :t_kwd, :E]))).to(d)
    um, km = torch.ones((1, L, t_utt), device=d), torch.ones((K, L, t_kwd), device=d)
    pu, pum = eng.project(utt, um)
    pk, pkm = eng.project(kwd, km)
    pu32, _ = eng.project_f32(utt, um)
    pk32, _ = eng.project_f32(kwd, km)
    pu, pum, pu32 = pu[0], pum[0], pu32[0]
    Tk, Tu = pk.shape[2], pu.shape[1]
    assert (Tk, Tu) == (15, 50)
    everyone = torch.arange(K, dtype=torch.int32, device=d)

    score = eng.score(pu, pum, pk, pkm, chunk=CHUNK)
    save("score", score)
    for tier in ("fp32", "x3"):
        save("rescore_" + tier, eng.rescore(pu32, pum, pk32, pkm, score.clone(), everyone, tier=tier))
    save("bias_offset", eng.calibrate_bias(pu32, pum, pk32, pkm, sel=everyone, utt=pu, kwd=pk))
    save("score_calibrated", eng.score(pu, pum, pk, pkm, chunk=CHUNK))
    eng.calibrate_bias()
    save("score_restored", eng.score(pu, pum, pk, pkm, chunk=CHUNK))
    if hp["resnet_version"] == "resnet-50":
        save("fp8_offset", eng.calibrate_fp8(pu32, pum, pk32, pkm, margin=1.0, utt=pu, kwd=pk))
        save("fp8_scales", eng.fp8_scales())
        save("score_fp8", eng.score_fp8(pu, pum, pk, pkm, chunk=CHUNK))
        calls = {"score": lambda: eng.score(pu, pum, pk, pkm, chunk=CHUNK),
                 "x3": lambda: eng.rescore(pu32, pum, pk32, pkm, score.clone(), everyone, tier="x3")}
        for what, call in calls.items():
            names, flops, tiers = profile(eng, call)
            save(f"profile_{what}_kernels", names)
            save(f"profile_{what}_flops", flops)
            save(f"profile_{what}_tiers", tiers)
    lib = eng.lib
    save("workspace", np.array([[lib.cbw_kws_workspace_bytes(eng.h, tk, tu, 4),
                                 lib.cbw_kws_workspace_bytes(eng.h, tk, tu, 1112),
                                 lib.cbw_kws_rescore_workspace_bytes(eng.h, tk, tu),
                                 lib.cbw_kws_rescore_x3_workspace_bytes(eng.h, tk, tu)]
                                for tk, tu in ((Tk, Tu), (30, 100), (150, 1500))], dtype=np.int64))
    torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    _lib.require_gpu()
    print("library:", _lib.LIB_PATH, _lib.load().cbw_source_id().decode())
    for cfg in CONFIGS:
        dump(cfg, os.path.join(sys.argv[1], cfg))
        print("dumped", cfg)
