"""Token-level timestamps on the GPU (cbw_align_matrix, cbw_dtw_dev, cbw.token_timestamps.
extract_token_timestamps_dev; include/cbw.h) against the host path they stand beside (extract_token_timestamps,
cbw_dtw) and the float64 restatement in tests/token_ts_ref.py, which tests/test_host_token_ts.py checks on the CPU.

The DTW is compared exactly: its arithmetic is cbw_dtw's.  The alignment matrix is compared with float64 under the
bound derived at test_matrix_against_float64.  The whole extraction is compared exactly with the host path on inputs
that tests/test_host_token_ts.py shows to be free of near-ties."""
import os

import numpy as np
import pytest
import torch

import token_ts_ref as R
from cbw import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTW_SHAPES = [(1, 1), (1, 7), (2, 1), (3, 5), (5, 3), (63, 65), (64, 64), (65, 63), (129, 300), (447, 1500)]
E2E_SHAPES = [(3, 33, 200), (6, 65, 400), (10, 129, 1500)]
E2E_CASES = [(7, "4.37", None, None), (7, "4.37", 300, None), (7, "5.x", None, 3), (7, "5.x", 300, 3),
             (3, "5.x", 300, 3), (1, "4.37", None, None)]     # (width, variant, num_frames, num_input_ids)
SENTINEL = -77


def _dtw_dev(m, path=True):
    """cbw_dtw_dev on a host f32 matrix -> (first_frame, text_idx, time_idx, len) as numpy, after asserting that
    nothing behind the outputs' and the workspace's ends was written"""
    from cbw import _lib
    lib = _lib.load()
    T, F = m.shape
    nb = lib.cbw_token_ts_ws_bytes(T, F)
    assert nb == 4 * T * -(-(T + F - 1) // 16)
    md = torch.from_numpy(m).to(DEV)
    ff = torch.full((T + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    ti = torch.full((T + F + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    tj = torch.full((T + F + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    ln = torch.full((4,), SENTINEL, dtype=torch.int32, device=DEV)
    ws = torch.full((nb + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(md.device):
        rc = lib.cbw_dtw_dev(md.data_ptr(), T, F, ff.data_ptr(), ti.data_ptr() if path else None,
                             tj.data_ptr() if path else None, ln.data_ptr() if path else None, ws.data_ptr(), nb,
                             _lib.stream_handle())
    assert rc == 0, lib.cbw_last_error()
    ff, ti, tj, ln, tail = ff.cpu().numpy(), ti.cpu().numpy(), tj.cpu().numpy(), ln.cpu().numpy(), ws[nb:].cpu().numpy()
    assert (ff[T:] == SENTINEL).all() and (ln[1:] == SENTINEL).all() and (tail == 0xA5).all()
    if not path:
        assert (ti == SENTINEL).all() and (tj == SENTINEL).all() and ln[0] == SENTINEL
        return ff[:T], None, None, None
    n = int(ln[0])
    assert 1 <= n <= T + F and (ti[n:] == SENTINEL).all() and (tj[n:] == SENTINEL).all()
    return ff[:T], ti[:n], tj[:n], n


@pytest.mark.parametrize("T,F", DTW_SHAPES)
def test_dtw_equals_host_dtw(T, F):
    """cbw_dtw_dev writes cbw_dtw's path for the same fp32 matrix, and first_frame is that path's jumps: on N(0, 1)
    values, and on values from {-1, 0, 1}, where every sum is exact and ties are everywhere, so that the order of the
    comparisons decides the path.  Twice the same; without the path pointers the same first_frame."""
    from cbw.token_timestamps import dtw
    g = np.random.default_rng(1000 * T + F)
    for m in (g.standard_normal((T, F)).astype(np.float32), g.integers(-1, 2, (T, F)).astype(np.float32)):
        want_ti, want_tj = dtw(m.astype(np.float64))
        ff, ti, tj, n = _dtw_dev(m)
        assert n == want_ti.size
        np.testing.assert_array_equal(ti, want_ti)
        np.testing.assert_array_equal(tj, want_tj)
        np.testing.assert_array_equal(ff, R.first_frames(want_ti, want_tj))
        again = _dtw_dev(m)
        assert all(np.array_equal(a, b) for a, b in zip((ff, ti, tj), again[:3])) and again[3] == n
        np.testing.assert_array_equal(_dtw_dev(m, path=False)[0], ff)


def _align_matrix(probs, n, t0, T, F, width):
    """cbw_align_matrix on a device tensor [n_all, T_all, 1500] -> (matrix [T, F] as numpy, flag)"""
    from cbw import _lib
    lib = _lib.load()
    T_all = probs.shape[1]
    nb = lib.cbw_token_ts_ws_bytes(T, F)
    out = torch.full((T * F + 8,), float("nan"), dtype=torch.float32, device=probs.device)
    flag = torch.full((4,), SENTINEL, dtype=torch.int32, device=probs.device)
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=probs.device)
    with torch.cuda.device(probs.device):
        rc = lib.cbw_align_matrix(probs.data_ptr(), n, T_all, t0, T, F, width, out.data_ptr(), flag.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _lib.stream_handle())
    assert rc == 0, lib.cbw_last_error()
    got, flag = out.cpu().numpy(), flag.cpu().numpy()
    assert np.isnan(got[T * F:]).all() and (flag[1:] == SENTINEL).all(), "wrote behind an output's end"
    return got[:T * F].reshape(T, F), int(flag[0])


def test_matrix_against_float64():
    """cbw_align_matrix against the float64 restatement for n in {1, 3, 10} heads, T in {2, 5, 65} positions at
    t0 in {0, 3}, F in {1, 3, 4, 7, 100, 1500} frames (3: the largest unfiltered F at width 7, 4: the smallest
    filtered one) and widths {1, 3, 7}, on softmax weights of N(0, 1) logits.

    Bound per element: (n + 3) 2^-24 A[t, f], A the largest |z| of the restatement over the heads and the filter window
    of the element.  The mean and the variance are float64 on both sides, so z = (float)((w - mean) / std) differs from
    the restatement's by its one rounding, at most 2^-24 |z| <= 2^-24 A; a median is one of its inputs and moves by at
    most the largest error among them, 2^-24 A; the n - 1 fp32 additions of the head sum round partial sums of at most
    k A, together at most (n^2 / 2) 2^-24 A before and (n / 2) 2^-24 A after the division by n; the division rounds
    once more, 2^-24 A: (n / 2 + 2) 2^-24 A in all to first order, and the bound leaves the other n / 2 + 1 units for the
    second-order terms.  The flag stays 0.  The largest error-to-bound ratio seen is printed: 0.381 on the MI355X, at
    n 3, T 65, t0 0, F 1500, width 1 (docs/MEASUREMENT_LOG.md)."""
    T_all = 68
    w = R.softmax_weights(10, T_all, 1500, seed=7)
    wd = torch.from_numpy(w).to(DEV)
    worst, where = 0.0, None
    for T in (2, 5, 65):
        for t0 in (0, 3):
            z_all = R.normalise(w[:, t0:t0 + T])
            for F in (1, 3, 4, 7, 100, 1500):
                z = z_all[..., :F]
                for width in (1, 3, 7):
                    med = R.median_filter(z, width)
                    for n in (1, 3, 10):
                        ref = -med[:n].mean(axis=0)
                        bound = (n + 3) * 2.0 ** -24 * R.window_absmax(z[:n], width)
                        got, flag = _align_matrix(wd, n, t0, T, F, width)
                        assert flag == 0, (n, T, t0, F, width)
                        err = np.abs(got.astype(np.float64) - ref)
                        ratio = float((err / bound).max())
                        if ratio > worst:
                            worst, where = ratio, (n, T, t0, F, width)
                        assert (err <= bound).all(), (f"n {n} T {T} t0 {t0} F {F} width {width}: err {err.max():.3g}, "
                                                      f"largest err / bound {ratio:.3g}")
    print(f"align matrix: largest error-to-bound ratio {worst:.3f} at (n, T, t0, F, width) = {where}")


def test_degenerate_flag_and_fallback():
    """A frame whose weight is the same at every used position has variance 0: the flag is set when that frame is among
    the first F, not otherwise, and extract_token_timestamps_dev then returns what extract_token_timestamps does."""
    from cbw.token_timestamps import extract_token_timestamps, extract_token_timestamps_dev
    w = R.softmax_weights(3, 20, 1500, seed=3)
    w[1, :, 150] = w[1, 0, 150]
    wd = torch.from_numpy(w).to(DEV)
    assert _align_matrix(wd, 3, 0, 20, 1500, 7)[1] != 0
    assert _align_matrix(wd, 3, 2, 18, 151, 3)[1] != 0
    assert _align_matrix(wd, 3, 0, 20, 150, 7)[1] == 0
    assert _align_matrix(wd, 1, 0, 20, 1500, 7)[1] == 0     # head 0 alone
    got = extract_token_timestamps_dev(wd, 7, 0.02, None, "4.37")
    want = extract_token_timestamps(wd, 7, 0.02, None, "4.37")
    assert torch.equal(got, want)
    assert torch.equal(extract_token_timestamps_dev(wd, 7, 0.02, 300, "5.x", 3),
                       extract_token_timestamps(wd, 7, 0.02, 300, "5.x", 3))


@pytest.mark.parametrize("n,T,F", E2E_SHAPES)
def test_extract_dev_equals_host_path(n, T, F):
    """extract_token_timestamps_dev == extract_token_timestamps (torch.equal) on weights with an alignment to find
    (tests/token_ts_ref.planted_weights; free of near-ties: tests/test_host_token_ts.py), for "4.37" and for "5.x" with
    3 input ids, num_frames None and 300, and for two narrower filters; with 1 position left, or width 9, the host path answers by construction."""
    from cbw.token_timestamps import extract_token_timestamps, extract_token_timestamps_dev
    w = torch.from_numpy(R.planted_weights(n, T, F, seed=T)).to(DEV)
    for width, variant, num_frames, n_in in E2E_CASES:
        got = extract_token_timestamps_dev(w, width, 0.02, num_frames, variant, n_in)
        want = extract_token_timestamps(w, width, 0.02, num_frames, variant, n_in)
        assert got.dtype == want.dtype and got.device == want.device
        assert torch.equal(got, want), (width, variant, num_frames, n_in, int((got != want).sum()))
    for args in [(w[:, :1], 7, 0.02, None, "4.37"), (w[:, :4], 7, 0.02, None, "5.x", 3), (w, 9, 0.02, None, "4.37")]:
        assert torch.equal(extract_token_timestamps_dev(*args), extract_token_timestamps(*args))
    with pytest.raises(ValueError, match="odd"):
        extract_token_timestamps_dev(w, 4)
    with pytest.raises(ValueError, match="unknown variant"):
        extract_token_timestamps_dev(w, 7, 0.02, None, "6.0")


def test_generate_with_and_without_the_device_path(golden_dir, monkeypatch):
    """generate(return_token_timestamps=True) on the long-form micro fixture with CBW_DEV_TOKEN_TS=1 and =0: the same
    sequences, and every window's token_timestamps torch.equal; the first run goes through the device function for
    every window and never falls back to the host one, the second never enters the device function."""
    import cbw.token_timestamps as tts
    from model.pba_whisper import PBAWhisper
    from test_gpu_decoder import micro_whisper_sd
    g = np.load(os.path.join(golden_dir, "longform_micro.npz"))
    w = PBAWhisper(synth.WHISPER_CONFIGS["micro"], synth.WHISPER_DECODERS["micro"], micro_whisper_sd(),
                   suppress_tokens=[1, 2, 7], max_initial_timestamp_index=50, alignment_heads=[[0, 1], [1, 0], [1, 1]])
    feats = torch.from_numpy(g["features"])[None].to(w.device)
    kw = dict(task="transcribe", language="en", return_timestamps=True, condition_on_prev_tokens=False,
              return_segments=True, num_beams=1, return_token_timestamps=True)
    calls = {"dev": 0, "host": 0}
    dev0, host0 = tts.extract_token_timestamps_dev, tts.extract_token_timestamps

    def dev(*a, **k):
        calls["dev"] += 1
        return dev0(*a, **k)

    def host(*a, **k):
        calls["host"] += 1
        return host0(*a, **k)
    monkeypatch.setattr(tts, "extract_token_timestamps_dev", dev)
    monkeypatch.setattr(tts, "extract_token_timestamps", host)

    def windows(res):
        out = []
        for s_ in res["segments"][0]:
            if not out or s_["result"] is not out[-1]:
                out.append(s_["result"])
        return out
    monkeypatch.setenv("CBW_DEV_TOKEN_TS", "1")
    on = w.generate(input_features=feats, **kw)
    assert calls["dev"] >= 1 and calls["host"] == 0, calls
    n_dev = calls["dev"]
    monkeypatch.setenv("CBW_DEV_TOKEN_TS", "0")
    off = w.generate(input_features=feats, **kw)
    assert calls["dev"] == n_dev and calls["host"] >= 1, calls
    assert torch.equal(on["sequences"], off["sequences"])
    a, b = windows(on), windows(off)
    assert len(a) == len(b) >= 1
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x["sequences"], y["sequences"])
        diff = (x["token_timestamps"] != y["token_timestamps"]).nonzero().flatten().tolist()
        assert torch.equal(x["token_timestamps"], y["token_timestamps"]), (k, diff)
