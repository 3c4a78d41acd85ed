"""The token-choice kernels of csrc/token_select.hip, each against float64 or the host's statement of the same rule:

* cbw_logprob_topk on both of its paths (two-stage by default, the one-pass kernel with CBW_TOPK_SPLIT=0) against float64
  log_softmax + bias.  The biases are 0 / -inf only, so the float64 order is exactly the order of the kernel's fp32 keys
  x + bias and the ids are compared exactly, no row left out for closeness; log-probs within 1e-4 (fp32 logsumexp of
  <= 51866 terms against float64; the bound of tests/test_gpu_decoder.py::test_logprob_topk_kernel_exact).
* cbw_timestamp_rules' values, not only its -inf pattern: -inf exactly where oracle.decoder.timestamp_mask says so on the
  float64 scores, bit-equal to the bias (or 0) elsewhere.  Its mass rule compares two fp32 numbers, so the inputs are
  chosen (and asserted, before any launch) to keep the float64 margin at least 0.01 away from 0 on every row.
* cbw_beam_select's state outputs (ts_state, st_out) against cbw.timestamps.TimestampRules.state.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def HISTORIES(TB):
    """the sampled tokens of test_gpu_decoder.py::test_timestamp_rules_kernel_vs_oracle's eight rows"""
    return [[], [TB + 3], [TB + 3, 17], [TB + 3, 17, TB + 9], [TB + 3, 17, TB + 9, TB + 9], [11, 12], [TB, TB],
            [TB + 2, 5, 6, TB + 2]]


SPLITS = [pytest.param(None, id="two-stage"), pytest.param("0", id="one-pass")]
EMPTY_ID = 0x7fffffff


def _set_split(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("CBW_TOPK_SPLIT", raising=False)
    else:
        monkeypatch.setenv("CBW_TOPK_SPLIT", split)


# ---------------------------------------------------------------- cbw_logprob_topk
TOPK_B, TOPK_KS = 3, (1, 5, 16)
# 1; fewer than k entries; 32 chunks of 2 with chunks 17-31 empty; one past a 1024-thread stride; one past the
# 8-in-flight stride; large-v3's vocabulary
TOPK_VS = (1, 5, 33, 1025, 8193, 51866)


@functools.lru_cache(maxsize=None)
def _topk_case(V):
    """Logits [B][ld] with ld > V (the padding holds values above every logit: a read past V would win), a tie at two
    adjacent ids of row 1, a shared bias and a per-row bias whose row 2 masks all but three tokens; for each bias the
    float64 reference log_softmax(x) + bias."""
    rng = np.random.default_rng(100 + V)
    ld = V + 7
    x = np.full((TOPK_B, ld), 100.0, np.float32)
    x[:, :V] = rng.standard_normal((TOPK_B, V)).astype(np.float32) * 3
    if V >= 2:
        x[1, V // 2 - 1] = x[1, V // 2] = 50.0
    shared = np.zeros(V, np.float32)
    if V >= 5:
        shared[[0, V // 2 - 1, V - 1]] = -np.inf   # the lower id of the tie among them
    rows = np.zeros((TOPK_B, V), np.float32)
    rows[0, :V // 3] = -np.inf
    rows[2, :] = -np.inf
    rows[2, [0, V // 2, V - 1]] = 0.0
    x64 = x[:, :V].astype(np.float64)
    m = x64.max(-1, keepdims=True)
    logp = x64 - (m + np.log(np.exp(x64 - m).sum(-1, keepdims=True)))
    return x, ld, {"shared": (shared, 0, logp + shared.astype(np.float64)),
                   "rows": (rows, V, logp + rows.astype(np.float64))}


def _run_topk(x, V, ld, bias, bias_ld, k):
    from cbw import _lib
    lib = _lib.load()
    d = torch.device("cuda:0")
    xd, bd = torch.from_numpy(x).to(d), torch.from_numpy(bias).to(d)
    lp = torch.full((TOPK_B, k), float("nan"), device=d)
    idx = torch.full((TOPK_B, k), -1, dtype=torch.int32, device=d)
    _lib.check(lib.cbw_logprob_topk(xd.data_ptr(), TOPK_B, V, ld, bd.data_ptr(), bias_ld, k, lp.data_ptr(),
                                    idx.data_ptr(), _lib.stream_handle()), "topk")
    return lp.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("V", TOPK_VS)
@pytest.mark.parametrize("split", SPLITS)
def test_logprob_topk_vs_float64(monkeypatch, split, V):
    _set_split(monkeypatch, split)
    x, ld, biases = _topk_case(V)
    for name, (bias, bias_ld, ref) in biases.items():
        for k in TOPK_KS:
            lp, idx = _run_topk(x, V, ld, bias, bias_ld, k)
            n = min(k, V)
            for r in range(TOPK_B):
                order = np.lexsort((np.arange(V), -ref[r]))[:n]
                what = f"{name} bias, k {k}, row {r}"
                assert idx[r, :n].tolist() == order.tolist(), what
                np.testing.assert_allclose(lp[r, :n], ref[r][order], atol=1e-4, rtol=0, err_msg=what)
                # fewer than k entries: the rest are empty slots
                assert idx[r, n:].tolist() == [EMPTY_ID] * (k - n), what
                assert np.all(np.isneginf(lp[r, n:])), what
    if V >= 5:   # the tie: the lower id is masked by the shared bias, first of the two under the per-row one
        assert _run_topk(x, V, ld, *biases["shared"][:2], 1)[1][1, 0] == V // 2
        assert _run_topk(x, V, ld, *biases["rows"][:2], 5)[1][1, :2].tolist() == [V // 2 - 1, V // 2]


@pytest.mark.parametrize("V", TOPK_VS)
def test_logprob_topk_paths_agree(monkeypatch, V):
    x, ld, biases = _topk_case(V)
    for name, (bias, bias_ld, _) in biases.items():
        for k in TOPK_KS:
            _set_split(monkeypatch, None)
            lp2, idx2 = _run_topk(x, V, ld, bias, bias_ld, k)
            _set_split(monkeypatch, "0")
            lp1, idx1 = _run_topk(x, V, ld, bias, bias_ld, k)
            assert idx1.tolist() == idx2.tolist(), f"{name} bias, k {k}"
            np.testing.assert_allclose(lp1, lp2, atol=2e-4, rtol=0, err_msg=f"{name} bias, k {k}")   # each within 1e-4


# ---------------------------------------------------------------- cbw_timestamp_rules
RULES_VS = (1030, 8193, 51865)
RULES_MAX_INITIAL = 50
RULES_MIN_MARGIN = 0.01


def _rules_ids(V):
    TB = V - 120
    return TB, TB - 1, TB - 107   # timestamp_begin, no_timestamps, eos


@functools.lru_cache(maxsize=None)
def _rules_case(V):
    """Logits for the eight histories and a bias with finite non-zero entries as well as -inf; per bias (given / NULL)
    the expected output and the float64 mass-rule margins."""
    from oracle.decoder import timestamp_mask, timestamp_mass_margin
    TB, NO_TS, EOS = _rules_ids(V)
    cases = HISTORIES(TB)
    rng = np.random.default_rng(7 + V)
    ld = V + 5
    x = rng.standard_normal((len(cases), ld)).astype(np.float32) * 4
    x[:, TB:V] -= rng.uniform(0, 8, (len(cases), 1)).astype(np.float32)
    bias = np.zeros(V, np.float32)
    finite = rng.choice(V, 64, replace=False)
    bias[finite] = (rng.standard_normal(64) * 2).astype(np.float32)
    bias[[1, 2, 7, TB + 4, V - 1]] = -np.inf
    out = {}
    for name, b in (("bias", bias), ("null", None)):
        b32 = bias if b is not None else np.zeros(V, np.float32)
        want = np.empty((len(cases), V), np.float32)
        margins = []
        for r, c in enumerate(cases):
            scores = x[r, :V].astype(np.float64) + b32.astype(np.float64)
            args = (c, TB, NO_TS, EOS, RULES_MAX_INITIAL)
            margins.append(timestamp_mass_margin(scores, *args))
            want[r] = np.where(np.isinf(timestamp_mask(scores, *args)), np.float32(-np.inf), b32)
        out[name] = (b, want, margins)
    return x, ld, cases, out


@pytest.mark.parametrize("V", RULES_VS)
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "null"])
def test_timestamp_rules_values(V, with_bias):
    from cbw import _lib
    from cbw.timestamps import TimestampRules
    TB, NO_TS, EOS = _rules_ids(V)
    x, ld, cases, out = _rules_case(V)
    bias, want, margins = out["bias" if with_bias else "null"]
    # the mass rule is one fp32 comparison: no row of the reference may sit close to it
    assert all(abs(m) >= RULES_MIN_MARGIN for m in margins), margins
    lib = _lib.load()
    d = torch.device("cuda:0")
    rules = TimestampRules(TB, NO_TS, EOS, RULES_MAX_INITIAL)
    st = torch.tensor([rules.state(c) for c in cases], dtype=torch.int32, device=d)
    xd = torch.from_numpy(x).to(d)
    bd = torch.from_numpy(bias).to(d) if with_bias else None
    got = torch.full((len(cases), V), float("nan"), device=d)
    _lib.check(lib.cbw_timestamp_rules(xd.data_ptr(), len(cases), V, ld, _lib.ptr(bd), st.data_ptr(), TB, NO_TS, EOS,
                                       RULES_MAX_INITIAL, got.data_ptr(), _lib.stream_handle()), "ts")
    got = got.cpu().numpy()
    for r, c in enumerate(cases):
        np.testing.assert_array_equal(got[r].view(np.uint32), want[r].view(np.uint32), err_msg=str(c))


# ---------------------------------------------------------------- cbw_beam_select's state outputs
def _history_state(h, tb):
    """ts_state of a row that sampled h: {n, last, second last, last timestamp} (-1: none), as _BeamWindow starts it"""
    ts = [t for t in h if t >= tb]
    return [len(h), h[-1] if h else -1, h[-2] if len(h) > 1 else -1, ts[-1] if ts else -1]


@pytest.mark.parametrize("count", [1, 0])
def test_beam_select_state_outputs(count):
    from cbw import _lib
    from cbw.timestamps import TimestampRules
    lib = _lib.load()
    d = torch.device("cuda:0")
    TB, NO_TS, EOS = 50364, 50363, 50257
    rules = TimestampRules(TB, NO_TS, EOS, 50)
    hist = HISTORIES(TB)
    B, k = len(hist), 16
    chosen = [TB + 1, 40, TB + 5, TB + 9, 41, 42, TB + 2, 43]   # half timestamps, half text, none EOS
    # beam r's only live candidate is its own slot 0 (score -r); every other candidate is 1000 below
    lp = torch.full((B, k), -1000.0)
    lp[:, 0] = 0.0
    idx = torch.arange(1000, 1000 + k, dtype=torch.int32).repeat(B, 1)
    idx[:, 0] = torch.tensor(chosen, dtype=torch.int32)
    scores = -torch.arange(B, dtype=torch.float64)
    lp, idx, scores = lp.to(d), idx.to(d), scores.to(d)
    ts_state = torch.tensor([_history_state(h, TB) for h in hist], dtype=torch.int32, device=d)
    st_out = torch.full((B, 4), -7, dtype=torch.int32, device=d)
    cand_score = torch.empty(k, dtype=torch.float64, device=d)
    cand_row, cand_tok = (torch.empty(k, dtype=torch.int32, device=d) for _ in range(2))
    tokens, parents = (torch.full((B,), -7, dtype=torch.int32, device=d) for _ in range(2))
    ok = torch.full((1,), -7, dtype=torch.int32, device=d)
    _lib.check(lib.cbw_beam_select(lp.data_ptr(), idx.data_ptr(), B, k, EOS, scores.data_ptr(), cand_score.data_ptr(),
                                   cand_row.data_ptr(), cand_tok.data_ptr(), tokens.data_ptr(), parents.data_ptr(),
                                   ok.data_ptr(), ts_state.data_ptr(), st_out.data_ptr(), TB, count,
                                   _lib.stream_handle()), "cbw_beam_select")
    assert ok.item() == 1
    assert parents.cpu().tolist() == list(range(B))
    assert tokens.cpu().tolist() == chosen
    assert scores.cpu().tolist() == [-float(r) for r in range(B)]
    after = [h + [t] if count else h for h, t in zip(hist, chosen)]
    assert ts_state.cpu().tolist() == [_history_state(h, TB) for h in after]
    assert st_out.cpu().tolist() == [list(rules.state(h)) for h in after]
