"""cbw_greedy_select alone against float64 numpy: the processors of HF's greedy loop (shared suppression bias, begin
suppression at a row's first free position, WhisperTimeStampLogitsProcessor = oracle.decoder.timestamp_mask), argmax
with ties to the lower id, log_softmax of the processed scores, and the per-row bookkeeping
(cbw.generate.greedy_select_state)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TB, NO_TS, EOS, MAX_INITIAL = 50364, 50363, 50257, 50
LD = 51968
HISTORIES = [[], [TB + 3], [TB + 3, 17], [TB + 3, 17, TB + 9], [TB + 3, 17, TB + 9, TB + 9], [11, 12], [TB, TB],
             [TB + 2, 5, 6, TB + 2]]


def _state(h):
    ts = [t for t in h if t >= TB]
    return [len(h), h[-1] if h else -1, h[-2] if len(h) > 1 else -1, ts[-1] if ts else -1]


def _reference(x, b, history, rules):
    """float64: (token, logprob, timestamp mass margin, top-two gap of the processed scores)"""
    from oracle.decoder import _logsumexp, timestamp_mask, timestamp_mass_margin
    s = x.astype(np.float64) + b
    margin = None
    if rules:
        with np.errstate(invalid="ignore"):
            margin = timestamp_mass_margin(s, history, TB, NO_TS, EOS, MAX_INITIAL)
            s = s + timestamp_mask(s, history, TB, NO_TS, EOS, MAX_INITIAL)
    tok = int(np.argmax(s))   # the first of equal maxima: the lower id
    top2 = np.partition(s, -2)[-2:]
    return tok, float(s[tok] - _logsumexp(s)), margin, float(top2[1] - top2[0])


@functools.lru_cache(maxsize=None)
def _cases(V):
    """The rows of the 16-row launch and of the rules-off launch, with their float64 references (computed once)."""
    rng = np.random.default_rng(1)   # the generator of test_timestamp_rules_kernel_vs_oracle
    x = rng.standard_normal((len(HISTORIES), LD)).astype(np.float32) * 4
    x[:, TB:V] -= rng.uniform(0, 8, (len(HISTORIES), 1)).astype(np.float32)
    bias = np.zeros(V, np.float32)
    bias[[1, 2, 7]] = -np.inf
    bias_begin = bias.copy()
    bias_begin[[220, EOS, TB + 5, 300]] = -np.inf
    rows = []   # (name, logits [LD], history, pos, limit, active on entry)
    for i, h in enumerate(HISTORIES):
        rows.append((f"history {h}", x[i], h, 10 + len(h), 100, 1))

    def variant(base, **cols):
        y = x[base].copy()
        for c, v in cols.items():
            y[int(c[1:])] = v
        return y
    rows.append(("begin: bias_begin suppresses the best timestamp", variant(0, **{f"c{TB + 5}": 30.0}), [], 3, 100, 1))
    rows.append(("after begin: bias, not bias_begin", variant(5, c300=30.0), [11, 12], 12, 100, 1))
    rows.append(("tie of two text logits", variant(5, c400=40.0, c900=40.0), [11, 12], 12, 100, 1))
    # the only timestamp left is V - 1 (floor = last timestamp + 1), so the mass margin of the tie is exactly 0: no
    # forcing, and the tie across the boundary goes to the text token
    rows.append(("tie across the text / timestamp boundary", variant(5, c500=40.0, **{f"c{V - 1}": 40.0}), [V - 2, 17], 12,
                 100, 1))
    rows.append(("EOS wins", variant(5, **{f"c{EOS}": 40.0}), [11, 12], 12, 100, 1))
    rows.append(("pos + 1 == limit", x[5].copy(), [11, 12], 20, 21, 1))
    rows.append(("inactive on entry", x[3].copy(), [TB + 3, 17, TB + 9], 30, 100, 0))
    g = x[2].copy()
    g[V:] = 100.0   # beyond V up to ld: would win if read
    rows.append(("garbage beyond V", g, [TB + 3, 17], 12, 100, 1))
    assert len(rows) == 16
    off = [("rules off", x[5].copy(), [11, 12], 12, 100, 1),
           ("rules off, begin", variant(0, c300=30.0, c301=29.0), [], 3, 100, 1),
           ("rules off, tie across the boundary", variant(5, c500=40.0, **{f"c{TB + 7}": 40.0}), [11, 12], 12, 100, 1)]

    def refs(rs, rules):
        return [_reference(r[1][:V], bias_begin if not r[2] else bias, r[2], rules) for r in rs]
    return bias, bias_begin, rows, refs(rows, True), off, refs(off, False)


def _launch(V, rows, bias, bias_begin, rules):
    from cbw import _lib
    lib = _lib.load()
    d = torch.device("cuda:0")
    B = len(rows)
    xd = torch.from_numpy(np.stack([r[1] for r in rows])).to(d)
    ts_state = torch.tensor([_state(r[2]) for r in rows], dtype=torch.int32, device=d)
    pos = torch.tensor([r[3] for r in rows], dtype=torch.int32, device=d)
    limit = torch.tensor([r[4] for r in rows], dtype=torch.int32, device=d)
    active = torch.tensor([r[5] for r in rows], dtype=torch.int32, device=d)
    tokens = torch.full((B,), -7, dtype=torch.int32, device=d)
    logprob = torch.full((B,), 123.0, dtype=torch.float32, device=d)
    bd, bbd = torch.from_numpy(bias).to(d), torch.from_numpy(bias_begin).to(d)
    _lib.check(lib.cbw_greedy_select(xd.data_ptr(), B, V, LD, bd.data_ptr(), bbd.data_ptr(), TB if rules else -1, NO_TS, EOS,
                                     MAX_INITIAL, ts_state.data_ptr(), pos.data_ptr(), limit.data_ptr(),
                                     active.data_ptr(), tokens.data_ptr(), logprob.data_ptr(), _lib.stream_handle()),
               "cbw_greedy_select")
    torch.cuda.synchronize()
    return tokens.cpu().tolist(), logprob.cpu().numpy(), ts_state.cpu().tolist(), active.cpu().tolist()


def _compare(rows, refs, got, rules):
    from cbw.generate import greedy_select_state
    tokens, logprob, ts_state, active = got
    for r, (row, ref) in enumerate(zip(rows, refs)):
        name, _, h, pos, limit, act = row
        tok, lp, _, _ = ref
        print(f"{name}: token {tokens[r]} (ref {tok}) logprob {logprob[r]:.6f} (ref {lp:.6f}) active {active[r]}")
        if not act:
            assert tokens[r] == EOS and ts_state[r] == _state(h) and active[r] == 0 and logprob[r] == 123.0, name
            continue
        st, a = greedy_select_state(_state(h), tok, pos, limit, EOS, TB if rules else -1)
        assert tokens[r] == tok, name
        assert ts_state[r] == st, name
        assert active[r] == a, name
        assert abs(float(logprob[r]) - lp) <= 1e-4, name


def _assert_reference_margins(V):
    """The float64 reference decides every history row well outside float32's reach: the timestamp mass rule by at
    least 2.4 (or infinitely), the argmax by at least 0.027 over the runner-up (to the three decimals that figure is
    stated with: the smallest gap, history [TB + 3, 17, TB + 9, TB + 9], is 0.0269985 -- some 10^4 float32 ulps of the
    scores)."""
    _, _, rows, refs, _, _ = _cases(V)
    for (name, *_), (_, _, margin, gap) in list(zip(rows, refs))[:len(HISTORIES)]:
        assert np.isinf(margin) or abs(margin) >= 2.4, (name, margin)
        assert round(gap, 3) >= 0.027, (name, gap)


@pytest.mark.parametrize("V", [51865, 51866])
def test_greedy_select_one_row_launches(V):
    """B = 1: each of the eight histories on its own."""
    bias, bias_begin, rows, refs, _, _ = _cases(V)
    _assert_reference_margins(V)
    for i in range(len(HISTORIES)):
        _compare(rows[i:i + 1], refs[i:i + 1], _launch(V, rows[i:i + 1], bias, bias_begin, True), True)


@pytest.mark.parametrize("V", [51865, 51866])
def test_greedy_select_sixteen_rows_in_one_launch(V):
    """B = 16: the eight histories and the extra rows (begin suppression, ties, EOS, the limit, an inactive row,
    garbage beyond V) in one launch."""
    bias, bias_begin, rows, refs, _, _ = _cases(V)
    _assert_reference_margins(V)
    by_name = {r[0]: ref for r, ref in zip(rows, refs)}
    assert by_name["begin: bias_begin suppresses the best timestamp"][0] != TB + 5
    assert by_name["after begin: bias, not bias_begin"][0] == 300
    assert by_name["tie of two text logits"][0] == 400
    assert by_name["tie across the text / timestamp boundary"][0] == 500
    assert by_name["tie across the text / timestamp boundary"][2] == 0.0
    assert by_name["EOS wins"][0] == EOS
    got = _launch(V, rows, bias, bias_begin, True)
    _compare(rows, refs, got, True)
    assert got[3][rows.index(next(r for r in rows if r[0] == "EOS wins"))] == 0
    assert got[3][rows.index(next(r for r in rows if r[0] == "pos + 1 == limit"))] == 0


@pytest.mark.parametrize("V", [51865, 51866])
def test_greedy_select_rules_off(V):
    """timestamp_begin < 0: only the shared biases (bias_begin at a row's first position), every token one class."""
    bias, bias_begin, _, _, off, refs = _cases(V)
    assert refs[1][0] == 301 and refs[2][0] == 500   # 300 is begin-suppressed; the tie goes to the lower id
    _compare(off, refs, _launch(V, off, bias, bias_begin, False), False)


def test_greedy_select_refuses_bad_arguments():
    from cbw import _lib
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    p = t.data_ptr()
    ok = [p, 1, 8, 8, None, None, -1, -1, 0, -1, p, p, p, p, p, p, _lib.stream_handle()]
    for i, v in [(0, None), (10, None), (11, None), (12, None), (13, None), (14, None), (15, None), (1, 0), (1, 17),
                 (2, 0), (3, 7)]:
        args = list(ok)
        args[i] = v
        assert lib.cbw_greedy_select(*args) == -1, (i, v)
