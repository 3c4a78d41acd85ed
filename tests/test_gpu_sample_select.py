"""cbw_sample_select alone against float64 numpy: the processed scores of cbw_greedy_select (shared suppression bias,
begin suppression, WhisperTimeStampLogitsProcessor = oracle.decoder.timestamp_mask), the top-k kept set by
s >= kth (exact), torch.multinomial's exponential race over it with injected noise q
(token = argmax of s / T - ln q), logprob = s[token] - logsumexp(kept s), and the per-row bookkeeping
(cbw.generate.greedy_select_state).  The logits, histories and biases are those of test_gpu_greedy_select.py.

The float64 race decides every row by a key gap >= 1e-2 (asserted before any launch; the noise seeds below were chosen
on the CPU so that it holds): more than 10^3 float32 ulps of the largest key, about 85 at T = 0.2 for these logits."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_greedy_select import EOS, HISTORIES, LD, MAX_INITIAL, NO_TS, TB, _state
from test_gpu_greedy_select import _cases as _greedy_cases

pytestmark = pytest.mark.gpu

FLT_MIN = float(np.finfo(np.float32).tiny)
TEMPERATURES = [0.2, 1.0]
# noise seed per (group of rows, V, T), chosen on the CPU: the first seed from 0 on with which every row of the group
# meets the key gap and the constructed rows' conditions below
NOISE_SEEDS = {(group, V, 1.0): 1 for group in ("histories", "sixteen", "rules off") for V in (51865, 51866)}


def _reference(x, b, q, history, rules, T, top_k):
    """float64: (token, logprob, kept mask, key gap of the race, timestamp mass margin, number of finite scores)"""
    from oracle.decoder import _logsumexp, timestamp_mask, timestamp_mass_margin
    s = x.astype(np.float64) + b
    margin = None
    if rules:
        with np.errstate(invalid="ignore"):
            margin = timestamp_mass_margin(s, history, TB, NO_TS, EOS, MAX_INITIAL)
            s = s + timestamp_mask(s, history, TB, NO_TS, EOS, MAX_INITIAL)
    finite = s > -np.inf
    if not finite.any():
        return EOS, -np.inf, finite, np.inf, margin, 0
    ranked = np.sort(s[finite])[::-1]
    kth = ranked[min(top_k, len(ranked)) - 1]   # the top_k-th largest finite score; fewer: the smallest finite one
    kept = finite & (s >= kth)
    q = q.astype(np.float64)
    q = np.where((q > 0) & np.isfinite(q), q, FLT_MIN)
    key = np.where(kept, s / T - np.log(q), -np.inf)
    tok = int(np.argmax(key))
    top2 = np.partition(key, -2)[-2:]
    return tok, float(s[tok] - _logsumexp(s[kept])), kept, float(top2[1] - top2[0]), margin, int(finite.sum())


def _ranked_ids(x, b):
    """token ids of a rules-free text row by descending score"""
    s = x.astype(np.float64) + b
    return np.argsort(-s, kind="stable")


def _build(V, T, group, seed):
    """(bias, bias_begin, rows, rules, top_k) of one launch group; rows = (name, logits [LD], history, pos, limit,
    active on entry, noise [LD]); every row has garbage beyond V in its logits (would win if read) and in its noise
    (1e-30: would win if read with a pitch of V)."""
    bias, bias_begin, grows, _, _, _ = _greedy_cases(V)
    x = [r[1].copy() for r in grows[:len(HISTORIES)]]
    for y in x:
        y[V:] = 100.0
    rng = np.random.default_rng(seed)
    rows = []

    def add(name, y, h, pos, limit, act=1, **noise):
        q = rng.exponential(size=LD).astype(np.float32)
        q[V:] = 1e-30
        for c, v in noise.items():
            q[int(c[1:])] = v
        rows.append((name, y, h, pos, limit, act, q))

    def variant(base, **cols):
        y = x[base].copy()
        for c, v in cols.items():
            y[int(c[1:])] = v
        return y
    rules, top_k = group != "rules off", {"top_k 1": 1, "top_k >= V": 60000}.get(group, 50)
    if group in ("histories", "rules off", "top_k 1", "top_k >= V"):
        for i, h in enumerate(HISTORIES):
            add(f"history {h}", x[i], h, 10 + len(h), 100)
    if group == "histories":
        order = _ranked_ids(x[5][:V], bias)
        add("pos + 1 == limit", x[5].copy(), [11, 12], 20, 21)
        add("q of 0 reads as FLT_MIN", x[5].copy(), [11, 12], 12, 100, **{f"c{order[49]}": 0.0})
    if group == "sixteen":
        for i, h in enumerate(HISTORIES):
            add(f"history {h}", x[i], h, 10 + len(h), 100)
        order = _ranked_ids(x[5][:V], bias)   # history [11, 12]: the rules mask no text token but <|notimestamps|>
        a, b51 = int(order[49]), int(order[50])
        j = 40000 if a != 40000 else 40001
        add("two equal scores at kth", variant(5, **{f"c{j}": x[5][a]}), [11, 12], 12, 100, **{f"c{j}": 1e-30})
        add("the lowest kept token wins with a tiny q", x[5].copy(), [11, 12], 12, 100, **{f"c{a}": 1e-30})
        add("a tiny q just outside the top-k", x[5].copy(), [11, 12], 12, 100, **{f"c{b51}": 1e-30})
        ts = {f"c{TB + 10 + i}": v for i, v in enumerate((25.0, 24.8, 24.6, 24.5, 24.3))}
        add("the mass rule forces a timestamp", variant(5, **ts), [11, 12], 12, 100,
            **{f"c{TB + 10 + i}": (1e-3 if i == 2 else 1.0) for i in range(5)})
        add("begin: bias_begin suppresses the best timestamp", variant(0, **{f"c{TB + 5}": 30.0}), [], 3, 100,
            **{f"c{TB + 5}": 1e-30})
        add("after begin: bias, not bias_begin", variant(5, c300=30.0), [11, 12], 12, 100)
        add("EOS drawn", variant(5, **{f"c{EOS}": 40.0}), [11, 12], 12, 100, **{f"c{EOS}": 1e-3})
        add("inactive on entry", x[3].copy(), [TB + 3, 17, TB + 9], 30, 100, act=0)
        assert len(rows) == 16
    return bias, bias_begin, rows, rules, top_k


@functools.lru_cache(maxsize=None)
def _cases(V, T, group, seed=None):
    """One launch group with its float64 references (computed once); asserts what the rows are there to show and that
    the reference decides every row outside float32's reach."""
    if seed is None:
        seed = NOISE_SEEDS.get((group, V, T), 0)
    bias, bias_begin, rows, rules, top_k = _build(V, T, group, seed)
    refs = [_reference(r[1][:V], bias_begin if not r[2] else bias, r[6][:V], r[2], rules, T, top_k) for r in rows]
    by = {r[0]: (r, ref) for r, ref in zip(rows, refs)}
    for (name, _, _, _, _, act, _), (tok, lp, kept, gap, margin, n_finite) in zip(rows, refs):
        if not act:
            continue
        assert gap >= 1e-2, (name, gap)
        assert margin is None or np.isinf(margin) or abs(margin) >= 2.4, (name, margin)
        assert 0 <= tok < V and kept[tok] and np.isfinite(lp), name
        if group == "top_k 1":
            assert kept.sum() == 1
        elif group == "top_k >= V":
            assert kept.sum() == n_finite >= 50   # every finite score
        else:
            assert kept.sum() == (51 if name == "two equal scores at kth" else 50), (name, kept.sum())
    if group == "histories":
        (r, ref) = by["q of 0 reads as FLT_MIN"]
        assert r[6][ref[0]] == 0.0
    if group == "sixteen":
        order = _ranked_ids(by["history [11, 12]"][0][1][:V], bias)
        a, b51 = int(order[49]), int(order[50])
        assert by["two equal scores at kth"][1][0] in (40000, 40001)
        assert by["the lowest kept token wins with a tiny q"][1][0] == a
        ref = by["a tiny q just outside the top-k"][1]
        assert not ref[2][b51] and ref[0] != b51
        ref = by["the mass rule forces a timestamp"][1]
        assert ref[0] == TB + 12 and ref[4] >= 2.4 and not ref[2][:TB].any()
        ref = by["begin: bias_begin suppresses the best timestamp"][1]
        assert not ref[2][TB + 5] and ref[0] >= TB
        assert by["after begin: bias, not bias_begin"][1][2][300]
        assert by["EOS drawn"][1][0] == EOS
    return bias, bias_begin, rows, refs, rules, top_k


def _launch(V, rows, bias, bias_begin, rules, T, top_k):
    from cbw import _lib
    lib = _lib.load()
    d = torch.device("cuda:0")
    B = len(rows)
    xd = torch.from_numpy(np.stack([r[1] for r in rows])).to(d)
    qd = torch.from_numpy(np.stack([r[6] for r in rows])).to(d)
    ts_state = torch.tensor([_state(r[2]) for r in rows], dtype=torch.int32, device=d)
    pos = torch.tensor([r[3] for r in rows], dtype=torch.int32, device=d)
    limit = torch.tensor([r[4] for r in rows], dtype=torch.int32, device=d)
    active = torch.tensor([r[5] for r in rows], dtype=torch.int32, device=d)
    tokens = torch.full((B,), -7, dtype=torch.int32, device=d)
    logprob = torch.full((B,), 123.0, dtype=torch.float32, device=d)
    bd, bbd = torch.from_numpy(bias).to(d), torch.from_numpy(bias_begin).to(d)
    _lib.check(lib.cbw_sample_select(xd.data_ptr(), B, V, LD, bd.data_ptr(), bbd.data_ptr(), TB if rules else -1, NO_TS, EOS,
                                     MAX_INITIAL, ts_state.data_ptr(), pos.data_ptr(), limit.data_ptr(),
                                     active.data_ptr(), tokens.data_ptr(), logprob.data_ptr(), T, top_k, qd.data_ptr(), LD,
                                     _lib.stream_handle()), "cbw_sample_select")
    torch.cuda.synchronize()
    return tokens.cpu().tolist(), logprob.cpu().numpy(), ts_state.cpu().tolist(), active.cpu().tolist()


def _compare(rows, refs, got, rules):
    from cbw.generate import greedy_select_state
    tokens, logprob, ts_state, active = got
    for r, (row, ref) in enumerate(zip(rows, refs)):
        name, _, h, pos, limit, act, _ = row
        tok, lp = ref[0], ref[1]
        print(f"{name}: token {tokens[r]} (ref {tok}) logprob {logprob[r]:.6f} (ref {lp:.6f}) active {active[r]} "
              f"key gap {ref[3]:.4f}")
        if not act:
            assert tokens[r] == EOS and ts_state[r] == _state(h) and active[r] == 0 and logprob[r] == 123.0, name
            continue
        st, a = greedy_select_state(_state(h), tok, pos, limit, EOS, TB if rules else -1)
        assert tokens[r] == tok, name
        assert ts_state[r] == st, name
        assert active[r] == a, name
        assert abs(float(logprob[r]) - lp) <= 1e-4, name


@pytest.mark.parametrize("T", TEMPERATURES)
@pytest.mark.parametrize("V", [51865, 51866])
def test_sample_select_one_row_launches(V, T):
    """B = 1: each of the eight histories on its own, a row at pos + 1 == limit, and a q of 0."""
    bias, bias_begin, rows, refs, rules, top_k = _cases(V, T, "histories")
    for i in range(len(rows)):
        got = _launch(V, rows[i:i + 1], bias, bias_begin, rules, T, top_k)
        _compare(rows[i:i + 1], refs[i:i + 1], got, rules)
        if rows[i][0] == "pos + 1 == limit":
            assert got[3] == [0] and got[0][0] != EOS


@pytest.mark.parametrize("T", TEMPERATURES)
@pytest.mark.parametrize("V", [51865, 51866])
def test_sample_select_sixteen_rows_in_one_launch(V, T):
    """B = 16: the eight histories and the rows that show the kept set (a tie at kth, the lowest kept token, the first
    one outside), the mass rule, begin suppression, EOS and an inactive row, each with its own noise row."""
    bias, bias_begin, rows, refs, rules, top_k = _cases(V, T, "sixteen")
    got = _launch(V, rows, bias, bias_begin, rules, T, top_k)
    _compare(rows, refs, got, rules)
    assert got[3][[r[0] for r in rows].index("EOS drawn")] == 0


@pytest.mark.parametrize("T", TEMPERATURES)
@pytest.mark.parametrize("V", [51865, 51866])
def test_sample_select_rules_off(V, T):
    """timestamp_begin < 0: only the shared biases (bias_begin at a row's first position), every token one class."""
    bias, bias_begin, rows, refs, rules, top_k = _cases(V, T, "rules off")
    assert not rules
    _compare(rows, refs, _launch(V, rows, bias, bias_begin, rules, T, top_k), rules)


@pytest.mark.parametrize("T", TEMPERATURES)
@pytest.mark.parametrize("V", [51865, 51866])
def test_sample_select_top_k_one_and_the_whole_vocabulary(V, T):
    """top_k = 1: the greedy argmax whatever the noise; top_k >= V: every finite score is kept."""
    _, _, _, grefs, _, _ = _greedy_cases(V)
    bias, bias_begin, rows, refs, rules, top_k = _cases(V, T, "top_k 1")
    assert top_k == 1 and [ref[0] for ref in refs] == [g[0] for g in grefs[:len(HISTORIES)]]
    _compare(rows, refs, _launch(V, rows, bias, bias_begin, rules, T, top_k), rules)
    bias, bias_begin, rows, refs, rules, top_k = _cases(V, T, "top_k >= V")
    assert top_k >= V
    _compare(rows, refs, _launch(V, rows, bias, bias_begin, rules, T, top_k), rules)


def test_sample_select_refuses_bad_arguments():
    from cbw import _lib
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    p = t.data_ptr()
    ok = [p, 1, 8, 8, None, None, -1, -1, 0, -1, p, p, p, p, p, p, 1.0, 50, p, 8, _lib.stream_handle()]
    assert lib.cbw_sample_select(*ok) == 0
    torch.cuda.synchronize()
    for i, v in [(0, None), (10, None), (11, None), (12, None), (13, None), (14, None), (15, None), (18, None), (1, 0),
                 (1, 17), (2, 0), (3, 7), (19, 7), (16, 0.0), (16, -1.0), (16, float("nan")), (16, float("inf")),
                 (17, 0)]:
        args = list(ok)
        args[i] = v
        assert lib.cbw_sample_select(*args) == -1, (i, v)
    # a row's scores are held in 51 registers per thread of a 1024-thread block
    args = list(ok)
    args[2] = args[3] = args[19] = 1024 * 51 + 1
    assert lib.cbw_sample_select(*args) == -1
