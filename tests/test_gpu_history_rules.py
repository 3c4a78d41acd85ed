"""cbw_history_rules alone against its numpy statement (tests/history_rules_ref.py, pinned against transformers on the
CPU): the rewritten logits bit for bit, everything else in the [B, ld] block untouched, the history the kernel keeps;
then chained in front of cbw_greedy_select against the float64 selection of test_gpu_greedy_select.py."""
import functools

import numpy as np
import pytest
import torch

from history_rules_ref import history_rules_ref

pytestmark = pytest.mark.gpu

CONTROLS = [(1.3, 0), (0.7, 0), (1.0, 1), (1.0, 2), (1.0, 3), (1.5, 3)]
WG = 256        # history_rules_kernel's workgroup: histories of WG - 1, WG and WG + 1 tokens straddle its strided loops
HIST_LD = 449   # max_len + 1 of the engines


@functools.lru_cache(maxsize=None)
def _sixteen_rows(V, ld, n):
    """-> (logits [16, ld], hist [16, HIST_LD], hist_len, pos, active, last_tokens, names).  ``n`` only sets two of the
    history lengths (n - 1 and n).  Tokens come from a small alphabet that holds 0 and V - 1, so tokens and n-grams
    repeat; pos is the position of the row's last token: hist_len - 1 for a whole history, hist_len for a row that
    moved and takes last_tokens."""
    rng = np.random.default_rng(7)
    alphabet = np.concatenate([[0, V - 1], rng.choice(np.arange(1, V - 1), 10, replace=False)])
    x = (rng.standard_normal((16, ld)) * 4).astype(np.float32)
    hist = np.full((16, HIST_LD), -12345, np.int32)   # beyond hist_len: never read
    m = max(n, 2)
    rows = []   # (name, history, append, active)

    def rand(length):
        return rng.choice(alphabet, length).tolist()
    rows.append(("empty history", [], False, 1))
    rows.append(("one token", rand(1), False, 1))
    rows.append((f"{m - 1} tokens", rand(m - 1), False, 1))
    rows.append((f"{m} tokens", rand(m), False, 1))
    rows.append(("workgroup - 1 tokens", rand(WG - 1), False, 1))
    rows.append(("workgroup tokens after the append", rand(WG - 1), True, 1))
    rows.append(("workgroup + 1 tokens", rand(WG + 1), False, 1))
    rows.append(("448 tokens after the append", rand(447), True, 1))
    rows.append(("one token forty times among others", [alphabet[3]] * 40 + rand(20) + [alphabet[3]] * 2, True, 1))
    rows.append(("all one token", [alphabet[4]] * 30, False, 1))
    a, b, c = (int(t) for t in alphabet[5:8])
    rows.append(("overlapping n-gram matches", [a, a, a, a, b, a, b, a, c, a, a, b, a], False, 1))
    rows.append(("special values at penalised ids", [int(t) for t in alphabet[2:8]] + [a, b], False, 1))
    rows.append(("inactive on entry", rand(50), True, 0))
    rows.append(("state fits neither relation", rand(50), None, 1))
    rows.append(("history entries outside [0, V)", [V + 5, -3, 2 ** 31 - 1, -2 ** 31, V, a, V + 5, -3], False, 1))
    rows.append(("448 tokens, whole", rand(448), False, 1))
    assert len(rows) == 16
    for t, v in zip(alphabet[2:8], (2.5, -2.5, 0.0, -0.0, -np.inf, 1e-38)):
        x[11, t] = v
    hist_len = np.zeros(16, np.int32)
    pos = np.zeros(16, np.int32)
    for r, (_, h, append, _) in enumerate(rows):
        hist[r, :len(h)] = h
        hist_len[r] = len(h)
        pos[r] = len(h) + 2 if append is None else len(h) if append else len(h) - 1
    active = np.array([r[3] for r in rows], np.int32)
    last = rng.choice(alphabet, 16).astype(np.int32)
    last[8] = alphabet[3]   # the repeated token once more: every n up to 3 then bans it
    return x, hist, hist_len, pos, active, last, [r[0] for r in rows]


def _launch(x, V, hist, hist_len, last, pos, active, p, n):
    from cbw import _lib
    lib = _lib.load()
    d = torch.device("cuda:0")
    xd, hd, hld, pd, ad = (torch.from_numpy(np.ascontiguousarray(t)).to(d) for t in (x, hist, hist_len, pos, active))
    ld_ = torch.from_numpy(last).to(d) if last is not None else None
    _lib.check(lib.cbw_history_rules(xd.data_ptr(), x.shape[0], V, x.shape[1], hd.data_ptr(), hist.shape[1],
                                     hld.data_ptr(), _lib.ptr(ld_), pd.data_ptr(), ad.data_ptr(), p, n,
                                     _lib.stream_handle()), "cbw_history_rules")
    torch.cuda.synchronize()
    assert np.array_equal(pd.cpu().numpy(), pos) and np.array_equal(ad.cpu().numpy(), active)
    return xd.cpu().numpy(), hd.cpu().numpy(), hld.cpu().numpy()


def _check(x, V, hist, hist_len, last, pos, active, p, n, names):
    want_x, want_h, want_len = history_rules_ref(x, V, hist, hist_len, last, pos, active, p, n)
    got_x, got_h, got_len = _launch(x, V, hist, hist_len, last, pos, active, p, n)
    assert np.array_equal(got_len, want_len)
    assert np.array_equal(got_h, want_h)
    for r, name in enumerate(names):   # the whole row of ld floats: what is rewritten, what is not, and [V, ld)
        diff = np.flatnonzero(got_x[r].view(np.uint32) != want_x[r].view(np.uint32))
        assert diff.size == 0, (name, p, n, diff[:8].tolist(), got_x[r, diff[:8]].tolist(), want_x[r, diff[:8]].tolist())
    return want_x, want_len


@pytest.mark.parametrize("null_last", [False, True], ids=["last_tokens", "no last_tokens"])
@pytest.mark.parametrize("p,n", CONTROLS)
def test_sixteen_rows_in_one_launch(p, n, null_last):
    V, ld = 51866, 51968
    x, hist, hist_len, pos, active, last, names = _sixteen_rows(V, ld, n)
    want_x, want_len = _check(x, V, hist, hist_len, None if null_last else last, pos, active, p, n, names)
    changed = [bool((want_x[r].view(np.uint32) != x[r].view(np.uint32)).any()) for r in range(16)]
    by = dict(zip(names, range(16)))
    # the reference itself: rows that must stay as they were do, and the controls act on the others
    for name in ("empty history", "inactive on entry", "state fits neither relation"):
        assert not changed[by[name]] and want_len[by[name]] == hist_len[by[name]]
    appended = [r for r in range(16) if pos[r] == hist_len[r] and active[r]]
    assert len(appended) == 3
    for r in appended:
        assert want_len[r] == hist_len[r] + (0 if null_last else 1) and changed[r] == (not null_last)
    assert want_len[by["448 tokens after the append"]] == (447 if null_last else 448)
    assert all(changed[by[k]] for k in ("all one token", "448 tokens, whole", "history entries outside [0, V)"))
    if n == 2:
        r = by["all one token"]
        assert np.isneginf(want_x[r, hist[r, 0]])
    if p != 1.0:   # forty occurrences, one penalty
        r = by["one token forty times among others"]
        t = hist[r, 0]
        if not null_last and not np.isneginf(want_x[r, t]):
            assert want_x[r, t] == (x[r, t] * np.float32(p) if x[r, t] < 0 else x[r, t] / np.float32(p))
        r = by["special values at penalised ids"]
        assert np.signbit(want_x[r, hist[r, 3]]) and want_x[r, hist[r, 3]] == 0 and not np.signbit(want_x[r, hist[r, 2]])


@pytest.mark.parametrize("p,n", CONTROLS)
def test_one_row_small_vocabulary(p, n):
    """B = 1, V = 200 in a pitch of 256: a history longer than the workgroup over few ids, so most are duplicates."""
    V, ld = 200, 256
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((1, ld)) * 4).astype(np.float32)
    hist = np.full((1, HIST_LD), -1, np.int32)
    hist[0, :300] = rng.integers(0, V, 300)
    _check(x, V, hist, np.array([300], np.int32), np.array([V - 1], np.int32), np.array([300], np.int32),
           np.array([1], np.int32), p, n, ["one row"])


def test_history_only_call_changes_no_logit():
    V, ld = 51866, 51968
    x, hist, hist_len, pos, active, last, names = _sixteen_rows(V, ld, 2)
    want_x, want_len = _check(x, V, hist, hist_len, last, pos, active, 1.0, 0, names)
    assert np.array_equal(want_x.view(np.uint32), x.view(np.uint32)) and (want_len != hist_len).sum() == 3


@functools.lru_cache(maxsize=None)
def _chain_rows(V):
    """Sixteen rows for cbw_history_rules -> cbw_greedy_select: test_gpu_greedy_select.py's eight timestamp-rule
    histories twice over logits of that file's scale.  Each row's token history repeats a trigram (u, tail,
    tok0) up to its last token, where tok0 is the token the float64 reference picks without the two processors: at
    p = 1.5, n = 3 it is penalised and banned, so the choice must move."""
    from test_gpu_greedy_select import EOS, HISTORIES, LD, TB, _reference
    rng = np.random.default_rng(6)   # chosen on the float64 reference alone: it decides all sixteen rows (see the test)
    x = rng.standard_normal((16, LD)).astype(np.float32) * 4
    # the timestamp logits shifted well down or up by turns, so that the mass rule is decided far outside fp32's reach
    x[:, TB:V] -= np.where(np.arange(16) % 2 == 0, 12.0, -6.0).astype(np.float32)[:, None]
    bias = np.zeros(V, np.float32)
    bias[[1, 2, 7]] = -np.inf
    bias_begin = bias.copy()
    bias_begin[[220, EOS, TB + 5, 300]] = -np.inf
    hs = [HISTORIES[r % len(HISTORIES)] for r in range(16)]
    hist = np.zeros((16, HIST_LD), np.int32)
    hist_len = np.zeros(16, np.int32)
    plain = []
    for r, h in enumerate(hs):
        tok0 = _reference(x[r, :V], bias_begin if not h else bias, h, True)[0]
        tail = h[-1] if h else 50359
        seq = [50258, 50259, 50359, 777, tail, tok0, 777, tail]
        hist[r, :len(seq)] = seq
        hist_len[r] = len(seq)
        plain.append(tok0)
    return x, bias, bias_begin, hs, hist, hist_len, plain


def test_chained_with_greedy_select():
    """The near-tie rule is test_gpu_greedy_select.py's (_assert_reference_margins): a row is decided when the float64
    reference's timestamp mass margin is infinite or at least 2.4 and its top-two gap at least 0.027.  With this seed
    the reference decides all sixteen rows, which is checked first, so every token must be equal."""
    from cbw import _lib
    from cbw.generate import greedy_select_state
    from test_gpu_greedy_select import EOS, LD, MAX_INITIAL, NO_TS, TB, _reference, _state
    V, p, n = 51866, 1.5, 3
    x, bias, bias_begin, hs, hist, hist_len, plain = _chain_rows(V)
    pos = (hist_len - 1).astype(np.int32)
    active = np.ones(16, np.int32)
    want_x, _, _ = history_rules_ref(x, V, hist, hist_len, None, pos, active, p, n)
    refs = [_reference(want_x[r, :V], bias_begin if not h else bias, h, True) for r, h in enumerate(hs)]
    excused = [r for r, (_, _, margin, gap) in enumerate(refs)
               if not (np.isinf(margin) or abs(margin) >= 2.4) or round(gap, 3) < 0.027]
    assert excused == [], [(r, refs[r][2:]) for r in excused]
    assert all(ref[0] != t0 for ref, t0 in zip(refs, plain))   # the controls matter in every row
    lib = _lib.load()
    d = torch.device("cuda:0")
    xd, hd, hld, pd, ad = (torch.from_numpy(t.copy()).to(d) for t in (x, hist, hist_len, pos, active))
    sel_pos = pd + 1   # the position the chosen token goes to
    ts_state = torch.tensor([_state(h) for h in hs], dtype=torch.int32, device=d)
    limit = torch.full((16,), 100, dtype=torch.int32, device=d)
    tokens = torch.full((16,), -7, dtype=torch.int32, device=d)
    logprob = torch.full((16,), 123.0, dtype=torch.float32, device=d)
    bd, bbd = torch.from_numpy(bias).to(d), torch.from_numpy(bias_begin).to(d)
    st = _lib.stream_handle()
    _lib.check(lib.cbw_history_rules(xd.data_ptr(), 16, V, LD, hd.data_ptr(), HIST_LD, hld.data_ptr(), None,
                                     pd.data_ptr(), ad.data_ptr(), p, n, st), "cbw_history_rules")
    _lib.check(lib.cbw_greedy_select(xd.data_ptr(), 16, V, LD, bd.data_ptr(), bbd.data_ptr(), TB, NO_TS, EOS, MAX_INITIAL,
                                     ts_state.data_ptr(), sel_pos.data_ptr(), limit.data_ptr(), ad.data_ptr(),
                                     tokens.data_ptr(), logprob.data_ptr(), st), "cbw_greedy_select")
    torch.cuda.synchronize()
    got, lps, states = tokens.cpu().tolist(), logprob.cpu().numpy(), ts_state.cpu().tolist()
    for r, (tok, lp, _, _) in enumerate(refs):
        print(f"row {r}: token {got[r]} (ref {tok}, without the processors {plain[r]}) logprob {lps[r]:.6f} (ref {lp:.6f})")
    wrong = [r for r in range(16) if got[r] != refs[r][0] and r not in excused]
    assert wrong == [] and len(excused) <= 1
    for r, (tok, lp, _, _) in enumerate(refs):
        assert states[r] == greedy_select_state(_state(hs[r]), tok, int(pos[r]) + 1, 100, EOS, TB)[0]
        assert abs(float(lps[r]) - lp) <= 1e-4


def test_refuses_bad_arguments_with_device_pointers():
    from cbw import _lib
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    q = t.data_ptr()
    ok = [q, 1, 8, 8, q, 4, q, None, q, q, 1.5, 2, _lib.stream_handle()]
    for i, v in [(0, None), (4, None), (6, None), (8, None), (9, None), (1, 0), (1, 17), (3, 7), (5, 0), (10, 0.0),
                 (10, float("nan")), (11, -1)]:
        args = list(ok)
        args[i] = v
        assert lib.cbw_history_rules(*args) == -1, (i, v)
    assert not t.cpu().any()
