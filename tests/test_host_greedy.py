"""CPU-only tests of the device greedy search's host side: cbw.generate.greedy_replay (the host's reading of the
device log DecoderEngine.greedy_windows copies back), the position / limit invariant of cbw_greedy_select's
bookkeeping (cbw.generate.greedy_select_state), and the C ABI entry (header symbol, ctypes signature)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

EOS = 50257


def _log(rows):
    """rows: per row the list of logged tokens -> (tokens [steps][rows], logprobs [steps][rows]); log-prob of step s,
    row r = -(s + 1) - r / 10."""
    steps = len(rows[0])
    toks = np.array(rows, np.int32).T.copy()
    lps = np.array([[-(s + 1) - r / 10 for r in range(len(rows))] for s in range(steps)], np.float32)
    return toks, lps


def test_replay_ends_a_row_at_eos_and_ignores_what_is_logged_after():
    from cbw.generate import greedy_replay
    toks, lps = _log([[11, 12, EOS, EOS, 77, EOS]])
    (seq, lp, fin), = greedy_replay(toks, lps, [[1, 2, 3]], [100], EOS)
    assert seq == [1, 2, 3, 11, 12, EOS] and fin
    assert lp == [float(lps[s, 0]) for s in range(3)]


def test_replay_ends_a_row_at_its_limit():
    from cbw.generate import greedy_replay
    toks, lps = _log([[11, 12, 13, 14, 15]])
    (seq, lp, fin), = greedy_replay(toks, lps, [[1, 2]], [5], EOS)
    assert seq == [1, 2, 11, 12, 13] and fin and len(lp) == 3
    # a limit the prefix already fills: nothing is taken
    (seq, lp, fin), = greedy_replay(toks, lps, [[1, 2]], [2], EOS)
    assert seq == [1, 2] and fin and lp == []


def test_replay_unfinished_row_continues_in_the_next_replay():
    from cbw.generate import greedy_replay
    toks, lps = _log([[11, 12, 13]])
    (seq, lp, fin), = greedy_replay(toks, lps, [[1, 2]], [9], EOS)
    assert seq == [1, 2, 11, 12, 13] and not fin and len(lp) == 3
    toks2, lps2 = _log([[14, EOS, EOS]])
    (seq2, lp2, fin2), = greedy_replay(toks2, lps2, [seq], [9], EOS)
    assert seq2 == [1, 2, 11, 12, 13, 14, EOS] and fin2 and len(lp2) == 2


def test_replay_two_windows_with_different_prefix_lengths_and_an_empty_row():
    from cbw.generate import greedy_replay
    toks, lps = _log([[11, EOS, EOS, EOS], [0, 0, 0, 0], [21, 22, 23, 24]])
    out = greedy_replay(toks, lps, [[1, 2, 3, 4, 5], None, [7, 8]], [50, 0, 5], EOS)
    assert out[1] is None
    assert out[0][0] == [1, 2, 3, 4, 5, 11, EOS] and out[0][2]
    assert out[2][0] == [7, 8, 21, 22, 23] and out[2][2]
    # log-probs only of the steps before each row's end, from that row's column
    assert out[0][1] == [float(lps[0, 0]), float(lps[1, 0])]
    assert out[2][1] == [float(lps[s, 2]) for s in range(3)]


def test_replay_matches_greedy_over_a_scripted_step_fn():
    """greedy_replay ends a row exactly where cbw.generate.greedy ends it (EOS, or max_length tokens)."""
    from cbw.generate import greedy, greedy_replay
    script = [31, 32, 33, 34, EOS, 36, 37]
    for limit in range(3, 12):
        calls = []

        def step_fn(tokens, pos, reorder_rows):
            calls.append(pos)
            n = max(len(calls) - 3, 0)   # the third call consumes the last prefix token: the first scripted choice
            return np.zeros((1, 1), np.float32), np.array([[script[min(n, len(script) - 1)]]], np.int32)
        want = greedy(step_fn, [1, 2, 3], EOS, limit)
        toks, lps = _log([script])
        (seq, _, fin), = greedy_replay(toks, lps, [[1, 2, 3]], [limit], EOS)
        assert seq == want and fin, limit


@pytest.mark.parametrize("n_prefix", [2, 3, 7, 445, 447])
@pytest.mark.parametrize("room", [1, 2, 3])
def test_limit_invariant_keeps_every_step_inside_the_cache(n_prefix, room):
    """cbw_greedy_select's bookkeeping (greedy_select_state) for a row that never takes EOS, the worst case: an active
    row steps at pos <= limit - 2, a row that ended stays at pos <= limit - 1, over more enqueued steps than the row
    has room for -- so every K/V write of cbw_decoder_step_rows is below max_len for limit <= max_len."""
    from cbw.generate import greedy_replay, greedy_select_state
    limit = n_prefix + room
    pos, active, st = n_prefix, 1, [0, -1, -1, -1]
    writes, toks = [], []
    for s in range(room + 4):
        if active:
            st, active = greedy_select_state(st, 100 + s, pos, limit, EOS, 50364)
            toks.append(100 + s)
            if active:
                assert pos <= limit - 2
        else:
            toks.append(EOS)
        writes.append(pos)          # the decode step of every row, active or not, writes its K/V at pos
        assert pos <= limit - 1
        pos += active
    assert max(writes) == limit - 1 and st[0] == room
    # the replay takes exactly the tokens of the active selects
    (seq, lp, fin), = greedy_replay(np.array(toks, np.int32)[:, None], np.zeros((len(toks), 1), np.float32),
                                    [list(range(n_prefix))], [limit], EOS)
    assert fin and len(seq) == limit and seq[n_prefix:] == [100 + s for s in range(room)]


def test_select_state_tracks_timestamps_and_eos():
    from cbw.generate import greedy_select_state
    TB = 50364
    st, a = greedy_select_state([0, -1, -1, -1], TB + 3, 5, 20, EOS, TB)
    assert (st, a) == ([1, TB + 3, -1, TB + 3], 1)
    st, a = greedy_select_state(st, 17, 6, 20, EOS, TB)
    assert (st, a) == ([2, 17, TB + 3, TB + 3], 1)
    st, a = greedy_select_state(st, EOS, 7, 20, EOS, TB)
    assert (st, a) == ([3, EOS, 17, TB + 3], 0)
    st, a = greedy_select_state([4, 9, 8, -1], TB + 1, 7, 20, EOS, -1)   # rules off: no timestamp is tracked
    assert (st, a) == ([5, TB + 1, 9, -1], 1)


def test_header_symbol_and_ctypes_signature():
    from cbw import _lib
    src = open(os.path.join(REPO, "include", "cbw.h")).read()
    m = re.search(r"^int\s+cbw_greedy_select\s*\((.*?)\)\s*;", src, flags=re.M | re.S)
    assert m, "include/cbw.h does not declare cbw_greedy_select"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const float* logits", "int B", "int V", "int ld", "const float* bias", "const float* bias_begin",
                      "int timestamp_begin", "int no_timestamps", "int eos", "int max_initial", "int32_t* ts_state",
                      "const int32_t* pos_rows", "const int32_t* limit", "int32_t* active", "int32_t* tokens",
                      "float* logprob", "cbw_stream_t stream"]
    res, args = _lib.SIGNATURES["cbw_greedy_select"]
    want = [ctypes.c_int if p.startswith("int ") else ctypes.c_void_p for p in params]
    assert res is ctypes.c_int and list(args) == want
    lib = _lib.load()
    assert hasattr(lib, "cbw_greedy_select")
    # the entry checks its arguments before any launch (no GPU needed to be refused)
    assert lib.cbw_greedy_select(None, 1, 8, 8, None, None, -1, -1, 0, -1, None, None, None, None, None, None, None) == -1
