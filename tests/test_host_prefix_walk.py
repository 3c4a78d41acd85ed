"""CPU-only test of the forced-prefix walk cbw.generate.beam_search, greedy and beam_sample share (_consume_prefix):
one pass through the step function's ``prefill`` when it has one and the prefix has more than one token, token by
token otherwise -- also when ``prefill`` returns None.  The step function is a deterministic fake over a 12-token
vocabulary whose scores depend only on (position, last token), so every way through the prefix gives one result."""
import numpy as np
import pytest
import torch

V, EOS, BEAMS = 12, 11, 3
PREFIXES = ([3], [3, 5, 2, 7])


def _logprobs(pos, tok):
    x = np.random.default_rng(1000 * pos + tok).normal(size=V) * 2.0
    return x - np.log(np.exp(x).sum())


class _Fake:
    """fn(tokens, pos, reorder_rows) -> the next position's scores of every row, from (pos, the row's token) alone:
    the sorted top-k (log-probs, ids) of a StepFn, or with ``as_tensor`` the [rows, V] log-probs of a scores_fn.
    ``calls`` records every (tokens, pos, reorder_rows); ``prefill`` ("value" / "none" / None: no such attribute)
    records its prefixes in ``prefills``."""

    def __init__(self, as_tensor, prefill):
        self.as_tensor, self.calls, self.prefills = as_tensor, [], []
        if prefill is not None:
            self.prefill = lambda prefix: self._prefill(prefix, prefill)

    def _out(self, pos, tokens):
        lp = np.stack([_logprobs(pos, int(t)) for t in tokens])
        if self.as_tensor:
            return torch.from_numpy(lp).float()
        idx = np.argsort(-lp, axis=-1, kind="stable")
        return np.take_along_axis(lp, idx, -1), idx.astype(np.int32)

    def __call__(self, tokens, pos, reorder_rows):
        self.calls.append((list(tokens), pos, None if reorder_rows is None else list(reorder_rows)))
        return self._out(pos, tokens)

    def _prefill(self, prefix, mode):
        self.prefills.append(list(prefix))
        return self._out(len(prefix) - 1, [prefix[-1]] * self.rows) if mode == "value" else None


def _run(kind, prefix, prefill):
    from cbw.generate import beam_sample, beam_search, greedy
    fn = _Fake(kind == "beam_sample", prefill)
    fn.rows = 1 if kind == "greedy" else BEAMS
    max_length = len(prefix) + 6
    if kind == "beam_search":
        out = beam_search(fn, prefix, BEAMS, EOS, max_length, return_score=True)
    elif kind == "greedy":
        out = greedy(fn, prefix, EOS, max_length)
    else:
        out = beam_sample(fn, prefix, BEAMS, EOS, max_length, 0.8, generator=torch.Generator().manual_seed(7),
                          return_score=True)
    return out, fn


@pytest.mark.parametrize("prefix", PREFIXES, ids=("prefix1", "prefix4"))
@pytest.mark.parametrize("kind", ("beam_search", "greedy", "beam_sample"))
def test_prefix_walk_is_the_same_through_prefill_and_token_by_token(kind, prefix):
    rows = 1 if kind == "greedy" else BEAMS
    want, walked = _run(kind, prefix, None)
    seq = want if kind == "greedy" else want[0]
    assert seq[:len(prefix)] == prefix and len(prefix) < len(seq) <= len(prefix) + 6
    walk = [([t] * rows, p, None) for p, t in enumerate(prefix)]
    assert walked.calls[:len(prefix)] == walk
    assert all(p == len(prefix) + i for i, (_, p, _) in enumerate(walked.calls[len(prefix):]))

    got, filled = _run(kind, prefix, "value")
    assert got == want
    if len(prefix) > 1:   # one pass: the prefix's positions never reach the step function
        assert filled.prefills == [prefix] and filled.calls == walked.calls[len(prefix):]
    else:                 # a one-token prefix is stepped, prefill is not called
        assert filled.prefills == [] and filled.calls == walked.calls

    got, fell_back = _run(kind, prefix, "none")   # prefill cannot run the pass: token by token after all
    assert got == want
    assert fell_back.prefills == ([prefix] if len(prefix) > 1 else [])
    assert fell_back.calls == walked.calls and fell_back.calls[:len(prefix)] == walk
