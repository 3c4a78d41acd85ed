"""numpy statement of one cbw_history_rules call (include/cbw.h): the history upkeep, transformers 4.37.2's
RepetitionPenaltyLogitsProcessor in fp32 on the history's distinct tokens, then NoRepeatNGramLogitsProcessor with its
bans from cbw.decoder.banned_ngram_tokens.  Shared by tests/test_host_history_rules.py (which checks it against
transformers and the float64 oracle) and the GPU tests."""
import numpy as np


def penalise(x: np.ndarray, tokens, p: float) -> None:
    """x (fp32 [V]) in place: x[t] = x[t] * p where x[t] < 0 else x[t] / p, once per distinct t, in fp32."""
    ids = np.array(sorted(set(int(t) for t in tokens)), np.int64)
    if ids.size == 0:
        return
    g = x[ids]
    with np.errstate(invalid="ignore"):
        x[ids] = np.where(g < 0, g * np.float32(p), g / np.float32(p)).astype(np.float32)


def process_row(x: np.ndarray, seq, p: float, n: int) -> None:
    """The two processors on one row's logits x (fp32 [V], in place) for the row's sequence so far."""
    from cbw.decoder import banned_ngram_tokens
    if p != 1.0:
        penalise(x, seq, p)
    ban = banned_ngram_tokens(list(seq), n)
    if ban:
        x[np.array(ban, np.int64)] = -np.inf


def history_rules_ref(logits: np.ndarray, V: int, hist: np.ndarray, hist_len: np.ndarray, last_tokens, pos_rows,
                      active, p: float, n: int):
    """One call on logits fp32 [B, ld], hist int32 [B, hist_ld], hist_len int32 [B]; last_tokens int32 [B] or None,
    pos_rows / active int32 [B] -> (logits, hist, hist_len) after the call, copies."""
    x, h, hl = np.array(logits, np.float32), np.array(hist, np.int32), np.array(hist_len, np.int32)
    hist_ld = h.shape[1]
    for r in range(x.shape[0]):
        if not active[r]:
            continue
        length, pos = int(hl[r]), int(pos_rows[r])
        if length < 0 or length > hist_ld:
            continue
        if length == pos:   # the row moved one position: its last token is appended, where that can be done
            if last_tokens is None or length >= hist_ld:
                continue
            h[r, length] = last_tokens[r]
            length += 1
            hl[r] = length
        elif length != pos + 1:
            continue
        seq = np.clip(h[r, :length], 0, V - 1).tolist()
        process_row(x[r, :V], seq, float(p), int(n))
    return x, h, hl
