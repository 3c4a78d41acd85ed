"""Float64 reference, error bound and seeded inputs for the decoder's attention kernels (cbw_decode_attention,
cbw_decode_cross_probs; include/cbw.h), shared by tests/test_host_dec_attention.py and tests/test_gpu_dec_attention.py.

Reference: out[r, h] = softmax_j(q_rh . k_jh) v_jh over the row's live keys, in float64 from the same bf16 operands
(bf16 -> float64 is exact), with a key count per row, the row-to-batch map r // rows_per_kv and the causal rule (row r
sees keys 0..r, stated as a count of r + 1).

Bound (derived, never tuned against a kernel), per output element:

    tol = 2^-8 |ref| + (2 eps_s + 2e-4) max_j |v[j, d]|,   eps_s = 64 * 2^-24 * max_j sum_i |q_i k_ji|

over the row's live keys: one bf16 ulp of the output; the worst-case fp32 rounding eps_s of a 64-term fma dot product,
which changes a weight by e^(+-eps_s) and so the output by at most about 2 eps_s max|v|; and 2e-4 for up to 1536 fp32
accumulations (1536 * 2^-24 ~ 9e-5), __expf and the division.  Probabilities (fp32 out): |got - ref| <= 1e-4 ref +
1e-12, each row summing to 1 within 1e-5.

Inputs: unit-normal k, q scaled by 0.1 (near-uniform attention over hundreds of keys), 0.35 (a few keys) or 3 (one-hot,
scores up to about +-100), v columns scaled by 0.1, 1, 10 in turn.  Planted so that a count error moves an output by
O(max|v|) in every regime: the last live key of a row (index count - 1) is aimed at the row's query so that it takes
about three quarters of the weight, with a v of +-4 x the column scale; every cache row past the count is poison, a key
aimed to score 60 above the row's maximum with v = 1e4 (finite), out to the full kv_bstride; the k and v slots of fused
q rows (ldq = 3 D) hold the same poison.  Rows that share a K/V batch get one signature key each (keys 0..R-1), heavy
for that row alone, so that a row computed from another row's query is told apart.  In a causal case key j is the last
live key of row j and the first dead key of row j - 1, and is aimed at both.  Every planted v row has a sign pattern
of its own, so that no two of them can stand in for each other.

Two hard cases for the combine: "underflow", where one 64-key chunk scores 250 below the row's maximum, so that its
factor exp(m_c - M) underflows, with a v of +-20 x the column scale that a mis-combined chunk would bring in; and
"equal", where every live key is the same vector, so that all scores are equal, the weights are 1 / count, and the last
live key's v is 4 x count x the column scale to keep a count error at O(max|v|)."""
import functools
from dataclasses import dataclass, field

import numpy as np
import torch

CS = np.array([0.1, 1.0, 10.0])          # v column scales
REGIMES = (0.1, 0.35, 3.0)               # q scales: near-uniform, a few keys, one-hot
POISON_V = 1e4
CHUNK = 64                               # the split kernel's key chunk


def to_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def f64(t):
    return t.to(torch.float64).numpy()


@dataclass
class Case:
    name: str
    q: torch.Tensor            # bf16 [B, ldq]
    k: torch.Tensor            # bf16 [NB, kv_rows, D]
    v: torch.Tensor            # bf16 [NB, kv_rows, D]
    counts: np.ndarray         # int64 [B]: live keys of each row
    rows_per_kv: int
    n_keys: int                # the host key count of the launch (>= every count)
    H: int
    D: int
    causal: bool = False
    hard_chunk: int = -1       # the chunk whose scores lie >= 200 below the row maximum (underflow case)
    extra: dict = field(default_factory=dict)

    @property
    def B(self):
        return self.q.shape[0]

    @property
    def ldq(self):
        return self.q.shape[1]

    @property
    def kv_rows(self):
        return self.k.shape[1]

    @property
    def kv_bstride(self):
        return self.k.shape[1] * self.D

    @property
    def batch(self):
        return np.arange(self.B) // self.rows_per_kv


def _softmax_out(s, V):
    p = np.exp(s - s.max())
    return (p / p.sum()) @ V


def _chunked_out(s, V, chunk, mode):
    """the split kernel's arithmetic in float64: per 64-key chunk (m, l, o), combined with exp(m_c - M); chunk `chunk`
    replaced by a neutral partial (mode "drop") or combined with factor 1 (mode "one": a combine that mishandles it)"""
    parts = []
    for c in range(0, len(s), CHUNK):
        m = s[c:c + CHUNK].max()
        e = np.exp(s[c:c + CHUNK] - m)
        parts.append((m, e.sum(), e @ V[c:c + CHUNK]))
    if mode == "drop":
        parts[chunk] = (-np.inf, 0.0, np.zeros(V.shape[1]))
    M = max(m for m, _, _ in parts)
    o, L = np.zeros(V.shape[1]), 0.0
    for c, (m, l, oc) in enumerate(parts):
        if l > 0.0:
            f = 1.0 if (mode == "one" and c == chunk) else np.exp(m - M)
            o, L = o + f * oc, L + f * l
    return o / L


def reference(case, counts=None, batch=None, qrow=None, swap_last=False, chunk_edit=None, rows=None, with_tol=True):
    """-> (ref float64 [B, 64 H], tol float64 [B, 64 H]).  The keyword arguments restate the operation wrongly (the
    mutants of the host test): other counts, another row-to-batch map, row r computed from query qrow[r], v of the last
    two live keys swapped, a chunk dropped or mis-combined.  rows: only these rows (the others stay 0)."""
    counts = case.counts if counts is None else counts
    batch = case.batch if batch is None else batch
    qf = f64(case.q[:, :64 * case.H])
    ref = np.zeros((case.B, 64 * case.H))
    tol = np.zeros_like(ref)
    last_b, K, V = -1, None, None
    for r in (range(case.B) if rows is None else rows):
        b, n = int(batch[r]), int(counts[r])
        if b != last_b:
            K, V, last_b = f64(case.k[b, :, :64 * case.H]), f64(case.v[b, :, :64 * case.H]), b
        Kn, Vn = K[:n], V[:n]
        if swap_last:
            Vn = Vn.copy()
            Vn[[n - 2, n - 1]] = Vn[[n - 1, n - 2]]
        for h in range(case.H):
            sl = slice(64 * h, 64 * h + 64)
            qv = qf[r if qrow is None else qrow[r], sl]
            s = Kn[:, sl] @ qv
            if chunk_edit is None:
                ref[r, sl] = _softmax_out(s, Vn[:, sl])
            else:
                ref[r, sl] = _chunked_out(s, Vn[:, sl], *chunk_edit)
            if with_tol:
                eps_s = 64 * 2.0 ** -24 * (np.abs(Kn[:, sl]) @ np.abs(qv)).max()
                tol[r, sl] = 2.0 ** -8 * np.abs(ref[r, sl]) + (2 * eps_s + 2e-4) * np.abs(Vn[:, sl]).max(axis=0)
    return ref, tol


def probabilities(case, head):
    """-> float64 [B, n_keys]: softmax_j(q_r . k_j) of one head over K/V batch 0's first n_keys keys"""
    sl = slice(64 * head, 64 * head + 64)
    s = f64(case.q[:, sl]) @ f64(case.k[0, :case.n_keys, sl]).T
    p = np.exp(s - s.max(axis=1, keepdims=True))
    return p / p.sum(axis=1, keepdims=True)


def emulate_fp32(case):
    """the kernels' arithmetic on the CPU: fp32 scores, max subtraction, exp, fp32 P.V, division, bf16 output
    -> float64 [B, 64 H] of the bf16 values"""
    out = torch.zeros(case.B, 64 * case.H, dtype=torch.bfloat16)
    for r in range(case.B):
        b, n = int(case.batch[r]), int(case.counts[r])
        for h in range(case.H):
            sl = slice(64 * h, 64 * h + 64)
            s = case.k[b, :n, sl].float() @ case.q[r, sl].float()
            p = torch.exp(s - s.max())
            out[r, sl] = ((p @ case.v[b, :n, sl].float()) / p.sum()).to(torch.bfloat16)
    return f64(out)


def worst_ratio(got, ref, tol, rows=None):
    """max |got - ref| / tol (over the given rows); inf where got is not finite"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref) / tol
    err = np.where(np.isfinite(err), err, np.inf)
    return float((err if rows is None else err[rows]).max())


# ---------------------------------------------------------------------------------------------------- input builders
def _aim(Q, t):
    """the least-norm u with Q u = t: a key that scores t[i] against query row i"""
    return Q.T @ np.linalg.solve(Q @ Q.T, np.asarray(t, dtype=np.float64))


def _lse(s):
    m = s.max()
    return m + np.log(np.exp(s - m).sum())


def build(name, seed, H, D, rows_per_kv, NB, counts, n_keys, kv_rows, fused, causal=False, kind="planted"):
    """counts: one per row (rows of a K/V batch share it unless causal).  fused: ldq = 3 D.  kind: "planted",
    "underflow" (chunk 2 of every batch scores 250 below the row maximum) or "equal" (every live key the same)."""
    g = np.random.default_rng(seed)
    B = NB * rows_per_kv
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.shape == (B,) and counts.min() >= 1 and counts.max() <= n_keys <= kv_rows and D >= 64 * H
    batch = np.arange(B) // rows_per_kv
    unit = batch if (rows_per_kv > 1 and not causal) else np.arange(B)   # the regime: per batch where rows share keys
    scale = np.array(REGIMES)[unit % 3] if kind == "planted" else np.full(B, 0.35)
    q = f64(to_bf16(g.standard_normal((B, 64 * H)) * scale[:, None]))
    k = to_bf16(g.standard_normal((NB, kv_rows, D), dtype=np.float32))
    v = to_bf16(g.standard_normal((NB, kv_rows, D), dtype=np.float32) * CS[np.arange(D) % 3].astype(np.float32))
    col = CS[np.arange(D) % 3]
    sig_sign = np.where(g.random((rows_per_kv, D)) < 0.5, -1.0, 1.0)
    hard = -1
    for b in range(NB):
        rows = np.flatnonzero(batch == b)
        maxc = int(counts[rows].max())
        K = f64(k[b])                                        # edited below, written back as bf16 at the end

        def put(j, h, u):
            K[j, 64 * h:64 * h + 64] = f64(to_bf16(u))

        def scores(r, h, n):
            return K[:n, 64 * h:64 * h + 64] @ q[r, 64 * h:64 * h + 64]

        Vb = f64(v[b])
        bsign = np.where(g.random(D) < 0.5, -1.0, 1.0)         # the batch's own pattern (the all-equal case)
        if kind == "equal":
            K[:maxc] = K[0]
        if kind == "underflow":
            hard = 2
            lo, hi = hard * CHUNK, hard * CHUNK + CHUNK
            assert hi < maxc - 1 and not causal
            for h in range(H):
                Q = q[rows, 64 * h:64 * h + 64]
                live = np.r_[0:lo, hi:maxc]
                smax = (K[live, 64 * h:64 * h + 64] @ Q.T).max(axis=0)
                u = _aim(Q, smax - 250.0)
                for j in range(lo, hi):
                    put(j, h, u + 0.05 * g.standard_normal(64))
            Vb[lo:hi] = 20.0 * col * np.where(g.random((CHUNK, D)) < 0.5, -1.0, 1.0)
        if not causal and rows_per_kv > 1 and maxc >= rows_per_kv + 2 and kind != "equal":
            for i, r in enumerate(rows):                     # signature keys: key i heavy for row i of the batch alone
                for h in range(H):
                    put(i, h, _aim(q[r:r + 1, 64 * h:64 * h + 64], [_lse(scores(r, h, maxc - 1)) + np.log(3.0)]))
                Vb[i] = 4.0 * col * sig_sign[i]
        if kind != "equal":
            for n in np.unique(counts[rows]):                # ascending: key n - 1, the last live key of these rows
                n = int(n)
                j = n - 1
                S, P = rows[counts[rows] == n], rows[counts[rows] == n - 1]
                for h in range(H):
                    aimed = np.r_[S, P]
                    t = [(_lse(scores(r, h, j)) if j else 0.0) + np.log(3.0) for r in aimed]
                    put(j, h, _aim(q[aimed, 64 * h:64 * h + 64], t))
                Vb[j] = 4.0 * col * np.where(g.random(D) < 0.5, -1.0, 1.0)    # its own pattern: distinct
        else:
            Vb[maxc - 1] = 4.0 * maxc * col * bsign   # weight 1 / maxc: an O(max|v|) share
        if maxc < kv_rows:                                   # poison: every cache row past the count
            top = rows[counts[rows] == maxc]
            for h in range(H):
                t = [scores(r, h, maxc).max() + 60.0 for r in top]
                u = f64(to_bf16(_aim(q[top, 64 * h:64 * h + 64], t)))
                K[maxc:, 64 * h:64 * h + 64] = u
            Vb[maxc:] = POISON_V
        k[b] = to_bf16(K)
        v[b] = to_bf16(Vb)
    if fused:
        qq = np.full((B, 3 * D), POISON_V)
        qq[:, :64 * H] = q
        qq[:, 64 * H:D] = 0.0
        for r in range(B):
            n = int(counts[r])
            for h in range(H):
                sl = slice(64 * h, 64 * h + 64)
                s = f64(k[batch[r], :n, sl]) @ q[r, sl]
                qq[r, D + 64 * h:D + 64 * h + 64] = _aim(q[r:r + 1, sl], [s.max() + 60.0])
            qq[r, D + 64 * H:2 * D] = 0.0
        qt = to_bf16(qq)
    else:
        qt = to_bf16(np.concatenate([q, np.zeros((B, D - 64 * H))], axis=1))
    return Case(name, qt, k, v, counts, rows_per_kv, n_keys, H, D, causal, hard)


def _pad(n):
    """cache rows for a launch over n keys: whole 64-key chunks and one more, so that poison follows every count"""
    return (n + CHUNK - 1) // CHUNK * CHUNK + CHUNK


SELF_HOST_KEYS = (1, 63, 64, 65, 127, 128, 129, 383, 384, 385, 447, 448)
CROSS_KEYS = (65, 128, 1472, 1473, 1499, 1500, 1535, 1536)
ROW_KEYS = (1, 31, 32, 33, 96, 97, 98, 129, 257, 1500, 1536)
ROW_RPK = (1, 5, 10)
PROB_T = (1, 7)
PROB_KEYS = (1, 255, 256, 257, 1500)


@functools.lru_cache(maxsize=None)
def self_every_count():
    """448 rows, row r with r + 1 keys (device counts), own K/V batch each, fused q rows, H 2, D 128"""
    return build("self_every_count", 1, 2, 128, 1, 448, np.arange(448) + 1, 448, 448, True)


@functools.lru_cache(maxsize=None)
def self_host(n):
    return build(f"self_host_{n}", 100 + n, 3, 192, 1, 5, [n] * 5, n, _pad(n), True)


@functools.lru_cache(maxsize=None)
def self_shared():
    """5 rows, one device count of 200 under a host bound of 448"""
    return build("self_shared", 2, 3, 192, 1, 5, [200] * 5, 448, 448, True)


@functools.lru_cache(maxsize=None)
def self_80():
    """80 rows with device counts spread over 1..448"""
    return build("self_80", 3, 3, 192, 1, 80, 1 + (np.arange(80) * 37) % 448, 448, 448, True)


@functools.lru_cache(maxsize=None)
def cross(R, n):
    """R rows per K/V batch, 3 batches of different data (one per regime), ldq = D"""
    return build(f"cross_R{R}_n{n}", 1000 * R + n, 3, 192, R, 3, [n] * (3 * R), n, _pad(n), False)


@functools.lru_cache(maxsize=None)
def cross_80():
    """the 80-row lock-step shape: 16 K/V batches of 5 rows at 1500 keys"""
    return build("cross_80", 4, 3, 192, 5, 16, [1500] * 80, 1500, 1536, False)


@functools.lru_cache(maxsize=None)
def cross_underflow():
    return build("cross_underflow", 5, 3, 192, 5, 2, [300] * 10, 300, _pad(300), False, kind="underflow")


@functools.lru_cache(maxsize=None)
def cross_equal():
    return build("cross_equal", 6, 3, 192, 5, 2, [130] * 10, 130, _pad(130), False, kind="equal")


@functools.lru_cache(maxsize=None)
def row_causal():
    """the prefill's self-attention: 300 rows of one K/V batch, row r sees keys 0..r; fused q rows"""
    return build("row_causal", 7, 3, 192, 300, 1, np.arange(300) + 1, 300, 304, True, causal=True)


@functools.lru_cache(maxsize=None)
def row_plain(n, rpk):
    return build(f"row_n{n}_rpk{rpk}", 10000 * rpk + n, 3, 192, rpk, 2, [n] * (2 * rpk), n, _pad(n), False)


@functools.lru_cache(maxsize=None)
def probs_case(T, n):
    """T query rows against one batch of n cross keys (the timestamp pass): ldq = D"""
    return build(f"probs_T{T}_n{n}", 20000 * T + n, 3, 192, T, 1, [n] * T, n, _pad(n), False)


def all_cases():
    """name -> builder of every input of the GPU tests, for the host test's mutant and emulation checks"""
    makers = {"self_every_count": self_every_count, "self_shared": self_shared, "self_80": self_80,
              "cross_80": cross_80, "cross_underflow": cross_underflow, "cross_equal": cross_equal,
              "row_causal": row_causal}
    for n in SELF_HOST_KEYS:
        makers[f"self_host_{n}"] = functools.partial(self_host, n)
    for n in CROSS_KEYS:
        for R in range(1, 9):
            makers[f"cross_R{R}_n{n}"] = functools.partial(cross, R, n)
    for n in ROW_KEYS:
        for rpk in ROW_RPK:
            makers[f"row_n{n}_rpk{rpk}"] = functools.partial(row_plain, n, rpk)
    for T in PROB_T:
        for n in PROB_KEYS:
            makers[f"probs_T{T}_n{n}"] = functools.partial(probs_case, T, n)
    return makers
