"""The decoder's attention kernels one by one (cbw_decode_attention, cbw_decode_cross_probs; include/cbw.h) against
the float64 reference of tests/dec_attention_ref.py under its derived bound: the row kernel
(path 2), split plus combine (path 3), the one-launch self-attention (path 4), the decode step's own routing (paths 0
and 1) and the cross-attention probabilities.  The inputs are planted so that an off-by-one key count, a wrong K/V
batch, a wrong query row or a mis-combined chunk leaves the bound by more than 10x, which
tests/test_host_dec_attention.py proves on the CPU together with the bound's fairness to fp32 arithmetic.

`out` is prefilled with NaN and every element must come back finite and inside the bound; each test prints its worst
error / tol (docs/MEASUREMENT_LOG.md keeps the MI355X figures).  Every launch is in range and every planted row lies
inside its allocation."""
import numpy as np
import pytest
import torch

import dec_attention_ref as R

pytestmark = pytest.mark.gpu

_REF = {}


def ref_of(case):
    if case.name not in _REF:
        _REF[case.name] = R.reference(case)
    return _REF[case.name]


def dev():
    return torch.device("cuda:0")


def run(case, path, device_counts=False, nk_rows=0, causal=0, rows=None, R_sub=None, raw=False):
    """One cbw_decode_attention call on the case -> the bf16 output as float64 [B, 64 H] (raw: the int16 bits).
    device_counts: n_keys_pos = count - 1 per K/V batch (nk_rows 1) or one shared entry (nk_rows 0).
    rows = (r0, n): only rows r0 .. r0 + n - 1, with their own K/V batches (rows_per_kv 1)."""
    from cbw import _lib
    lib = _lib.load()
    d = dev()
    q, k, v = case.q.to(d), case.k.to(d), case.v.to(d)
    B, H, D, rpk = case.B, case.H, case.D, case.rows_per_kv
    pos = None
    if device_counts:
        per_batch = case.counts[::rpk] - 1
        pos = torch.from_numpy((per_batch if nk_rows else per_batch[:1]).astype(np.int32)).to(d)
    r0 = 0
    if rows is not None:
        assert rpk == 1
        r0, B = rows
        assert 0 <= r0 and r0 + B <= case.B
    out = torch.full((B, D), float("nan"), dtype=torch.bfloat16, device=d)
    ws_floats = lib.cbw_decode_attention_ws_floats(B, H)
    ws = torch.empty(ws_floats, dtype=torch.float32, device=d)
    esz = 2
    rc = lib.cbw_decode_attention(q.data_ptr() + r0 * case.ldq * esz, case.ldq, k.data_ptr() + r0 * case.kv_bstride * esz,
                                  v.data_ptr() + r0 * case.kv_bstride * esz, case.kv_bstride, case.n_keys, rpk,
                                  (pos.data_ptr() + (4 * r0 if nk_rows else 0)) if pos is not None else None, nk_rows,
                                  causal, path, out.data_ptr(), B, H, D, ws.data_ptr(), ws_floats, _lib.stream_handle())
    _lib.check(rc, "cbw_decode_attention")
    torch.cuda.synchronize()
    if raw:
        return out[:, :64 * H].contiguous().view(torch.int16).cpu().numpy()
    return out[:, :64 * H].double().cpu().numpy()


def check(case, got, what, rows=None):
    ref, tol = ref_of(case)
    if rows is not None:
        ref, tol = ref[rows], tol[rows]
    assert np.isfinite(got).all(), f"{case.name} {what}: {int((~np.isfinite(got)).sum())} elements not written or not finite"
    ratio = R.worst_ratio(got, ref, tol)
    print(f"{case.name} {what}: worst error / tol {ratio:.3f}")
    assert ratio <= 1.0, (case.name, what, ratio)
    return ratio


# ------------------------------------------------------------------------------- one-launch self-attention and split
@pytest.mark.parametrize("path", [4, 3])
def test_every_key_count_in_one_launch(path):
    """448 rows, row r over r + 1 keys read from the device (nk_rows 1) under the host bound 448: every count of the
    one-launch kernel's seven bodies; on the split kernel S = 7 with neutral partials past the live keys."""
    case = R.self_every_count()
    check(case, run(case, path, device_counts=True, nk_rows=1), f"path {path}, device counts 1..448")


@pytest.mark.parametrize("n", R.SELF_HOST_KEYS)
def test_self_attention_host_counts(n):
    """5 rows at a host key count on each side of every 64-key pass; on the split kernel 1, 63 and 64 keys take the
    direct-write branch (S = 1, no device count)"""
    case = R.self_host(n)
    check(case, run(case, 4), "path 4, host count")
    check(case, run(case, 3), "path 3, host count")


@pytest.mark.parametrize("path", [4, 3])
def test_self_attention_shared_device_count(path):
    case = R.self_shared()
    check(case, run(case, path, device_counts=True, nk_rows=0), f"path {path}, one device count for all rows")


# ---------------------------------------------------------------------------------------- split + combine, cross shapes
@pytest.mark.parametrize("n", R.CROSS_KEYS)
def test_split_cross_shapes(n):
    """R = 1..8 rows per K/V batch, 3 batches of different data, ldq = D; 1500 keys end in a 28-key chunk"""
    worst = 0.0
    for rpk in range(1, 9):
        case = R.cross(rpk, n)
        worst = max(worst, check(case, run(case, 3), "path 3"))
    print(f"cross n_keys {n}: worst error / tol over R = 1..8 {worst:.3f}")


def test_split_80_rows():
    case = R.cross_80()
    check(case, run(case, 3), "path 3, 16 batches of 5 at 1500 keys")


@pytest.mark.parametrize("make", [R.cross_underflow, R.cross_equal])
def test_split_hard_cases(make):
    """a chunk whose combine factor exp(m_c - M) underflows, and all scores equal"""
    case = make()
    check(case, run(case, 3), "path 3")
    check(case, run(case, 2), "path 2")


# --------------------------------------------------------------------------------------------------------- row kernel
def test_row_kernel_causal():
    """the prefill: 300 rows of one K/V batch, row r over keys 0..r -- every count 1..300, so every residue of the
    128-key and 32-key P.V loops, twice"""
    case = R.row_causal()
    check(case, run(case, 2, causal=1), "path 2, causal")


@pytest.mark.parametrize("n", R.ROW_KEYS)
def test_row_kernel(n):
    for rpk in R.ROW_RPK:
        case = R.row_plain(n, rpk)
        check(case, run(case, 2), "path 2")


# ------------------------------------------------------------------------------------------------- the step's routing
def _same(a, b):
    return np.array_equal(a, b)


def test_paths_0_and_1_are_the_step_routes(monkeypatch):
    """Paths 0 and 1 give the bits of the path that the decode step's routing names, under each switch."""
    for name in ("CBW_DEC_SPLIT", "CBW_DEC_SELF_ONE", "CBW_DEC_SELF_SPLIT"):
        monkeypatch.delenv(name, raising=False)
    s = R.self_host(129)
    c5, c10 = R.cross(5, 1500), R.row_plain(257, 10)
    named = {p: run(s, p, raw=True) for p in (2, 3, 4)}
    assert _same(run(s, 0, raw=True), named[4])                                   # self: one launch
    assert _same(run(c5, 1, raw=True), run(c5, 3, raw=True))                      # cross, <= 8 rows per batch: split
    assert _same(run(c10, 1, raw=True), run(c10, 2, raw=True))                    # cross, 10 rows per batch: row kernel
    sd = R.self_80()
    assert _same(run(sd, 0, device_counts=True, nk_rows=1, raw=True), run(sd, 4, device_counts=True, nk_rows=1, raw=True))
    monkeypatch.setenv("CBW_DEC_SELF_ONE", "0")
    assert _same(run(s, 0, raw=True), named[3])                                   # self on split + combine
    assert _same(run(sd, 0, device_counts=True, nk_rows=1, raw=True), run(sd, 3, device_counts=True, nk_rows=1, raw=True))
    monkeypatch.setenv("CBW_DEC_SELF_SPLIT", "129")
    assert _same(run(s, 0, raw=True), named[2])                                   # up to 129 keys: row kernel
    monkeypatch.setenv("CBW_DEC_SELF_SPLIT", "128")
    assert _same(run(s, 0, raw=True), named[3])
    monkeypatch.delenv("CBW_DEC_SELF_ONE")
    monkeypatch.delenv("CBW_DEC_SELF_SPLIT")
    monkeypatch.setenv("CBW_DEC_SPLIT", "0")
    assert _same(run(s, 0, raw=True), named[2])                                   # everything on the row kernel
    assert _same(run(c5, 1, raw=True), run(c5, 2, raw=True))
    assert _same(run(sd, 0, device_counts=True, nk_rows=1, raw=True),             # but device counts need the split kernel
                 run(sd, 3, device_counts=True, nk_rows=1, raw=True))


# ------------------------------------------------------------------------------------------------------ bit-level claims
def test_two_runs_give_identical_bits():
    for case, path, kw in [(R.self_80(), 4, dict(device_counts=True, nk_rows=1)),
                           (R.self_80(), 3, dict(device_counts=True, nk_rows=1)),
                           (R.cross_80(), 3, {}), (R.cross(8, 1500), 3, {}), (R.row_plain(1500, 5), 2, {}),
                           (R.row_causal(), 2, dict(causal=1))]:
        assert _same(run(case, path, raw=True, **kw), run(case, path, raw=True, **kw)), (case.name, path)


def test_one_launch_row_bits_do_not_depend_on_the_row_count():
    case = R.self_80()
    full = run(case, 4, device_counts=True, nk_rows=1, raw=True)
    check(case, run(case, 4, device_counts=True, nk_rows=1), "path 4, 80 rows")
    for r in (0, 41, 79):
        assert _same(run(case, 4, device_counts=True, nk_rows=1, rows=(r, 1), raw=True)[0], full[r]), r


def _first_rows(case, keep):
    """the case with only the first `keep` rows of every K/V batch"""
    rows = np.concatenate([np.arange(b * case.rows_per_kv, b * case.rows_per_kv + keep) for b in range(case.k.shape[0])])
    sub = R.Case(f"{case.name}_first{keep}", case.q[rows].contiguous(), case.k, case.v, case.counts[rows], keep,
                 case.n_keys, case.H, case.D)
    return sub, rows


@pytest.mark.parametrize("n", [128, 1500])
def test_split_row_bits_do_not_depend_on_rows_per_batch(n):
    """Rows 0..R'-1 of every batch launched as R' = 2..8 rows per batch carry the same bits; R' = 1 runs another
    template, so there only the bound is asserted and the agreement reported."""
    case = R.cross(8, n)
    full = run(case, 3, raw=True)
    for keep in range(2, 8):
        sub, rows = _first_rows(case, keep)
        assert _same(run(sub, 3, raw=True), full[rows]), keep
    sub, rows = _first_rows(case, 1)
    ref, tol = ref_of(case)
    _REF[sub.name] = (ref[rows], tol[rows])
    check(sub, run(sub, 3), "path 3, R = 1 of the R = 8 data")
    print(f"{sub.name}: R = 1 bits equal R = 8 bits: {_same(run(sub, 3, raw=True), full[rows])}")


# --------------------------------------------------------------------------------------------------------- probabilities
@pytest.mark.parametrize("T", R.PROB_T)
@pytest.mark.parametrize("n", R.PROB_KEYS)
def test_cross_probabilities(T, n):
    from cbw import _lib
    lib = _lib.load()
    case = R.probs_case(T, n)
    d = dev()
    q, k = case.q.to(d), case.k.to(d)
    out2 = run(case, 2)
    check(case, out2, "path 2")
    _, tol = ref_of(case)
    for head in (0, case.H - 1):
        out = torch.full((T, n), float("nan"), dtype=torch.float32, device=d)
        _lib.check(lib.cbw_decode_cross_probs(q.data_ptr(), case.ldq, k.data_ptr(), n, T, case.D, head, out.data_ptr(),
                                              _lib.stream_handle()), "cbw_decode_cross_probs")
        torch.cuda.synchronize()
        got = out.double().cpu().numpy()
        ref = R.probabilities(case, head)
        assert np.isfinite(got).all()
        ratio = float((np.abs(got - ref) / (1e-4 * ref + 1e-12)).max())
        sums = float(np.abs(got.sum(axis=1) - 1).max())
        sl = slice(64 * head, 64 * head + 64)
        back = float((np.abs(got @ R.f64(case.v[0, :n, sl]) - out2[:, sl]) / tol[:, sl]).max())
        print(f"{case.name} head {head}: worst error / bound {ratio:.3f}, row sums off by {sums:.2e}, "
              f"weights x v against path 2: {back:.3f} of the bound")
        assert ratio <= 1.0 and sums <= 1e-5 and back <= 1.0, (case.name, head, ratio, sums, back)


# -------------------------------------------------------------------------------------------------------------- refusals
def test_a_refused_call_leaves_out_untouched():
    from cbw import _lib
    lib = _lib.load()
    case = R.self_host(129)
    d = dev()
    q, k, v = case.q.to(d), case.k.to(d), case.v.to(d)
    B, H, D = case.B, case.H, case.D
    out = torch.full((B, D), float("nan"), dtype=torch.bfloat16, device=d)
    ws_floats = lib.cbw_decode_attention_ws_floats(B, H)
    ws = torch.empty(ws_floats, dtype=torch.float32, device=d)
    pos = torch.zeros(B, dtype=torch.int32, device=d)
    ok = dict(ldq=case.ldq, kv_bstride=case.kv_bstride, n_keys=case.n_keys, rows_per_kv=1, n_keys_pos=None, nk_rows=0,
              causal=0, path=3, B=B, H=H, D=D, ws=ws.data_ptr(), ws_floats=ws_floats)
    for kw in [dict(path=5), dict(path=2, rows_per_kv=0), dict(path=3, ws=None), dict(path=3, ws_floats=ws_floats - 1),
               dict(path=4, n_keys=449), dict(path=4, rows_per_kv=5), dict(path=3, causal=1),
               dict(path=2, n_keys_pos=pos.data_ptr()), dict(path=3, n_keys=case.kv_rows + 1), dict(path=2, H=H + 1),
               dict(path=4, ldq=case.ldq + 4), dict(path=3, B=B, rows_per_kv=2)]:
        a = {**ok, **kw}
        rc = lib.cbw_decode_attention(q.data_ptr(), a["ldq"], k.data_ptr(), v.data_ptr(), a["kv_bstride"], a["n_keys"],
                                      a["rows_per_kv"], a["n_keys_pos"], a["nk_rows"], a["causal"], a["path"],
                                      out.data_ptr(), a["B"], a["H"], a["D"], a["ws"], a["ws_floats"],
                                      _lib.stream_handle())
        assert rc == -1 and b"cbw_decode_attention:" in lib.cbw_last_error(), kw
    pout = torch.full((B, case.n_keys), float("nan"), dtype=torch.float32, device=d)
    for n_keys, T, head in [(0, B, 0), (1537, B, 0), (case.n_keys, 0, 0), (case.n_keys, B, H), (case.n_keys, B, -1)]:
        rc = lib.cbw_decode_cross_probs(q.data_ptr(), case.ldq, k.data_ptr(), n_keys, T, D, head, pout.data_ptr(),
                                        _lib.stream_handle())
        assert rc == -1 and b"cbw_decode_cross_probs" in lib.cbw_last_error(), (n_keys, T, head)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(pout).all()
