"""The kernels of the exact-decision tiers one by one, each against a float64 CPU reference of the same operands.

The fp32 tier (kws_exact.hip) is the ground truth of every `*_exact` test and of bench.py's audits, and the compensated
tier (the 3-term bf16 split on the tile kernels) and the band selection decide which pairs reach it.  Here every kernel
of the three runs alone through its building-block entry point (include/cbw.h, "the kernels of the exact-decision
tiers one by one") at the smallest shapes at which it can still go wrong: partial tiles, one output pixel more than a
tile, tiles that span two images, both sides of every dispatch switch.

Every assertion is per element against a bound derived from the arithmetic, never tuned to pass, with u = 2^-24 (the
unit roundoff of fp32):
  * n fp32 additions in any order over exact or correctly rounded products err by at most ~n u sum|terms|;
  * bf16 keeps 8 significant bits, so round-to-nearest-even errs by at most 2^-8 relative (half a unit in the last
    place, 2^(e-8) for a value in [2^e, 2^(e+1))), and a [hi | lo] pair by at most 2^-17 relative.
The bound of each kernel is stated at its test.  Each test prints its worst |err| / bound (pytest -s shows them;
docs/MEASUREMENT_LOG.md records the values observed on an MI355X), so a later reader sees the room each bound leaves.
"""
import functools

import numpy as np
import pytest
import torch

from cbw import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


# ------------------------------------------------------------------ helpers: device buffers, references, bounds
def dev():
    return torch.device("cuda:0")


def lib_():
    from cbw import _lib
    return _lib, _lib.load()


def to_dev(a):
    """A numpy array on the GPU, contiguous (uint16 bf16 bit patterns travel as int16)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(dev())


def ptr(t):
    return None if t is None else t.data_ptr()


def bf16_rne(x):
    """float32 -> (bf16 bit patterns uint16, their float32 values): round to nearest, ties to even, on the bits
    (finite inputs; subnormals included, they round like any other encoding)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return r, (r.astype(np.uint32) << 16).view(np.float32)


def split_hi_lo(x):
    """The compensated tier's split of fp32 values: hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32).
    Returns (hi bits, lo bits, hi, lo)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hb, hi = bf16_rne(x)
    lb, lo = bf16_rne(x - hi)
    return hb, lb, hi, lo


def conv64(x, w, stride, pad):
    """float64 conv of NHWC x with w [Cout][KH][KW][Cin] -> NHWC."""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.asarray(w, dtype=np.float64)).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(xt, wt, None, stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def check(name, got, ref, bound, say=True):
    """Per element |got - ref| <= bound (and got == ref exactly where the bound is 0); prints (unless the caller
    prints a summary over several calls) and returns the worst |err| / bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    zero = bound == 0
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    if say:
        print(f"exact-kernels {name}: worst |err| / bound = {ratio:.4g}")
    assert not err[zero].any(), f"{name}: {np.count_nonzero(err[zero])} elements differ where the bound is 0"
    if ratio > 1.0:
        i = np.unravel_index(np.argmax(np.where(zero, 0, err / np.where(zero, 1, bound))), err.shape)
        raise AssertionError(f"{name}: |err| / bound = {ratio:.4g} at {i}: got {got[i]!r} ref {ref[i]!r} "
                             f"bound {bound[i]:.3g}; {np.count_nonzero(err > bound)} of {err.size} elements over")
    return ratio


def frame_masks(n, L, T):
    """0/1 masks f32 [n][L][T], different per item and layer: zeros at the tail (0, 1 or 2 frames, so some rows keep
    their last frame), one in the middle, and frame 0 on every other (item, layer)."""
    m = np.ones((n, L, T), np.float32)
    for i in range(n):
        for l in range(L):
            tail = (i + 2 * l) % 3
            if tail:
                m[i, l, T - tail:] = 0
            m[i, l, T // 2 - (i + l) % 2] = 0
            if (i + l) % 2 == 0:
                m[i, l, 0] = 0
    return m


def sim64(kwd, utt):
    """float64 inner products of kwd [K][L][Tk][E] with utt [B][L][Tu][E] -> [B][K][L][Tk][Tu]."""
    return np.matmul(kwd[None], np.swapaxes(utt, -1, -2)[:, None])


def unit_rows(rng, shape):
    """L2-normalised rows (as the projector produces them), float32."""
    x = rng.standard_normal(shape)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------ fp32 conv (conv_f32_kernel<true> / <false>)
# N, H, W, Cin, Cout, k, stride, pad, what (1 bias | 2 residual | 4 ReLU).  Cin % 16 == 0 runs conv_f32_kernel<true>
# (float4 loads, a 16-wide K-step inside one tap), any other Cin conv_f32_kernel<false> (element-wise, K tail).
F32_CONV_CASES = [
    # the stem: 7x7 s2 p3, K = 49 Cin is no multiple of 16 (147 at Cin = 3); M = 300 / 1116: tiles span images
    (3, 9, 40, 3, 64, 7, 2, 3, 1 | 4),
    (3, 23, 61, 3, 64, 7, 2, 3, 1 | 4),
    (3, 9, 40, 1, 64, 7, 2, 3, 1),
    (3, 23, 61, 1, 64, 7, 2, 3, 4),
    (3, 9, 40, 4, 64, 7, 2, 3, 1 | 2 | 4),
    (3, 23, 61, 4, 64, 7, 2, 3, 0),
    (2, 7, 13, 16, 64, 1, 1, 0, 1 | 4),       # 1x1, the smallest vector path: a K-step is exactly one tap; M = 182
    (2, 19, 37, 64, 64, 1, 1, 0, 1 | 4),      # 1x1 stage-1 reduce; M = 1406, Ho Wo = 703 (a tile spans two images)
    (2, 9, 11, 64, 256, 1, 1, 0, 1 | 2 | 4),  # 1x1 expand with residual, four channel tiles
    (1, 10, 23, 256, 64, 1, 1, 0, 1 | 4),     # 1x1 256 -> 64
    (2, 19, 37, 64, 128, 1, 2, 0, 1),         # 1x1 s2 (the projection shortcut) at odd H, W: 10 x 19
    (2, 7, 13, 16, 64, 3, 1, 1, 1 | 4),       # 3x3 s1 p1, one tap per K-step
    (2, 19, 37, 64, 64, 3, 1, 1, 1 | 4),      # 3x3 s1 p1 stage 1
    (2, 19, 37, 64, 64, 3, 2, 1, 1 | 4),      # 3x3 s2 p1 at odd H, W
    (2, 10, 24, 128, 128, 3, 2, 1, 1 | 2),    # 3x3 s2 p1 at even H, W
    (1, 5, 7, 64, 64, 1, 1, 0, 1 | 2 | 4),    # M = 35 < 64
    (1, 5, 7, 16, 64, 3, 1, 1, 2),            # M = 35 < 64, 3x3
    (1, 5, 13, 64, 64, 1, 1, 0, 1 | 4),       # M = 65 = 64 + 1
    (1, 5, 13, 32, 64, 3, 1, 1, 1 | 2 | 4),   # M = 65, 3x3
    (3, 3, 43, 48, 64, 3, 1, 1, 1 | 4),       # M = 387 = 64 * 6 + 3, N = 3, Cin = 48 (three K-steps per tap)
]


def run_conv_f32(rng, N, H, W, Cin, Cout, k, stride, pad, what):
    _lib, lib = lib_()
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((Cout, k, k, Cin)) / np.sqrt(k * k * Cin)).astype(np.float32)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    bias = rng.standard_normal(Cout).astype(np.float32) if what & 1 else None
    res = rng.standard_normal((N, Ho, Wo, Cout)).astype(np.float32) if what & 2 else None
    xd, wd = to_dev(x), to_dev(w)
    bd = None if bias is None else to_dev(bias)
    rd = None if res is None else to_dev(res)
    y = torch.full((N, Ho, Wo, Cout), float("nan"), dtype=torch.float32, device=dev())
    _lib.check(lib.cbw_conv2d_f32(xd.data_ptr(), wd.data_ptr(), ptr(bd), ptr(rd), y.data_ptr(), N, H, W, Cin, Cout, k, k,
                                  stride, stride, pad, pad, 1 if what & 4 else 0, _lib.stream_handle()),
               "cbw_conv2d_f32")
    torch.cuda.synchronize()
    ref = conv64(x, w, stride, pad)
    A = conv64(np.abs(x), np.abs(w), stride, pad)
    if bias is not None:
        ref = ref + bias.astype(np.float64)
        A = A + np.abs(bias.astype(np.float64))
    if res is not None:
        ref = ref + res.astype(np.float64)
        A = A + np.abs(res.astype(np.float64))
    if what & 4:
        ref = np.maximum(ref, 0)   # |relu(a) - relu(b)| <= |a - b|: the bound carries over
    return y.cpu().numpy(), ref, (k * k * Cin + 4) * U * A


@pytest.mark.parametrize("case", F32_CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_f32_vs_float64(case):
    """|got - ref| <= (K + 4) u A per element, K = KH KW Cin, A = (|x| conv |w|) + |bias| + |res| in float64: fp32
    accumulation of K exact (or correctly rounded) products in any order errs by at most ~K u sum|x||w|, the bias
    and the residual add one rounding each."""
    got, ref, bound = run_conv_f32(np.random.default_rng(1000 + F32_CONV_CASES.index(case)), *case)
    check(f"conv_f32 {case}", got, ref, bound)


@pytest.mark.parametrize("what", range(8))
def test_conv_f32_epilogue_combinations(what):
    """Every combination of bias, residual and ReLU on both load paths, same bound."""
    for j, (Cin, k, stride, pad) in enumerate([(16, 3, 1, 1), (3, 7, 2, 3)]):
        got, ref, bound = run_conv_f32(np.random.default_rng(2000 + 2 * what + j), 2, 9, 13, Cin, 64, k, stride, pad,
                                       what)
        check(f"conv_f32 epilogue {what} Cin {Cin}", got, ref, bound)


# ------------------------------------------------------------------ fp32 similarity maps
# E, L, Tk, Tu.  E == 64 with L Tk 260 <= 131072 bytes of LDS: sim_f32_e64_kernel / sim_f32_e64_pairs_kernel (one
# block per 256 utterance frames); everything else sim_f32_kernel / sim_f32_pairs_kernel (one block per keyword frame).
SIM_F32_CASES = [
    (64, 3, 75, 257),    # e64, the production Tk; the second 256-frame block holds one frame
    (64, 1, 7, 7),
    (64, 4, 15, 513),
    (64, 3, 15, 255),
    (64, 4, 7, 256),
    (64, 3, 168, 7),     # 3 * 168 * 260 = 131040 <= 131072: still the LDS kernel
    (64, 3, 169, 7),     # 131820: falls back to the generic kernel at E = 64
    (64, 4, 126, 9),     # 131040: LDS
    (64, 4, 127, 9),     # 132080: generic
    (32, 3, 15, 257),    # generic
    (68, 3, 7, 255),     # E % 4 == 0, no multiple of 32
    (128, 4, 75, 7),
    (128, 1, 15, 513),
    (384, 3, 7, 256),
    (384, 4, 15, 17),
]


def sim_maps_f32(utt, um, B, kwd, km, pair_utt, pair_kwd, n_pairs, sel, p0, P):
    """cbw_sim_maps_f32 on device tensors -> numpy f32 [P][Tk][Tu][L]."""
    _lib, lib = lib_()
    K, L, Tk, E = kwd.shape
    Tu = utt.shape[-2]
    out = torch.full((P, Tk, Tu, L), float("nan"), dtype=torch.float32, device=dev())
    _lib.check(lib.cbw_sim_maps_f32(utt.data_ptr(), um.data_ptr(), B, kwd.data_ptr(), km.data_ptr(), K, L, Tk, Tu, E,
                                    ptr(pair_utt), ptr(pair_kwd), n_pairs, sel.data_ptr(), p0, P, out.data_ptr(),
                                    _lib.stream_handle()), "cbw_sim_maps_f32")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", SIM_F32_CASES, ids=lambda c: "x".join(map(str, c)))
def test_sim_maps_f32_vs_float64(case):
    """|got - ref| <= (E + 4) u sum_e |k_e||u_e| mask per element: E fused multiply-adds in fp32 and the two mask
    products; a masked element is exactly 0.  The one-utterance form (sel unordered with a repeated keyword, p0 > 0),
    the explicit pair list and the NULL pair list (q = b K + k) over B = 3 utterances: the pair forms must equal the
    one-utterance maps bit for bit and meet the same bound."""
    E, L, Tk, Tu = case
    K, B = 3, 3
    rng = np.random.default_rng(3000 + SIM_F32_CASES.index(case))
    kwd, utt = unit_rows(rng, (K, L, Tk, E)), unit_rows(rng, (B, L, Tu, E))
    km, um = frame_masks(K, L, Tk), frame_masks(B, L, Tu)[:, ::-1].copy()
    k64, u64 = kwd.astype(np.float64), utt.astype(np.float64)
    mask = np.einsum("kli,blj->bkijl", km.astype(np.float64), um.astype(np.float64))
    ref = sim64(k64, u64).transpose(0, 1, 3, 4, 2) * mask                      # [B][K][Tk][Tu][L]
    bound = (E + 4) * U * sim64(np.abs(k64), np.abs(u64)).transpose(0, 1, 3, 4, 2) * mask
    assert (mask == 0).any() and (mask[..., -1, -1, :] == 1).any()             # masked elements and live last frames
    kd, kmd, ud, umd = to_dev(kwd), to_dev(km), to_dev(utt), to_dev(um)
    i32 = lambda a: to_dev(np.asarray(a, dtype=np.int32))  # noqa: E731

    # one utterance: sel unordered with a repeat, every keyword named, p0 = 1
    order = list(reversed(range(K)))
    order.insert(1, order[-1])
    sel = [K - 1] + order
    one, worst = {}, 0.0
    for b in range(B):
        got = sim_maps_f32(ud[b], umd[b], 0, kd, kmd, None, None, 0, i32(sel), 1, len(order))
        for p, k in enumerate(order):
            worst = max(worst, check(f"sim_f32 {case} one-utterance b={b} k={k}", got[p], ref[b, k], bound[b, k], say=False))
            if (b, k) in one:
                assert np.array_equal(one[(b, k)].view(np.uint32), got[p].view(np.uint32)), "repeated keyword differs"
            one[(b, k)] = got[p]
    assert len(one) == B * K

    # explicit pair list: every (b, k) in a scrambled order, one pair twice; sel scrambled with a repeat, p0 = 2
    pairs = [(b, k) for b in range(B) for k in range(K)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))] + [pairs[0]]
    sel_p = list(rng.permutation(len(pairs))) + [3]
    sel_full = [0, 0] + sel_p
    got = sim_maps_f32(ud, umd, B, kd, kmd, i32([p[0] for p in pairs]), i32([p[1] for p in pairs]), len(pairs),
                       i32(sel_full), 2, len(sel_p))
    for p, q in enumerate(sel_p):
        b, k = pairs[q]
        assert np.array_equal(got[p].view(np.uint32), one[(b, k)].view(np.uint32)), f"pair ({b}, {k}) != one-utterance map"
        worst = max(worst, check(f"sim_f32 {case} pairs ({b}, {k})", got[p], ref[b, k], bound[b, k], say=False))

    # NULL pair list: q = b K + k
    sel_q = list(rng.permutation(B * K)) + [B * K - 1]
    got = sim_maps_f32(ud, umd, B, kd, kmd, None, None, B * K, i32([1] + sel_q), 1, len(sel_q))
    for p, q in enumerate(sel_q):
        b, k = divmod(int(q), K)
        assert np.array_equal(got[p].view(np.uint32), one[(b, k)].view(np.uint32)), f"pair q={q} != one-utterance map"
        worst = max(worst, check(f"sim_f32 {case} cross product q={q}", got[p], ref[b, k], bound[b, k], say=False))
    print(f"exact-kernels sim_f32 {case}: worst over all forms = {worst:.4g}")


# ------------------------------------------------------------------ max-pool, pool + fc, split, channel sums
@pytest.mark.parametrize("shape", [(2, 5, 20, 64), (2, 12, 31, 64), (1, 1, 9, 64), (3, 8, 1, 4), (1, 1, 1, 3),
                                   (2, 6, 6, 5), (1, 2, 2, 64)], ids=str)
def test_maxpool_f32_exact(shape):
    """Exactly MaxPool2d(3, 2, 1) with -inf padding (inputs mostly negative, so a zero pad would show)."""
    _lib, lib = lib_()
    N, H, W, C = shape
    rng = np.random.default_rng(4000 + H * 100 + W)
    x = (rng.standard_normal(shape) - 1.5).astype(np.float32)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xd = to_dev(x)
    y = torch.full((N, Ho, Wo, C), float("nan"), dtype=torch.float32, device=dev())
    _lib.check(lib.cbw_maxpool_f32(xd.data_ptr(), y.data_ptr(), N, H, W, C, _lib.stream_handle()), "cbw_maxpool_f32")
    torch.cuda.synchronize()
    ref = torch.nn.functional.max_pool2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert tuple(ref.shape) == (N, Ho, Wo, C)
    assert (x < 0).any()
    np.testing.assert_array_equal(y.cpu().numpy().astype(np.float64), ref.numpy())
    print(f"exact-kernels maxpool_f32 {shape}: exact")


@pytest.mark.parametrize("C", [512, 2048])
@pytest.mark.parametrize("HW", [1, 7, 8, 9, 72])
def test_pool_fc_f32_vs_float64(HW, C):
    """|got - ref| <= (HW + C + 4) u sum|x||w| / HW + u |b|: HW additions per channel mean, one division, C fused
    multiply-adds and the tree over lanes and waves, the bias.  Rows sel does not name keep their sentinel."""
    _lib, lib = lib_()
    P, R = 3, 7
    rng = np.random.default_rng(5000 + HW * 10 + C)
    x = rng.standard_normal((P, HW, C)).astype(np.float32)
    w = (rng.standard_normal((2, C)) / np.sqrt(C)).astype(np.float32)
    b = rng.standard_normal(2).astype(np.float32)
    sel = np.array([6, 5, 0, 3, 1], np.int32)   # p0 = 2: rows 0, 3, 1 receive x[0], x[1], x[2]
    sentinel = -12345.5
    logits = torch.full((R, 2), sentinel, dtype=torch.float32, device=dev())
    xd, wd, bd, sd = to_dev(x), to_dev(w), to_dev(b), to_dev(sel)
    _lib.check(lib.cbw_pool_fc_f32(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), sd.data_ptr(), 2, P, logits.data_ptr(),
                                   HW, C, _lib.stream_handle()), "cbw_pool_fc_f32")
    torch.cuda.synchronize()
    got = logits.cpu().numpy()
    rows = sel[2:]
    untouched = np.setdiff1d(np.arange(R), rows)
    assert (got[untouched] == sentinel).all(), "a row sel does not name was written"
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    ref = np.einsum("phc,oc->po", x64, w64) / HW + b.astype(np.float64)
    bound = (HW + C + 4) * U * np.einsum("phc,oc->po", np.abs(x64), np.abs(w64)) / HW + U * np.abs(b.astype(np.float64))
    check(f"pool_fc_f32 HW={HW} C={C}", got[rows], ref, bound)


@pytest.mark.parametrize("C", [4, 64, 68])
def test_split3_f32_exact(C):
    """Exactly hi = bf16_rne(x), lo = bf16_rne(x - hi), bit for bit: values across many binades, values that round up
    into the next binade, exact ties (to even, both ways), zeros of both signs and fp32 / bf16 subnormals."""
    _lib, lib = lib_()
    M = 37
    rng = np.random.default_rng(6000 + C)
    x = (rng.standard_normal((M, C)) * np.exp2(rng.integers(-20, 20, (M, C)))).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0,
                        np.float32(2.0) - np.float32(2.0 ** -23), -(np.float32(4.0) - np.float32(2.0 ** -22)),  # round up
                        1.99609375 + 2.0 ** -9, 255.5,                    # 1.1111111|1 and 11111111|.1: up to 2 / 256
                        1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,              # ties: down to 1 (even), up to 1 + 2^-6
                        1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23,
                        1e-39, -1e-39, 1e-40, 2.0 ** -149, 2.0 ** -126, 2.0 ** -133 * 1.5, 3e-38, -1.5e-38,
                        65504.0, 1e30, -3.3e38 / 1.5], dtype=np.float32)
    x.reshape(-1)[:special.size] = special
    x.reshape(-1)[-special.size:] = -special
    xd = to_dev(x)
    y = torch.zeros((M, 2 * C), dtype=torch.int16, device=dev())
    _lib.check(lib.cbw_split3_f32(xd.data_ptr(), y.data_ptr(), M, C, _lib.stream_handle()), "cbw_split3_f32")
    torch.cuda.synchronize()
    got = y.cpu().numpy().view(np.uint16)
    hb, lb, hi, lo = split_hi_lo(x)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    assert hi.reshape(-1)[4] == 2.0 and hi.reshape(-1)[7] == 256.0 and hi.reshape(-1)[8] == 1.0   # the reference rounds so
    np.testing.assert_array_equal(got[:, :C], hb, err_msg="hi")
    np.testing.assert_array_equal(got[:, C:], lb, err_msg="lo")
    print(f"exact-kernels split3 C={C}: exact")


@pytest.mark.parametrize("C", [3, 4, 64, 200, 256, 512])
def test_channel_sum_f32_vs_float64(C):
    """After the G partials are summed in float64: |got - ref| <= M u sum|x| per channel (fewer than M fp32 additions
    per channel, in any grouping).  C >= 256 takes the one-channel-per-thread path, C < 256 the row-lane path
    (C = 3 is what the calibration feeds it for the maps); M = 1, 63, 64, 65 put 0 or 1 row in a workgroup."""
    _lib, lib = lib_()
    nbytes = lib.cbw_channel_sum_workspace_bytes(C)
    assert nbytes > 0 and nbytes % (4 * C) == 0
    G = nbytes // (4 * C)
    worst = 0.0
    for M in (1, 63, 64, 65, 1000):
        rng = np.random.default_rng(7000 + C * 7 + M)
        x = (rng.standard_normal((M, C)) + 0.5).astype(np.float32)
        xd = to_dev(x)
        part = torch.zeros((G, C), dtype=torch.float32, device=dev())
        _lib.check(lib.cbw_channel_sum_f32(xd.data_ptr(), M, C, part.data_ptr(), nbytes, _lib.stream_handle()),
                   "cbw_channel_sum_f32")
        torch.cuda.synchronize()
        got = part.cpu().numpy().astype(np.float64).sum(0)
        x64 = x.astype(np.float64)
        worst = max(worst, check(f"channel_sum C={C} M={M}", got, x64.sum(0), M * U * np.abs(x64).sum(0),
                                 say=False))
    print(f"exact-kernels channel_sum C={C}: worst over M = {worst:.4g}")


# ------------------------------------------------------------------ one conv of the compensated tier
# N, H, W, C, Cout, k, stride, residual (0 none, 1 fp32, 2 split), out_split, y32, relu
# At these sizes (fewer tiles than CUs) cbw_conv_igemm runs the 4-wave tile kernels: the 256 x 64 tile at Cout = 64, the
# 128 x 128 tile at Cout % 128 == 0 (its persistent form with a residual).  The 256-wide tiles the tier takes at
# production sizes are held bit-identical to these by test_gpu_kws.py::test_compensated_tier_on_p8_bit_identical.
X3_CASES = [
    (2, 9, 13, 64, 64, 1, 1, 0, 1, 0, 1),      # stage-1 1x1 reduce -> [hi | lo]
    (2, 9, 13, 64, 64, 3, 1, 0, 1, 0, 1),      # stage-1 3x3
    (2, 9, 13, 64, 256, 1, 1, 0, 0, 0, 0),     # stage-1 projection shortcut: fp32 out, no ReLU
    (2, 9, 13, 64, 256, 1, 1, 1, 1, 1, 1),     # stage-1 expand, fp32 residual (the shortcut), [hi | lo] + y32
    (2, 9, 13, 64, 256, 1, 1, 2, 1, 1, 1),     # stage-1 identity expand, split residual
    (2, 11, 19, 128, 128, 3, 2, 0, 1, 0, 1),   # stage-2 strided 3x3 at odd H, W: 6 x 10
]


@pytest.mark.parametrize("case", X3_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_x3_vs_float64(case):
    """One conv of the compensated tier against the float64 conv of the fp32 values it stands for: x = x_hi + x_lo
    (exactly what the kernel reads) and the unsplit fp32 w.

    |got - ref| <= (3 2^-18 + (3K + 4) u) A, K = k k C, A = (|x| conv |w|) + |bias| + |res|.

    Where the two terms come from.  For w in [2^e, 2^(e+1)): w_hi = bf16(w) leaves r = w - w_hi, exact in fp32, with
    |r| <= 2^(e-8); either r is that power of two (then w_lo = r exactly) or it lies a binade lower and w_lo = bf16(r)
    errs by at most 2^(e-17): the split residue is |w - w_hi - w_lo| <= 2^-17 |w|, and |w_lo| <= 2^-8 |w|; the same for
    x, whose residue does not count here because the reference takes x = x_hi + x_lo.  The kernel sums x_hi w_hi +
    x_hi w_lo + x_lo w_hi = x (w_hi + w_lo) - x_lo w_lo, so each product is off by the weight residue times |x| plus
    the dropped lo.lo term, at most (2^-17 + 2^-16) |x||w| = 6 2^-18 |x||w| -- and that only when both mantissas sit
    just above a power of two with residues of the largest size.  Averaged over mantissas the two are ~0.35 2^-17 and
    ~0.5 2^-18 of |x||w| with signs independent from tap to tap, so over K >= 64 taps their sum is a random walk of
    ~2^-18 A / sqrt(K): the bound's 3 2^-18 A (half the per-product worst case) is what a correct kernel meets with
    a wide margin on seeded normal operands, while a lost segment still shows (x_hi w_lo or x_lo w_hi missing costs
    ~2^-9.5 A / sqrt(K), several times the whole bound at the 1x1 convs' K = 64).  The second term is rigorous: the
    3K bf16 products are exact in fp32 and their fp32 accumulation in any order errs by at most (3K - 1) u times the
    sum of their magnitudes (<= 1.012 A), bias and residual add a rounding each.  For the [hi | lo] output, hi + lo
    is the split of v, off by at most 2^-17 |v| as above: a further 2^-17 |ref|; y32 is v itself, and the split must
    be y32's, bit for bit."""
    _lib, lib = lib_()
    N, H, W, C, Cout, k, stride, res_kind, out_split, want_y32, relu = case
    rng = np.random.default_rng(8000 + X3_CASES.index(case))
    xh, xl, x_hi, x_lo = split_hi_lo(rng.standard_normal((N, H, W, C)))
    w = (rng.standard_normal((Cout, k, k, C)) / np.sqrt(k * k * C)).astype(np.float32)
    wh, wl, _, _ = split_hi_lo(w)
    bias = rng.standard_normal(Cout).astype(np.float32)
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    M = N * Ho * Wo
    x64 = x_hi.astype(np.float64) + x_lo.astype(np.float64)
    ref = conv64(x64, w, stride, k // 2) + bias.astype(np.float64)
    A = conv64(np.abs(x64), np.abs(w), stride, k // 2) + np.abs(bias.astype(np.float64))
    rd = None
    if res_kind:
        r32 = rng.standard_normal((N, Ho, Wo, Cout)).astype(np.float32)
        if res_kind == 2:
            rh, rl, r_hi, r_lo = split_hi_lo(r32)
            rd = to_dev(np.concatenate([rh, rl], -1))        # [M][2 Cout] = [hi | lo]
            r64 = r_hi.astype(np.float64) + r_lo.astype(np.float64)
        else:
            rd, r64 = to_dev(r32), r32.astype(np.float64)
        ref, A = ref + r64, A + np.abs(r64)
    if relu:
        ref = np.maximum(ref, 0)
    xd = to_dev(np.concatenate([xh, xl], -1))                # [N][H][W][2C] = [hi | lo]
    wd = to_dev(np.concatenate([wh, wl, wh], -1))            # [Cout][k][k][3C] = [w_hi | w_lo | w_hi]
    bd = to_dev(bias)
    y = (torch.zeros((M, 2 * Cout), dtype=torch.int16, device=dev()) if out_split else
         torch.full((M, Cout), float("nan"), dtype=torch.float32, device=dev()))
    y32 = torch.full((M, Cout), float("nan"), dtype=torch.float32, device=dev()) if want_y32 else None
    _lib.check(lib.cbw_conv2d_x3(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), ptr(rd), 1 if res_kind == 2 else 0,
                                 y.data_ptr(), ptr(y32), out_split, N, H, W, C, Cout, k, stride, relu,
                                 _lib.stream_handle()), "cbw_conv2d_x3")
    torch.cuda.synchronize()
    ref, A = ref.reshape(M, Cout), A.reshape(M, Cout)
    bound = (3 * 2.0 ** -18 + (3 * k * k * C + 4) * U) * A
    if out_split:
        bits = y.cpu().numpy().view(np.uint16).astype(np.uint32) << 16
        v = bits.view(np.float32).astype(np.float64)
        check(f"conv_x3 {case} hi + lo", v[:, :Cout] + v[:, Cout:], ref, bound + 2.0 ** -17 * np.abs(ref))
        if want_y32:
            got32 = y32.cpu().numpy()
            check(f"conv_x3 {case} y32", got32, ref, bound)
            hb, lb, _, _ = split_hi_lo(got32)                 # the split output is the split of y32, bit for bit
            np.testing.assert_array_equal(bits[:, :Cout] >> 16, hb)
            np.testing.assert_array_equal(bits[:, Cout:] >> 16, lb)
    else:
        check(f"conv_x3 {case} fp32", y.cpu().numpy(), ref, bound)


# ------------------------------------------------------------------ bf16 similarity maps, every element
# kernel kind -> (hparams without n_layers, E): which map kernel cbw_kws_score / cbw_kws_score_pairs dispatches to
BF16_SIM_KINDS = {
    # E == 32: sim_maps_rows_kernel<1> / sim_maps_rows_pairs_kernel<1> (the L variant on raw 32-wide states)
    "rows1_L_E32": (dict(embedding_dim=32, learn_features=False, proj_mlp=False), 32),
    # E == 64: sim_maps_rows_kernel<2> / sim_maps_rows_pairs_kernel<2> (LE: proj_mlp_units = 64)
    "rows2_LE_E64": (dict(embedding_dim=128, learn_features=True, proj_mlp=True, frames_conv=False,
                          proj_mlp_units=64, resnet_version="resnet-18"), 64),
    # any other E % 32 == 0: sim_maps_kernel / sim_maps_pairs_kernel (the L variant)
    "tile_L_E96": (dict(embedding_dim=96, learn_features=False, proj_mlp=False), 96),
    "tile_L_E128": (dict(embedding_dim=128, learn_features=False, proj_mlp=False), 128),
}
BF16_SIM_SHAPES = [(7, 7), (15, 17), (16, 64), (17, 65), (23, 61), (75, 750)]


@functools.lru_cache(maxsize=None)
def sim_engine(kind, L):
    from cbw.kws import KwsEngine
    hp = dict(BF16_SIM_KINDS[kind][0], n_layers=L)
    return KwsEngine(hp, synth.synth_kws_state_dict(seed=11, **hp))


@pytest.mark.parametrize("L", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", list(BF16_SIM_KINDS))
def test_bf16_sim_maps_every_element(kind, L):
    """KwsEngine.score / score_pairs with features=True: the whole [K][L][Tk][Tu] map against float64 over the same
    bf16 rows and masks, |got - ref| <= 2^-8 |ref| + (E + 4) u per element (fp32 accumulation of E exact bf16
    products of unit rows, one bf16 rounding of the output), masked elements exactly 0.  Every element, so the
    partial 16 x 16 tiles at the last rows and columns count (Tk, Tu = 7, 15, 17, 23, 61, 65, 75, 750)."""
    eng, E = sim_engine(kind, L), BF16_SIM_KINDS[kind][1]
    assert eng.feat_dim == E and eng.n_layers == L
    K, B = 3, 3
    d = eng.device
    worst = 0.0
    for si, (Tk, Tu) in enumerate(BF16_SIM_SHAPES):
        rng = np.random.default_rng(9000 + 100 * L + 10 * list(BF16_SIM_KINDS).index(kind) + si)
        kwd = torch.from_numpy(unit_rows(rng, (K, L, Tk, E))).to(torch.bfloat16)
        utt = torch.from_numpy(unit_rows(rng, (B, L, Tu, E))).to(torch.bfloat16)
        km, um = frame_masks(K, L, Tk), frame_masks(B, L, Tu)[:, ::-1].copy()
        mask = np.einsum("kli,blj->bklij", km.astype(np.float64), um.astype(np.float64))
        ref = sim64(kwd.double().numpy(), utt.double().numpy()) * mask          # [B][K][L][Tk][Tu]
        bound = (2.0 ** -8 * np.abs(ref) + (E + 4) * U) * mask
        kd, ud, kmd, umd = kwd.to(d), utt.to(d), torch.from_numpy(km).to(d), torch.from_numpy(um).to(d)
        for b in (0, B - 1):
            _, feats = eng.score(ud[b], umd[b], kd, kmd, features=True)
            torch.cuda.synchronize()
            worst = max(worst, check(f"bf16 sim {kind} L={L} {Tk}x{Tu} utt {b}", feats.cpu().numpy(), ref[b], bound[b],
                                     say=False))
        pu, pk = [2, 0, 1, 2, 0], [0, 1, 2, 2, 0]
        _, feats = eng.score_pairs(ud, umd, kd, kmd, pu, pk, features=True)
        torch.cuda.synchronize()
        worst = max(worst, check(f"bf16 sim {kind} L={L} {Tk}x{Tu} pairs", feats.cpu().numpy(), ref[pu, pk],
                                 bound[pu, pk], say=False))
    print(f"exact-kernels bf16 sim {kind} L={L}: worst over shapes and forms = {worst:.4g}")


# ------------------------------------------------------------------ band selection (spot_kernel modes 2 and 3)
EDGE = 1e-5


def band_call(scaled, logits, ghost, thr, width):
    """cbw_kws_band / cbw_kws_band_scaled -> (indices int32 [n], n)."""
    _lib, lib = lib_()
    K = logits.shape[0]
    ld = to_dev(np.asarray(logits, np.float32).reshape(K, 2))
    gd = None if ghost is None else to_dev(np.asarray(ghost, np.float32))
    idx = torch.full((max(K, 1),), -1, dtype=torch.int32, device=dev())
    n = torch.full((1,), -1, dtype=torch.int32, device=dev())
    fn = lib.cbw_kws_band_scaled if scaled else lib.cbw_kws_band
    _lib.check(fn(ld.data_ptr(), ptr(gd), K, float(thr), float(width), idx.data_ptr(), n.data_ptr(),
                  _lib.stream_handle()), "cbw_kws_band")
    torch.cuda.synchronize()
    cnt = int(n.item())
    assert 0 <= cnt <= K
    return idx.cpu().numpy()[:cnt], cnt


def band_ref(scaled, logits, ghost, thr, width):
    """The restatement in float64 over the fp32 logits and the fp32 values of thr and the width (what the kernel is
    given): (hit [K] bool, distance of |p - thr| from the band's edge [K])."""
    l0, l1 = logits[:, 0].astype(np.float64), logits[:, 1].astype(np.float64)
    p = 1.0 / (1.0 + np.exp(l0 - l1))
    if ghost is not None:
        p = p * ghost.astype(np.float64)
    thr, width = float(np.float32(thr)), float(np.float32(width))
    half = width * np.maximum(np.abs(l0), np.abs(l1)) if scaled else np.full_like(p, width)
    dist = np.abs(p - thr)
    return dist <= half, np.abs(dist - half)


@pytest.mark.parametrize("with_ghost", [False, True], ids=["no_ghost", "ghost"])
@pytest.mark.parametrize("scaled", [False, True], ids=["band", "band_scaled"])
@pytest.mark.parametrize("K", [1, 63, 64, 1023, 1024, 1025, 5000])
def test_band_selection_vs_numpy(K, scaled, with_ghost):
    """idx must be exactly the sorted indices of hit = |p - thr| <= band (or <= coef max(|l0|, |l1|)), p = ghost /
    (1 + exp(l0 - l1)) in float64, and n their count.  The kernel works in fp32 (p is off by ~1e-7), so a pair closer
    than 1e-5 to the band's edge would be undecidable: the logits are redrawn until the reference itself has none,
    and no pair is left out of the comparison."""
    rng = np.random.default_rng(10000 + K * 4 + 2 * scaled + with_ghost)
    ghost = (rng.random(K) > 0.15).astype(np.float32) if with_ghost else None
    for thr, width in ([(0.5, 0.03), (0.3, 0.1), (0.9, 0.01)] if not scaled else [(0.5, 0.02), (0.3, 0.05), (0.7, 0.004)]):
        logits = (rng.standard_normal((K, 2)) * 1.5).astype(np.float32)
        for _ in range(100):
            hit, edge = band_ref(scaled, logits, ghost, thr, width)
            close = edge < EDGE
            if not close.any():
                break
            logits[close] = (rng.standard_normal((int(close.sum()), 2)) * 1.5).astype(np.float32)
        hit, edge = band_ref(scaled, logits, ghost, thr, width)
        assert (edge >= EDGE).all(), "reference pairs within 1e-5 of the band's edge"
        idx, n = band_call(scaled, logits, ghost, thr, width)
        want = np.nonzero(hit)[0]
        assert n == want.size, f"K={K} thr={thr} width={width}: n = {n}, numpy counts {want.size}"
        assert idx.tolist() == want.tolist()
        print(f"exact-kernels band K={K} scaled={scaled} ghost={with_ghost} thr={thr} width={width}: {n} hits, "
              f"closest pair {edge.min():.3g} from the edge")


@pytest.mark.parametrize("K", [64, 1025])
def test_band_selection_exact_cases(K):
    """The cases that sit on an edge by construction and are still exact in fp32."""
    rng = np.random.default_rng(11000 + K)
    far = np.stack([np.full(K, 3.0), np.full(K, -2.0)], 1).astype(np.float32)      # p = 1 / (1 + e^5) ~ 0.0067
    far += rng.integers(0, 4, (K, 2)).astype(np.float32)                            # p <= 1 / (1 + e^2) ~ 0.12
    every = np.arange(K).tolist()
    ties = sorted({0, K // 3, K - 1})
    tied = far.copy()
    tied[ties] = np.array([[0.25, 0.25], [-1.5, -1.5], [7.0, 7.0]], np.float32)[:len(ties)]
    # l0 == l1 gives p = 0.5 exactly: with thr = 0.5 and band = 0 a hit; away from the threshold band = 0 hits nothing
    idx, n = band_call(False, tied, None, 0.5, 0.0)
    assert (n, idx.tolist()) == (len(ties), ties)
    idx, n = band_call(False, far, None, 0.5, 0.0)
    assert (n, idx.tolist()) == (0, [])
    # coef = 0: the scaled band has zero width everywhere
    idx, n = band_call(True, tied, None, 0.5, 0.0)
    assert (n, idx.tolist()) == (len(ties), ties)
    idx, n = band_call(True, far, None, 0.5, 0.0)
    assert (n, idx.tolist()) == (0, [])
    # every pair hits: |p - thr| <= 1 always; the scaled band with coef 1 and max|l| >= 2 likewise
    idx, n = band_call(False, tied, None, 0.5, 1.0)
    assert (n, idx.tolist()) == (K, every)
    idx, n = band_call(True, far, None, 0.5, 1.0)
    assert (n, idx.tolist()) == (K, every)
    # no pair hits: p <= 0.12 is at least 0.35 from 0.5
    idx, n = band_call(False, far, None, 0.5, 0.03)
    assert (n, idx.tolist()) == (0, [])
    idx, n = band_call(True, far, None, 0.5, 0.01)     # half-width <= 0.01 * 6
    assert (n, idx.tolist()) == (0, [])
    # a ghost of 0 makes p = 0 exactly: with thr <= band a hit, whatever the logits; here only the ghosts hit
    ghost = np.ones(K, np.float32)
    ghosts = sorted({1 % K, K // 2, K - 1})
    ghost[ghosts] = 0
    big = np.stack([np.full(K, -4.0), np.full(K, 4.0)], 1).astype(np.float32)       # p ~ 0.9997 without the ghost
    idx, n = band_call(False, big, ghost, 0.02, 0.03)
    assert (n, idx.tolist()) == (len(ghosts), ghosts)
    idx, n = band_call(False, big, ghost, 0.03, 0.03)  # thr == band: |0 - thr| <= band holds with equality
    assert (n, idx.tolist()) == (len(ghosts), ghosts)
    idx, n = band_call(False, big, ghost, 0.04, 0.03)  # thr > band: the ghosts are out again
    assert (n, idx.tolist()) == (0, [])
