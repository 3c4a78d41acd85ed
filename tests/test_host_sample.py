"""CPU-only tests of what the device sampling path (cbw_sample_select, DecoderEngine.sample_windows) rests on:
torch.multinomial(p, 1, generator) is an exponential race -- it fills a tensor shaped like p with Exp(1) numbers q from
the generator and returns argmax(p / q) -- so a kernel given the same q draws the same token; a saved generator state
replays a draw; and the C ABI entry (header symbol, ctypes signature)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO


def _warped_probs(V, seed, T, top_k=50):
    """softmax of the temperature / top-k warped scores, as DecoderEngine.sample_search forms it ([1, V])"""
    g = torch.Generator().manual_seed(1000 + seed)
    scores = torch.randn((1, V), generator=g) * 4
    kth = torch.topk(scores, top_k, dim=-1).values[:, -1:]
    w = torch.where(scores >= kth, scores / T, torch.full_like(scores, float("-inf")))
    return torch.softmax(w, -1)


@pytest.mark.parametrize("V", [51865, 51866])
@pytest.mark.parametrize("T", [0.2, 1.0])
def test_multinomial_is_the_exponential_race_over_one_draw_of_v_numbers(V, T):
    for seed in range(5):
        p = _warped_probs(V, seed, T)
        g1, g2 = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        tok = int(torch.multinomial(p, 1, generator=g1)[0, 0])
        q = torch.empty(V).exponential_(1, generator=g2)   # a [V] row draws what the [1, V] tensor draws
        assert tok == int(torch.argmax(p[0] / q)), (V, T, seed)
        assert p[0, tok] > 0
        assert torch.equal(g1.get_state(), g2.get_state()), "multinomial consumed something else than one [V] draw"
        assert torch.equal(torch.rand(3, generator=g1), torch.rand(3, generator=g2))


@pytest.mark.parametrize("V", [51865, 51866])
def test_a_saved_generator_state_replays_the_draw(V):
    g = torch.Generator().manual_seed(7)
    torch.empty(V).exponential_(generator=g)
    state = g.get_state()
    first = torch.empty(V).exponential_(generator=g)
    torch.empty(V).exponential_(generator=g)   # draws past the point of interest
    torch.empty(V).exponential_(generator=g)
    g.set_state(state)
    assert torch.equal(torch.empty(V).exponential_(generator=g), first)
    # and multinomial after a restore draws from the same numbers
    p = _warped_probs(V, 3, 1.0)
    g.set_state(state)
    assert int(torch.multinomial(p, 1, generator=g)[0, 0]) == int(torch.argmax(p[0] / first))


def test_header_symbol_and_ctypes_signature():
    from cbw import _lib
    src = open(os.path.join(REPO, "include", "cbw.h")).read()

    def params(name):
        m = re.search(r"^int\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.M | re.S)
        assert m, f"include/cbw.h does not declare {name}"
        return [" ".join(p.split()) for p in m.group(1).split(",")]
    greedy, sample = params("cbw_greedy_select"), params("cbw_sample_select")
    # cbw_greedy_select's signature plus four arguments before the stream
    assert sample == greedy[:-1] + ["float temperature", "int top_k", "const float* noise", "int64_t noise_ld",
                                    "cbw_stream_t stream"]
    kinds = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64}
    want = [kinds.get(p.split()[0], ctypes.c_void_p) if "*" not in p and not p.startswith("cbw_stream_t")
            else ctypes.c_void_p for p in sample]
    res, args = _lib.SIGNATURES["cbw_sample_select"]
    assert res is ctypes.c_int and list(args) == want
    lib = _lib.load()
    assert hasattr(lib, "cbw_sample_select")
    # the entry checks its arguments before any launch (no GPU needed to be refused)
    assert lib.cbw_sample_select(None, 1, 8, 8, None, None, -1, -1, 0, -1, None, None, None, None, None, None, 1.0, 50,
                                 None, 8, None) == -1
    assert "pba_whisper.py:318-331" in src[src.index("One sampling step"):src.index("int cbw_sample_select")]
