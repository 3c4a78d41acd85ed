"""CPU-only: the pairs form of the two re-scoring tiers is part of the C ABI -- declared in include/cbw.h, exported
by libcbw.so and present in the ctypes table with the declared argument count (no compute calls: no GPU here)."""
import os
import re

import pytest

from conftest import REPO

NEW = ["cbw_kws_rescore_pairs", "cbw_kws_rescore_x3_pairs"]


def declaration(name):
    src = open(os.path.join(REPO, "include", "cbw.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.M | re.S)
    assert m, f"include/cbw.h does not declare {name}"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NEW)
def test_pairs_rescoring_symbols_exported_and_declared(name):
    from cbw import _lib
    args = declaration(name)
    # the per-utterance call's arguments plus B, the two index arrays and P
    assert len(args) == len(declaration(name[:-len("_pairs")])) + 4
    assert [a.split()[-1].lstrip("*") for a in args[:4]] == ["h", "utt", "utt_mask", "B"]
    assert "pair_utt" in args[9] and "pair_kwd" in args[10] and args[11] == "int P"
    lib = _lib.load()
    assert hasattr(lib, name), f"libcbw.so does not export {name}"
    restype, argtypes = _lib.SIGNATURES[name]
    assert len(argtypes) == len(args)
    # a null handle is refused before anything else is read
    assert getattr(lib, name)(*([None] + [0 if "int" in a and "*" not in a else None for a in args[1:]])) == -1
    assert lib.cbw_last_error()
