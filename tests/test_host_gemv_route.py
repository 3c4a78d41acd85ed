"""CPU-only: which kernel a decode-step Linear runs on (csrc/gemv_route.h) is a pure host function of (rows, N, K,
LayerNorm prologue or not); tests/host/gemv_route_check.cpp checks that every route of every row count 1..16 at the
widths of synth.WHISPER_DECODERS is launchable, that the kernel family of a (K, LN) does not depend on the row count
(cbw_decoder_step_rows' bit-for-bit guarantee), and pins the routes of 1, 5, 10 and 15 rows field for field as the
launcher ran them before the dispatch moved into the header."""
import os
import shutil
import subprocess

from conftest import REPO

FLAGS = ["-std=c++17", "-O1", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_gemv_route(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gemv_route_check")
    src = os.path.join(REPO, "tests", "host", "gemv_route_check.cpp")
    inc = os.path.join(REPO, "enhance-cb-whisper_amd", "csrc")

    def build(extra):
        return subprocess.run([cxx, *FLAGS, *extra, "-I", inc, src, "-o", exe], capture_output=True, text=True, timeout=300)

    b = build(SANITIZE)
    if b.returncode != 0 and any(w in b.stderr.lower() for w in ("asan", "ubsan", "sanitize")):   # no runtime to link
        b = build([])
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    t = subprocess.run([exe, "--table"], capture_output=True, text=True, timeout=300)
    assert t.returncode == 0 and t.stdout.count("\n") > 15, (t.stdout + t.stderr)[-4000:]
    with open(os.path.join(REPO, "DESIGN.md")) as f:   # the table DESIGN.md quotes is this one
        design = f.read()
    stale = [line for line in t.stdout.splitlines() if line not in design]
    assert not stale, "DESIGN.md's GEMV route table differs from --table:\n" + "\n".join(stale)


def test_decoder_widths_are_the_checked_ones():
    """gemv_route_check.cpp restates synth.WHISPER_DECODERS' (vocab, d_model, ffn_dim): the table there is this one."""
    import re
    from cbw import synth
    src = open(os.path.join(REPO, "tests", "host", "gemv_route_check.cpp")).read()
    rows = {(n, int(v), int(d), int(f)) for n, v, d, f in re.findall(r'\{"([\w.\-]+)", (\d+), (\d+), (\d+)\}', src)}
    want = {(n, c[0], c[1], c[4]) for n, c in synth.WHISPER_DECODERS.items() if n != "large-v3-2l"}
    assert rows == want
    assert synth.WHISPER_DECODERS["large-v3-2l"][1::3] == synth.WHISPER_DECODERS["large-v3"][1::3]
