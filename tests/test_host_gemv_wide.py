"""CPU-only: the dispatch of a decode-step Linear over 1..80 rows (gemv_wide_route, csrc/gemv_route.h) as a pure host
function; tests/host/gemv_wide_check.cpp checks that every M = 1..80 at every (K, LayerNorm) of DESIGN.md's table runs
as ceil(M / 16) row groups on the 16-slot kernel of the family gemv_route gives that (K, LayerNorm), within the raised
LDS limit, that M = 0 and M = 81 have no route, and that gemv_route still ends at 16 rows."""
import os
import shutil
import subprocess

from conftest import REPO

FLAGS = ["-std=c++17", "-O1", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_gemv_wide_route(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gemv_wide_check")
    src = os.path.join(REPO, "tests", "host", "gemv_wide_check.cpp")
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
    assert not stale, "DESIGN.md's wide GEMV route table differs from --table:\n" + "\n".join(stale)
