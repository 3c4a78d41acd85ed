"""CPU-only: the row order and the K-tile range of conv_igemm_p8's 3x3 tiles (csrc/p8_rowmap.h, CBW_P8_ROWSKIP) are
plain integer functions shared by the kernel and the host; tests/host/p8_rowmap_check.cpp brute-forces them over
N 1..9, Ho 1..5, Wo 1..7, tiles of 8 rows, G in {1, 2, 3, N, N + 5}, 3x3 pad 1 at strides 1 and 2: the row map is a
bijection of [0, M), no dropped kernel row is read by any row of its tile, and no range is empty."""
import os
import shutil
import subprocess

from conftest import REPO


def test_p8_rowmap_brute_force(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "p8_rowmap_check")
    src = os.path.join(REPO, "tests", "host", "p8_rowmap_check.cpp")
    inc = os.path.join(REPO, "enhance-cb-whisper_amd", "csrc")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-I", inc, src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
