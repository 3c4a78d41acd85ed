"""bench.py --dump-outputs on the host (no GPU): benchlib.common.dump_outputs writes float32 / float64 .npy files,
cuts an output that is too large to a fixed seeded sample, and bench.py's command line knows --full and
--dump-outputs."""
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import REPO


def test_dump_outputs_dtypes_and_values(tmp_path):
    from benchlib.common import dump_outputs
    d = str(tmp_path / "out" / "nested")
    lg = torch.arange(12, dtype=torch.float32).reshape(6, 2) / 7
    arrays = {"logits": lg, "half": lg.to(torch.bfloat16), "idx": torch.tensor([3, 5, 2 ** 31 + 1], dtype=torch.int64),
              "f64": np.linspace(0, 1, 5), "i32": np.array([1, 2], dtype=np.int32), "empty": torch.empty((0,), dtype=torch.int32)}
    shapes = dump_outputs(d, arrays)
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in arrays)
    got = {k: np.load(os.path.join(d, k + ".npy")) for k in arrays}
    assert shapes == {k: list(v.shape) for k, v in got.items()}
    assert got["logits"].dtype == np.float32 and np.array_equal(got["logits"], lg.numpy())
    assert got["half"].dtype == np.float32 and np.array_equal(got["half"], lg.to(torch.bfloat16).float().numpy())
    assert got["idx"].dtype == np.float64 and got["idx"].tolist() == [3.0, 5.0, 2.0 ** 31 + 1]
    assert got["f64"].dtype == np.float64 and np.array_equal(got["f64"], np.linspace(0, 1, 5))
    assert got["i32"].dtype == np.float64 and got["empty"].shape == (0,)


def test_dump_outputs_samples_what_is_too_large(tmp_path, monkeypatch):
    """Over the limit an output is cut to the same sorted, seeded positions in every run; the files together stay
    under the limit and a small output beside it is written whole."""
    import benchlib.common as bc
    monkeypatch.setattr(bc, "DUMP_LIMIT_BYTES", 4096)
    big = np.arange(5000, dtype=np.float32).reshape(50, 100)
    small = np.arange(7, dtype=np.float32)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ra = bc.dump_outputs(a, {"big": big, "small": small})
    bc.dump_outputs(b, {"big": big + 1, "small": small})
    xa, xb = np.load(os.path.join(a, "big.npy")), np.load(os.path.join(b, "big.npy"))
    assert xa.ndim == 1 and 0 < xa.size < big.size and np.all(np.diff(xa) > 0)   # values = flat positions, sorted
    assert np.array_equal(xb, xa + 1)                                             # the same positions in both runs
    assert np.array_equal(np.load(os.path.join(a, "small.npy")), small)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 4096
    # the result says what was sampled, and the large output gets what the small one left, not half the budget
    assert ra == {"big": {"sample": xa.size, "of_shape": [50, 100]}, "small": [7]}
    assert xa.nbytes > 4096 // 2
    # unequal outputs that fit the limit together are all written whole
    monkeypatch.setattr(bc, "DUMP_LIMIT_BYTES", 21000)
    c = str(tmp_path / "c")
    assert bc.dump_outputs(c, {"big": big, "small": small}) == {"big": [50, 100], "small": [7]}
    assert np.array_equal(np.load(os.path.join(c, "big.npy")), big)


def test_bench_command_line_has_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
    # the CPU plumbing envelope computes nothing: asking for its outputs is an error, not an empty folder
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--plumbing", "--dump-outputs", "unused"],
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode != 0 and "no outputs for --dump-outputs" in r.stderr and not os.path.exists(
        os.path.join(REPO, "unused"))
