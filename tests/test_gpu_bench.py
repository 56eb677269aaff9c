"""bench.py's plain run on the GPU: the contract line without the side measurements of `--full`, and `--dump-outputs`
reproducible bit for bit from run to run (the synthetic pair is rendered with deterministic reductions).  Small workload;
the numbers mean nothing."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--size", "1024", "--pois", "64", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_is_lean_and_its_outputs_reproduce(tmp_path):
    a = _plain_run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in a, k
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0 and a["value"] > 0
    for k in ("cpu_baseline", "oht_pair", "pcie_inclusive", "arith_fma", "paths_8f_row1", "roofline_secondary", "multi_gpu_check"):
        assert k not in a, k
    got = np.load(tmp_path / "a" / "pois.npy")
    assert got.dtype == np.float32 and got.shape == (64 * 64, 25)
    assert int((got[:, 16] >= 0).sum()) == a["config"]["converged_pois"] >= 0.99 * 64 * 64
    _plain_run(tmp_path / "b")
    again = np.load(tmp_path / "b" / "pois.npy")
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
