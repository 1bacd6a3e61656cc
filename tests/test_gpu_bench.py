"""GPU: bench.py's plain run and --dump-outputs.  A plain run prints the headline line alone (no side legs); --dump-outputs
writes the last timed step's embeddings, and two runs with the same arguments write the same bits (seeded inputs and
weights), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a small network and batch: the same code path as the headline, a fraction of its set-up time
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--model", "r18", "--batch", "96", "--chunk", "64"]


def _run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(out_dir)],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-800:]
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(gpu, tmp_path):
    a = _run(tmp_path / "a")
    assert a["steps"] == 3 and a["warmup"] == 1 and a["unit"] == "embeddings/s" and a["higher_is_better"] is True
    assert a["dtype"] == "bf16" and a["ms_per_step"] > 0
    assert abs(a["value"] - 96 / (a["ms_per_step"] / 1e3)) < 1e-6 * a["value"]
    for k in ("roofline", "cpu_baseline", "exact_selection", "config3", "config4", "config5", "parity"):
        assert k not in a, k
    e = np.load(tmp_path / "a" / "embeddings.npy")
    assert e.dtype == np.float32 and e.shape == (96, 512) and np.isfinite(e).all()
    assert np.abs(np.linalg.norm(e.astype(np.float64), axis=1) - 1.0).max() < 1e-5
    _run(tmp_path / "b")
    assert np.array_equal(e, np.load(tmp_path / "b" / "embeddings.npy")), "the same arguments gave different outputs"
