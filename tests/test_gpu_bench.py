"""GPU: `bench.py --steps K --dump-outputs DIR` end to end on the default configuration (extra legs off): one JSON line on stdout
whose `steps` and `ms_per_step` describe K timed steps, and the records of exactly those K steps in DIR."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_LEGS = ["--extra-configs", "", "--profile-steps", "0", "--cpu-steps", "0", "--many-chains", "0", "--root-sampler-leg", "0",
           "--dropin-leg", "0", "--parallel-cpu-budget", "0"]


@pytest.mark.gpu
def test_bench_steps_and_dump(tmp_path):
    steps, warmup = 37, 5
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out)] + NO_LEGS, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0
    rec, last = np.load(out / "records.npy"), np.load(out / "last_step.npy")
    assert rec.dtype == np.float64 and rec.shape == (steps, 14 + 51)  # femur-50 GPMM: rank 51
    assert np.all(np.diff(rec[:, 0]) == 1), "the records are not K consecutive steps"
    assert np.array_equal(last, rec[-1:]) and np.all(np.isfinite(rec))
    assert int(rec[:, 1].sum()) == line["config"]["accepted"]
