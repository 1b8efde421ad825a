"""bench.py's plain run and --dump-outputs (a small config-2 shape, in child processes as the driver
runs it): the result line carries the headline keys and nothing that belongs to --full, --steps sets
the number of timed steps, and the dumped arrays are float32, of the documented shapes, and
identical from run to run (seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, N, ITERS, STEPS = 8, 500, 300, 3
FULL_ONLY = ("roofline", "cpu_baseline", "sim3", "mlpnp", "events", "single_event_latency", "config1",
             "rccl_check", "poseopt", "search_by_bow", "search_by_sim3", "optimize_sim3", "kfdb_relocalization")


def _run(dump):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--candidates", str(C), "--corrs", str(N), "--iters", str(ITERS),
                        "--dump-outputs", dump], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(dump, f)) for f in sorted(os.listdir(dump))}


def test_plain_run_and_dump(tmp_path):
    line, a = _run(str(tmp_path / "a"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert not [k for k in FULL_ONLY if k in line]
    assert line["steps"] == STEPS and line["unit"] == "hypotheses/s" and line["higher_is_better"] is True
    # exhaustive mode: every candidate runs ITERS hypotheses in each of the STEPS timed steps
    # (ms_per_step is printed to 4 decimals: 5e-5 ms of a step that takes at least 0.02 ms)
    assert line["value"] == pytest.approx(C * ITERS / (line["ms_per_step"] * 1e-3), rel=5e-3)
    shapes = dict(ok=(C,), no_more=(C,), n_inliers=(C,), iterations=(C,), T=(C, 16),
                  hypothesis_inliers=(C, ITERS), hypothesis_poses=(C, ITERS, 12))
    assert {k: v.shape for k, v in a.items()} == shapes
    assert all(v.dtype == np.float32 for v in a.values())
    assert np.array_equal(a["iterations"], np.full(C, ITERS, np.float32))
    cnt = a["hypothesis_inliers"]
    assert cnt.min() >= 0 and 0 < cnt.max() <= N
    assert np.nanmax(np.abs(a["hypothesis_poses"])) > 0
    _, b = _run(str(tmp_path / "b"))
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
