"""The drivers' host bookkeeping (rsc_rounds.h: the event round-robin, the shared-stream events on it, the
PoseOptimization batch, the row gather) against the loops the driver entry points carried before they
shared it, on the host (tests/cpp/rounds_test.cpp, built by the Makefile).  Scripted iterate(5) calls: per
round the candidates iterated, every event and candidate record, the rand() position of every call and
every stream afterwards; a failing round gives its status back with every solver's own stream restored;
both fill forms of the batch for n in {0, 1, 3, 257} and four slot patterns, four problems per batch.
Once in the plain build and once in the build with the host address and undefined-behaviour sanitizers."""
import json
import os
import subprocess

import pytest

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb-slam2-optimized_amd", "lib")


@pytest.mark.parametrize("prog", ["rounds_test", "rounds_test_san"])
def test_rounds_match_former_driver_loops(prog):
    path = os.path.join(LIB, prog)
    assert os.path.exists(path), f"{path} not built: run make"
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mismatches"] == 0 and out["checks"] > 1000
    # 13 batches (no event, ten single events, all ten, a resolved next to an unresolved one) x
    # (plain, gated, gated with rejections, shared stream)
    assert out["runs"] == 52 and out["rounds"] > out["runs"]
    # every outcome class occurs, so a script set with a single path cannot pass
    for k in ("won_round0", "won_later", "exhausted", "empty"):
        assert out[k] >= 4, (k, out)
    # the failing round: every solver of the ten events had its own stream compared
    assert out["error_path_solvers"] == 21
    # four patterns x four sizes x two fill forms, one n == 0 problem per batch
    assert out["poseopt_problems"] == 32 and out["poseopt_n0"] == 8
