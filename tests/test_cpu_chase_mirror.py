"""tridiag_qr<double, 12> (rsc_core.h) with a rotation sink that opts into the mirror() / any_lane()
hooks — the chase wave of the split eigen stage — against a sink without them, on the host
(tests/cpp/chase_mirror_test.cpp, built by the Makefile): diag, sub, perm, the return value and every
(k, c, s, apply) call bit for bit.  The program draws its own inputs; this test checks that every
input class ran and that nothing differed, once in the plain build and once in the build with the
host address and undefined-behaviour sanitizers."""
import json
import os
import subprocess

import pytest

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb-slam2-optimized_amd", "lib")
MINIMUM = {"random": 10000, "mid_zero": 1000, "multi_zero": 1000, "converged": 100, "nan_block": 100,
           "nan_above_finite": 100, "nan_middle": 100}


@pytest.mark.parametrize("prog", ["chase_mirror_test", "chase_mirror_test_san"])
def test_hooked_chase_bit_identical(prog):
    path = os.path.join(LIB, prog)
    assert os.path.exists(path), f"{path} not built: run make"
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mismatches"] == 0
    for k, n in MINIMUM.items():
        assert out[k] >= n, (k, out[k])
    # the hooked sinks ran (three mirror forms per matrix), rotations were compared, and the NaN
    # classes ended without convergence (the Q4 exit)
    assert out["mirror_runs"] == 3 * sum(out[k] for k in MINIMUM)
    assert out["rotations"] > 100 * out["random"]
    assert out["not_converged"] >= out["nan_block"] + out["nan_above_finite"] + out["nan_middle"]
