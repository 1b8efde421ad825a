"""The closed form of srand(seed)'s 31-word window (rsc_core.h rng_seed_word: the code the kernels of
the argument-path PnP round run, r[i] = r0 * 16807^i mod (2^31 - 1)) against RngStream's Schrage loop
on the host (tests/cpp/seed_window_test.cpp, built by the Makefile): seeds 0, 1, 2, 127773, 2^31 - 2,
2^31 - 1, 2^31, 2^31 + 1, 2^32 - 1 and 2^20 stratified seeds, all 31 words equal.  Same program:
RngStream::seed stores only the seed and the mark; the window read afterwards equals the eager one;
ensure() moving the window (0, 1, 5, 1,200 and 16,394 draws into the table, one draw past its reach)
clears the mark and leaves the eager stream's moved window, and the draws continue across the move.
Once in the plain build and once in the build with the host address and undefined-behaviour
sanitizers."""
import json
import os
import subprocess

import pytest

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb-slam2-optimized_amd", "lib")


@pytest.mark.parametrize("prog", ["seed_window_test", "seed_window_test_san"])
def test_closed_form_and_lazy_window(prog):
    path = os.path.join(LIB, prog)
    assert os.path.exists(path), f"{path} not built: run make"
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mismatches"] == 0
    assert out["edge_seeds"] == 9 and out["stratified_seeds"] == 1 << 20
    # 9 edge seeds x 5 positions at which ensure() has to move the window
    assert out["moved_windows"] == 45
    assert out["checks"] == 9 + (1 << 20) + 9 * (4 + 3 * 5 + 2)
