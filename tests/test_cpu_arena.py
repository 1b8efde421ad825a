"""The staging-arena cursor of the batched matchers (rsc_arena.h) against the offset arithmetic the six
entry points carried before they shared it, on the host (tests/cpp/arena_test.cpp, built by the
Makefile): every piece's offset, the upload and download marks and the total for count 1 and 3 with sizes
from {0, 1, 255, 256, 257}, two shapes against hand-computed numbers, alignment, sections and no overlap.
Once in the plain build and once in the build with the host address and undefined-behaviour sanitizers."""
import json
import os
import subprocess

import pytest

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb-slam2-optimized_amd", "lib")


@pytest.mark.parametrize("prog", ["arena_test", "arena_test_san"])
def test_arena_layouts_match_former_arithmetic(prog):
    path = os.path.join(LIB, prog)
    assert os.path.exists(path), f"{path} not built: run make"
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mismatches"] == 0
    # seven layouts (the local-map matcher in both forms) x eight shapes, two hand-computed ones
    assert out["layouts"] == 56 and out["literals"] == 2
    # every layout has at least table + one uploaded + one returned piece; the count-3 shapes have pieces
    # that start behind a problem's packed count words
    assert out["pieces"] >= 3 * out["layouts"]
    assert out["after_packed"] >= 2 * 6 * 3
