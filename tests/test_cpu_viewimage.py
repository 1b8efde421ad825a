"""The view-image builder of the resident views (rsc_viewimage.h) against the offset arithmetic the seven image
builders (six views and the vocabulary) carried before they shared it, on the host (tests/cpp/viewimage_test.cpp, built by the Makefile):
every piece's offset, the image's length, the bytes at every offset and at() on two bases, for n in
{0, 1, 7, 255, 256, 257, 8192} with the grid entries, FeatureVector nodes and levels varied on their own;
check_grid_csr on a valid grid and on every way a grid can be wrong; the radius guard at 2^30.
Once in the plain build and once in the build with the host address and undefined-behaviour sanitizers."""
import json
import os
import subprocess

import pytest

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb-slam2-optimized_amd", "lib")


@pytest.mark.parametrize("prog", ["viewimage_test", "viewimage_test_san"])
def test_view_images_match_former_arithmetic(prog):
    path = os.path.join(LIB, prog)
    assert os.path.exists(path), f"{path} not built: run make"
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mismatches"] == 0
    # seven sizes x (KeyFrame and Frame views: 16 shapes each, BoW: 12, MapPoints, LastFrame, triangulation and the
    # vocabulary: 1)
    assert out["cases"] == 7 * (2 * 16 + 12 + 4)
    assert out["pieces"] >= 4 * out["cases"]
    assert out["grid_checks"] == 6 and out["radius_checks"] == 3
