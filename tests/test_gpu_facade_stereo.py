"""rsc_orb::ComputeStereoMatches(F) and ComputeStereoMatches(F, view) (facade/Frame.hpp) through the C++ driver
tests/cpp/facade_stereo_test.cpp on a mock Frame: what both calls leave in mvuRight / mvDepth and their records
against the sequential restatement (tests/stereo_ref.py), bit for bit, and the kept view is usable by the local-map
matcher only after the call."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import stereo_cases as sc
import stereo_ref as sr
from rsc import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "orb-slam2-optimized_amd", "lib", "facade_stereo_test")


def pack(fr):
    b = [struct.pack("<i", len(fr.scale)), fr.scale.tobytes(), struct.pack("<3f", float(synth.LOG_SCALE_FACTOR),
                                                                         float(fr.mbf), float(fr.mb))]
    for kp, octave, desc in ((fr.kp, fr.octave, fr.desc), (fr.r_kp, fr.r_octave, fr.r_desc)):
        b += [struct.pack("<i", len(kp)), np.ascontiguousarray(kp, np.float32).tobytes(),
              np.ascontiguousarray(octave, np.int32).tobytes(), np.ascontiguousarray(desc, np.uint8).tobytes()]
    return b"".join(b)


def run(fr):
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(a, "wb") as f:
            f.write(pack(fr))
        subprocess.run([BIN, a, b], check=True, timeout=120)
        raw = open(b, "rb").read()
    status, n = struct.unpack_from("<2i", raw, 0)
    assert status == 0 and n == len(fr.kp), (status, n)
    recs = [struct.unpack_from("<3if", raw, 8 + 16 * k) for k in range(2)]
    arr = np.frombuffer(raw, np.float32, 4 * n, 40).reshape(4, n)
    return [dict(u_right=arr[2 * k], depth=arr[2 * k + 1], n_candidates=recs[k][0], n_removed=recs[k][1],
                 median=recs[k][2], th_dist=np.float32(recs[k][3])) for k in range(2)]


def check(fr):
    want = sr.compute(fr)
    for got in run(fr):
        assert np.array_equal(got["u_right"].view(np.uint32), want["u_right"].view(np.uint32))
        assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32))
        for k in ("n_candidates", "n_removed", "median"):
            assert got[k] == want[k], k
        assert got["th_dist"].view(np.uint32) == want["th_dist"].view(np.uint32)
    return want


def test_facade_on_a_random_frame():
    want = check(sc.random_frame(*sc.RANDOM_FRAMES["r_200x2049"]))
    assert want["n_candidates"] >= 160 and 0 < want["n_removed"] < want["n_candidates"]


def test_facade_on_hand_built_cases():
    cases = {name: fr for name, fr, _ in sc.cases()}
    for name in ("median_10_cuts_21_keeps_20", "zero_disparity_double_subtraction", "tie_across_signed_zero",
                 "empty_right", "empty_left"):
        check(cases[name])
