"""Frame::ComputeStereoMatches without a GPU: the sequential restatement (tests/stereo_ref.py) against the answers
worked out by hand (tests/stereo_cases.py) and against the golden fixture it wrote; what the random frames exercise;
the host build of the kernels' arithmetic in the kernels' decomposition (tests/stereo_emu) against the restatement,
bit for bit, on every case and every random frame; the key's row order; the limit; and the stand-alone emulation
program plain and under the host sanitizers."""
import json
import os
import subprocess

import numpy as np
import pytest

import stereo_cases as sc
import stereo_emu_lib as se
import stereo_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {name: (fr, exp) for name, fr, exp in sc.cases()}
ARRAYS = ("u_right", "depth", "best_right", "best_dist")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "stereo_traces.npz"))


@pytest.fixture(scope="module")
def randoms():
    """name -> (frame, the restatement's result), computed once."""
    return {name: (fr, sr.compute(fr)) for name, fr in sc.random_frames().items()}


def from_golden(golden, name):
    r = {k: golden[f"{name}/{k}"] for k in ARRAYS}
    rec = golden[f"{name}/result"]
    r.update(n_candidates=int(rec[0]), n_removed=int(rec[1]), median=int(rec[2]), th_dist=np.float32(rec[3]))
    return r


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_known_answer(name, golden):
    fr, exp = CASES[name]
    r = sr.compute(fr)
    assert sr.same(r, exp) == [], (r, exp)
    assert sr.same(r, from_golden(golden, name)) == []


def test_cases_cover_the_fixture(golden):
    assert sorted(str(s) for s in golden["names"]) == sorted(CASES)


def test_random_frames_match_the_fixture(randoms, golden):
    for name, (fr, r) in randoms.items():
        assert np.array_equal(sc.digest(fr), golden[f"{name}/digest"]), f"{name}: the generator drifted"
        assert sr.same(r, from_golden(golden, name)) == [], name


def test_random_frames_are_not_vacuous(randoms):
    """Every random frame of 64 or more left keypoints: at least 80 % accepted before the cut, between 1 and 50 %
    of those removed by it, at least one kept; the set holds a zero-disparity match and both kinds of tie."""
    total = dict(zero_disparity=0, tie_same_row=0, tie_other_row=0)
    seen = 0
    for name, (fr, r) in randoms.items():
        for k, v in sc.traits(fr, r).items():
            total[k] += v
        n = len(fr.kp)
        if n < 64:
            continue
        seen += 1
        assert r["n_candidates"] >= 0.8 * n, name
        assert 0.01 * r["n_candidates"] <= r["n_removed"] <= 0.5 * r["n_candidates"], name
        assert r["n_candidates"] - r["n_removed"] >= 1, name
        assert int((r["u_right"] != -1.0).sum()) == r["n_candidates"] - r["n_removed"], name
    assert seen >= 8
    assert all(v > 0 for v in total.values()), total


@pytest.mark.parametrize("mode", [0, 1])
def test_emulation_matches_the_restatement_on_the_cases(mode):
    for name, (fr, exp) in CASES.items():
        r = se.compute(fr, mode)
        assert sr.same(r, exp) == [], (name, mode, r)


@pytest.mark.parametrize("mode", [0, 1])
def test_emulation_matches_the_restatement_on_random_frames(mode, randoms):
    for name, (fr, want) in randoms.items():
        assert sr.same(se.compute(fr, mode), want) == [], (name, mode)


def test_key_row_order():
    """stm_order is monotonic in y and maps both zeros to one word."""
    L = se.lib()
    ys = np.array([-np.inf, -3.0e38, -480.0, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 479.99997, 480.0, 3.0e38, np.inf],
                  np.float32)
    w = [L.stme_order(float(y)) for y in ys]
    assert w[5] == w[6]
    w = w[:5] + w[6:]
    assert all(a < b for a, b in zip(w, w[1:])), w


def test_emulation_refuses_one_right_keypoint_too_many():
    m = 8193
    fr = sr.frame(np.zeros((1, 2)), [0], np.zeros((1, 32)), sc.scale_factors(), np.zeros((m, 2)), np.zeros(m),
                  np.zeros((m, 32)), 40.0, 0.5)
    assert se.compute(fr, 0) is None and se.compute(fr, 1) is None


@pytest.mark.parametrize("prog", [se.MAIN, se.MAIN_SAN])
def test_standalone_emulation_program(prog):
    """The stand-alone program (its own main, no Python): both modes agree on frames it draws; the second build
    runs under the host address / undefined-behaviour sanitizers."""
    se.lib()  # builds all three targets
    assert os.path.exists(prog), prog
    p = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["mismatches"] == 0 and out["refused"] == 2 and out["frames"] == 12
    assert out["accepted"] > 200 and 0 < out["removed"] < out["accepted"]
