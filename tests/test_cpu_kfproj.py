"""The loop-closing matchers ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
(ORBmatcher.cpp:241-352) and ORBmatcher::Fuse (:823-946), and the Sim3 composition of
LoopClosing.cpp:318-320, on the CPU:

* the sequential Python restatement (tests/kfproj_ref.py) against answers worked out by hand, one case per
  rule (tests/kfproj_cases.py);
* the host build of the kernels' per-point functions (tests/kfproj_emu): its sequential loop equals the
  restatement, and the fixed-point rounds the kernel runs equal the sequential loop, on the cases, the domino
  and the random crowded problems of the golden fixture;
* the stand-alone program of the emulation, plain and under the host address / undefined-behaviour
  sanitizers;
* the host build of rsc_sim3compose.h against the float64 restatement over 1,000 random Sim3 pairs and one
  pair per matrix-to-quaternion branch.
Everything is compared bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

import kfproj_cases as kc
import kfproj_emu_lib as ke
import kfproj_ref as kr
from rsc import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = kc.cases()
FUSE_CASES = kc.fuse_cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "kfproj_traces.npz"))


def ref(p, trace=None):
    return kr.search_by_projection_kf(p.kf, p.pts, p.Scw, p.already, p.occupied, p.th, trace)


def check_emulation(p, n, out):
    """emulation sequential == restatement; emulation fixed point == emulation sequential"""
    n1, out1 = ke.search_sequential(p.kf, p.pts, p.Scw, p.already, p.occupied, p.th)
    n2, out2, rounds, walks = ke.search_fixed_point(p.kf, p.pts, p.Scw, p.already, p.occupied, p.th)
    assert (n1, n2) == (n, n)
    assert np.array_equal(out1, out)
    assert np.array_equal(out2, out1)
    assert 1 <= rounds <= kr.n_eligible(p.pts, p.already) + 1
    return rounds, walks


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_known_answer(name):
    p, exp = CASES[name]
    oc0, al0 = p.occupied.copy(), p.already.copy()
    n, out = ref(p)
    assert n == len(exp)
    assert np.array_equal(out, kc.expected_out(p, exp))
    assert np.array_equal(p.occupied, oc0) and np.array_equal(p.already, al0)


def test_z_zero_is_skipped_before_the_cell_arithmetic():
    """invz = inf: u is inf for x != 0 and NaN for x == 0; IsInImage rejects both, so project() returns before
    features_in_area (which asserts finite inputs) could see them."""
    p, _ = CASES["z_zero"]
    R, t, Ow = kr.decompose(p.Scw, False)
    for i, test in ((0, np.isinf), (1, np.isnan)):
        info = {}
        assert kr.project(p.kf, p.pts, R, t, Ow, i, p.th, False, info) is None
        assert test(info["u"])
        assert not kr.is_in_image(p.kf, info["u"], info["v"])


def test_edge_cases_differ_only_in_one_float():
    for a, b, field in (("dist_min_edge", "dist_min_below", "dmin"), ("dist_max_edge", "dist_max_above", "dmax"),
                        ("angle_edge", "angle_below", "normal")):
        pa, pb = CASES[a][0], CASES[b][0]
        va, vb = getattr(pa.pts, field).ravel(), getattr(pb.pts, field).ravel()
        k = np.nonzero(va != vb)[0]
        assert len(k) == 1 and abs(int(va.view(np.int32)[k[0]]) - int(vb.view(np.int32)[k[0]])) == 1  # one ulp
        assert ref(pa)[0] == 1 and ref(pb)[0] == 0


def test_level_above_is_what_the_frame_matcher_accepts():
    """The octave L + 1 keypoint of `level_above` carries the best descriptor: a [L-1, L+1] window would take it."""
    p, exp = CASES["level_above"]
    assert p.kf.octave[0] == 4 and exp == {1: 0}


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulation_hand_built(name):
    p, exp = CASES[name]
    check_emulation(p, len(exp), kc.expected_out(p, exp))


@pytest.mark.parametrize("name", sorted(FUSE_CASES))
def test_fuse_known_answer(name):
    p, exp = FUSE_CASES[name]
    r = kr.fuse(p.kf, p.pts, p.Scw, p.in_kf, float(p.th))
    for k in ("best_idx", "replace", "added"):
        assert r[k].tolist() == exp[k], k
    assert r["nfused"] == sum(b >= 0 for b in exp["best_idx"])
    n, best = ke.fuse(p.kf, p.pts, p.Scw, p.in_kf, float(p.th))
    assert n == r["nfused"] and np.array_equal(best, r["best_idx"])


def test_fuse_scale_is_divided_out():
    """The same Scw with the scale left in (as SearchByProjection would read it) rejects the point."""
    p, _ = FUSE_CASES["scale_two"]
    assert ref(p)[0] == 0


def test_domino(golden):
    p, exp = kc.domino(40)
    n, out = ref(p)
    assert n == 40 and np.array_equal(out, kc.expected_out(p, exp))  # point k -> keypoint k
    rounds, _ = check_emulation(p, n, out)
    assert rounds == 41 == int(golden["domino/rounds"][0])  # one round per displacement, one to confirm
    claim, r2, _ = kr.fixed_point_rounds(p.kf, p.pts, p.Scw, p.already, p.occupied, p.th)
    assert r2 == 41 and np.array_equal(claim, np.arange(40))
    round1 = golden["domino/round1"]
    assert np.array_equal(round1, np.maximum(np.arange(40) - 1, 0))  # every point first goes for its left neighbour's


def test_golden_fixture(golden):
    names = [str(s) for s in golden["names"]]
    assert "domino" in names and "random_a" in names and "random_b" in names
    for name in names:
        p = kc.from_arrays(golden, name)
        n, out = int(golden[f"{name}/nmatches"][0]), golden[f"{name}/out"]
        if not name.startswith("random"):  # the random ones are restated once, in the test below
            assert ref(p)[0] == n and np.array_equal(ref(p)[1], out), name
        rounds, walks = check_emulation(p, n, out)
        assert rounds == int(golden[f"{name}/rounds"][0]), name
        if name.startswith("random"):
            assert n >= 100 and walks >= 1, (name, n, walks)
            assert int((golden[f"{name}/round1"][out[out >= 0]] != np.nonzero(out >= 0)[0]).sum()) >= 10


@pytest.mark.parametrize("name", sorted(kc.RANDOM_SEEDS))
def test_random_crowded_restatement(golden, name):
    """The generator reproduces the fixture's inputs, and the restatement its outputs."""
    p = kc.random_problem(kc.RANDOM_SEEDS[name])
    q = kc.from_arrays(golden, name)
    assert np.array_equal(p.pts.pos, q.pts.pos) and np.array_equal(p.kf.kp, q.kf.kp)
    assert p.kf.n == 600 and p.pts.n == 1500
    tr = {}
    n, out = ref(q, tr)
    assert n == int(golden[f"{name}/nmatches"][0]) and np.array_equal(out, golden[f"{name}/out"])
    assert np.array_equal(tr["free_best"], golden[f"{name}/round1"])
    assert int((tr["claim"] != tr["free_best"]).sum()) >= 10


def test_fuse_batch(golden):
    p = kc.from_arrays(golden, "random_a")
    th = float(golden["fuse/th"][0])
    for k in range(len(golden["fuse/Scw"])):
        kf = kc.make_kf(p.kf.kp, p.kf.octave, p.kf.desc, golden["fuse/mp_state"][k])
        S, ik = golden["fuse/Scw"][k], golden["fuse/in_kf"][k]
        n, best = ke.fuse(kf, p.pts, S, ik, th)
        assert n == int(golden["fuse/nfused"][k]) >= 100 and np.array_equal(best, golden["fuse/best_idx"][k])
        if k == 1:  # the restatement itself, once
            r = kr.fuse(kf, p.pts, S, ik, th)
            assert np.array_equal(r["best_idx"], best) and np.array_equal(r["replace"], golden["fuse/replace"][k])
            assert np.array_equal(r["added"], golden["fuse/added"][k])
            assert np.array_equal(r["holder"], golden["fuse/holder"][k]) and (r["holder"] >= 0).any()


def test_no_eligible_point():
    p = kc.random_problem(3, 100, 200, n_clusters=4)
    p.already = np.ones(p.pts.n, np.uint8)
    n, out = ref(p)
    assert n == 0
    assert check_emulation(p, n, out)[0] == 1


@pytest.mark.parametrize("prog", ["kfproj_emu_main", "kfproj_emu_main_san"])
def test_standalone_program(prog):
    ke.lib()  # builds the directory
    path = os.path.join(ke.DIR, "build", prog)
    assert os.path.exists(path), path
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mismatches"] == 0
    assert out["nmatches"] >= 100 and out["rounds"] >= 3 and out["fallback_walks"] >= 1 and out["nfused"] >= 100


# ---- LoopClosing.cpp:318-320 ----------------------------------------------------------------------------
def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _branch(R):
    R = np.asarray(R, np.float32).astype(np.float64)
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return "trace"
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    return "xyz"[i]


def test_compose_bit_for_bit():
    rng = np.random.default_rng(77)
    Rs = [_rot([1, 2, 3], 0.4), _rot([1, 0.1, 0.1], 3.0), _rot([0.1, 1, 0.1], 3.0), _rot([0.1, 0.1, 1], 3.0)]
    assert [_branch(R) for R in Rs] == ["trace", "x", "y", "z"]  # one pair per matrix-to-quaternion branch
    Rs += [synth.random_rotation(rng, np.pi) for _ in range(1000)]
    seen = {_branch(R) for R in Rs[4:]}
    assert "trace" in seen and len(seen) >= 2
    n = len(Rs)
    S_cm = np.zeros((n, 8))
    q = rng.normal(0, 1, (n, 4))
    S_cm[:, :4] = q / np.linalg.norm(q, axis=1, keepdims=True) * (1 + rng.normal(0, 1e-9, (n, 1)))  # g2o never renormalises
    S_cm[:, 4:7] = rng.normal(0, 2, (n, 3))
    S_cm[:, 7] = rng.uniform(0.5, 2.0, n)
    R_mw = np.array(Rs).astype(np.float32)
    t_mw = rng.normal(0, 2, (n, 3)).astype(np.float32)
    S_cw, T = ke.compose(S_cm, R_mw, t_mw)
    for k in range(n):
        s_ref, T_ref = kr.compose(S_cm[k], R_mw[k], t_mw[k])
        assert np.array_equal(S_cw[k].view(np.uint64), s_ref.view(np.uint64)), k
        assert np.array_equal(T[k].view(np.uint32), T_ref.view(np.uint32)), k
    # toIso keeps the unit rotation and the unscaled translation: the scale appears nowhere in mScw
    k = 5
    Rk = T[k].reshape(4, 4)[:3, :3].astype(np.float64)
    assert abs(np.linalg.det(Rk) - 1.0) < 1e-5 and S_cw[k, 7] == S_cm[k, 7]
    assert np.array_equal(T[k].reshape(4, 4)[:3, 3], S_cw[k, 4:7].astype(np.float32))
