"""ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cpp:671-821), the matcher of LocalMapping::SearchInNeighbors,
on the CPU:

* the sequential Python restatement (tests/fusekf_ref.py) against answers worked out by hand, one case per rule
  (tests/fusekf_cases.py);
* the host build of the kernel's per-pair function (tests/fusekf_emu), one lane per pair and the 16-lane window
  walk, against the restatement on every case and against the golden fixture on the random crowded problems;
* the fixture recomputed (one pose by the restatement, all of them by the emulation), with the conditions that
  keep it from being vacuous;
* the restatement's map model on the bookkeeping of :797-817;
* the stand-alone program of the emulation, plain and under the host address / undefined-behaviour sanitizers.
Everything is compared bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

import fusekf_cases as fc
import fusekf_emu_lib as fe
import fusekf_ref as fr
from rsc import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fc.cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "fusekf_traces.npz"))


@pytest.fixture(scope="module")
def randoms():
    return {name: fc.random_problem(seed) for name, seed in fc.RANDOM_SEEDS.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_known_answer(name, golden):
    p, exp = CASES[name]
    skip0 = p.skip.copy()
    best = fr.fuse_kf(p.kf, p.pts, p.skip, p.th)
    assert best.tolist() == exp
    assert np.array_equal(best, golden[f"{name}/best_idx"]) and np.array_equal(p.skip, skip0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulation_hand_built(name):
    p, exp = CASES[name]
    for lanes in (0, 16, 1, 5):
        n, best = fe.fuse(p.kf, p.pts, p.skip, p.th, lanes)
        assert best.tolist() == exp, lanes
        assert n == sum(b >= 0 for b in exp)


def test_cases_cover_the_fixture(golden):
    assert sorted(str(s) for s in golden["names"]) == sorted(CASES)


def test_z_zero_is_skipped_before_the_cell_arithmetic():
    """z = +-0: the projection is inf or NaN, IsInImage rejects it, and project() returns before features_in_area
    (which asserts finite inputs) could see it; z = -0 is not `< 0`, so it gets that far."""
    p, _ = CASES["z_sign"]
    z = np.float32(-0.0) * np.float32(1.0) + np.asarray(p.kf.tcw, np.float32)[2]
    assert z == 0 and np.signbit(z)  # the camera z of point 4
    for i, test in ((2, np.isposinf), (3, np.isnan), (4, np.isposinf)):  # point 4: x * invz = -1 * -inf
        info = {}
        assert fr.project(p.kf, p.pts, i, p.th, info) is None
        assert test(info["u"]) and not fr.kr.is_in_image(p.kf, info["u"], info["v"])
    for i in (0, 1):  # z < 0 returns before the projection
        info = {}
        assert fr.project(p.kf, p.pts, i, p.th, info) is None and not info


def test_large_window_and_stride():
    """The tie cases walk a window of 80 features, more than one wave's worth and five trips of a 16-lane stride."""
    p, _ = CASES["tie_stride"]
    st = {}
    fr.fuse_kf(p.kf, p.pts, p.skip, p.th, st)
    assert st["largest"] == 80 > 64


def test_inv_sigma2_derivation():
    """1.0f / (sf * sf) in float, as the gate derives it, equals the restatement's and differs from a double
    evaluation rounded once on at least one level (so the order of the roundings is pinned)."""
    sf = synth.scale_factors()
    a, b = fe.inv_sigma2(sf), fr.inv_level_sigma2(sf)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    once = (1.0 / (sf.astype(np.float64) ** 2)).astype(np.float32)
    assert (a != once).any()


@pytest.mark.parametrize("name", sorted(fc.RANDOM_SEEDS))
def test_random_crowded(golden, randoms, name):
    pts, kfs, skips = randoms[name]
    assert np.array_equal(pts.pos, golden[f"{name}/pt_pos"])  # the generator reproduces the fixture's inputs
    assert kfs[0].n == 600 and pts.n == 1500 and 0.2 < float((kfs[0].u_right >= 0).mean()) < 0.4
    for k, (kf, skip) in enumerate(zip(kfs, skips)):
        gold = golden[f"{name}/{k}/best_idx"]
        level, stereo, mono, windows, largest = (int(v) for v in golden[f"{name}/{k}/stats"])
        assert int((gold >= 0).sum()) >= 100 and level >= 1 and stereo >= 1 and mono >= 1
        for lanes in (0, 16):
            n, best = fe.fuse(kf, pts, skip, fc.TH, lanes)
            assert np.array_equal(best, gold), (k, lanes)
            assert n == int((gold >= 0).sum())
    # the restatement itself, on the points of one pose that have a match or are among the first 200
    k = 1
    gold = golden[f"{name}/{k}/best_idx"]
    sel = np.nonzero((gold >= 0) | (np.arange(pts.n) < 200))[0][:400]
    sub = fr.kr.points_of(state=pts.state[sel], pos=pts.pos[sel], normal=pts.normal[sel], dmax=pts.dmax[sel],
                          dmin=pts.dmin[sel], desc=pts.desc[sel])
    st = {}
    assert np.array_equal(fr.fuse_kf(kfs[k], sub, skips[k][sel], fc.TH, st), gold[sel])
    assert st["level"] >= 1 and st["stereo"] >= 1 and st["mono"] >= 1


def test_poses_differ(golden):
    """The three target poses give three different answers (so a kernel that read one pose for all would fail)."""
    for name in fc.RANDOM_SEEDS:
        b = [golden[f"{name}/{k}/best_idx"] for k in range(3)]
        assert not np.array_equal(b[0], b[1]) and not np.array_equal(b[1], b[2])


# ---- the map model -------------------------------------------------------------------------------------------
def _model(n_kf_slots=4):
    p, _ = CASES["no_claims"]  # two points, both nearest to keypoint 0 (distance 2); keypoint 1 at distance 30
    kf = fr.KeyFrame(7, p.kf)
    mk = lambda pid, i: fr.MapPoint(pid, p.pts.pos[i], p.pts.normal[i], p.pts.dmax[i], p.pts.dmin[i], p.pts.desc[i])
    return p, kf, mk


def test_model_fill_then_claim():
    """:811-815 then :801-809 within one call: point A fills the empty slot, point B finds A there; with equal
    Observations() the else branch runs: pMPinKF->Replace(pMP), so B survives in the slot and A turns bad."""
    p, kf, mk = _model()
    other = fr.KeyFrame(8, p.kf)
    a, b = mk(0, 0), mk(1, 1)
    b.add_observation(other, 1)  # one observation, as A has once it sits in the slot: a tie
    other.slots[1] = b
    assert fr.fuse(kf, [a, None, b, a], p.th) == 2  # the null is skipped, the repeated A is bad by then
    assert kf.slots[0] is b and a.bad and a.replaced is b and not b.bad
    assert sorted(b.obs) == [7, 8] and b.obs[7][1] == 0 and b.nobs == 2 and a.obs == {}
    assert b.desc.tolist() == fc.desc_bits(2).tolist()  # ComputeDistinctiveDescriptors ran on the survivor


def test_model_more_observations_wins():
    p, kf, mk = _model()
    other = fr.KeyFrame(8, p.kf)
    a, b = mk(0, 0), mk(1, 1)
    a.add_observation(other, 1)
    other.slots[1] = a
    assert fr.fuse(kf, [a, b], p.th) == 2
    assert kf.slots[0] is a and b.bad and b.replaced is a and a.nobs == 2  # B->Replace(A): A has 2 > 0


def test_model_bad_occupant_counts():
    p, kf, mk = _model()
    occ, a = mk(5, 0), mk(0, 0)
    occ.bad = True
    kf.slots[0] = occ
    assert fr.fuse(kf, [a], p.th) == 1  # :816 counts although nothing happened
    assert kf.slots[0] is occ and a.obs == {} and not a.bad


@pytest.mark.parametrize("prog", ["fusekf_emu_main", "fusekf_emu_main_san"])
def test_standalone_program(prog):
    fe.lib()  # builds the directory
    path = os.path.join(fe.DIR, "build", prog)
    assert os.path.exists(path), path
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mismatches"] == 0 and out["nfused"] >= 100
