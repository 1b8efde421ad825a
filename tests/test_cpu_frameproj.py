"""ORBmatcher::SearchByProjection(Frame&, KeyFrame, sAlreadyFound, th, ORBdist) (ORBmatcher.cpp:1317-1444) and
Tracking::Relocalization's refinement chain (Tracking.cpp:1294-1323) on the CPU:

* the sequential Python reference (tests/frameproj_ref.py) against answers worked out by hand, one case
  per rule (tests/frameproj_cases.py);
* the host build of the kernel's per-MapPoint functions (tests/frameproj_emu): its sequential loop
  equals the Python reference, and the fixed-point rounds the kernel runs equal the sequential loop;
* reloc_refine_ref on entry states crafted for each branch of the chain.
Everything is compared bit for bit."""
import os

import numpy as np
import pytest

import frameproj_cases as fc
import frameproj_emu_lib as fe
import frameproj_ref as fr
from rsc import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fc.cases()


def ref(p, trace=None):
    return fr.search_by_projection(p.frame, p.kf, p.Tcw, p.already, p.frame_mp, p.th, p.orb_dist,
                                   p.check_orientation, trace)


def emu_seq(p):
    return fe.search_sequential(p.frame, p.kf, p.Tcw, p.already, p.frame_mp, p.th, p.orb_dist, p.check_orientation)


def emu_fp(p):
    return fe.search_fixed_point(p.frame, p.kf, p.Tcw, p.already, p.frame_mp, p.th, p.orb_dist,
                                 p.check_orientation)


def check_emulation(p):
    """emulation sequential == Python reference; emulation fixed point == emulation sequential"""
    n, out = ref(p)
    n1, out1 = emu_seq(p)
    n2, out2, rounds = emu_fp(p)
    assert (n1, n2) == (n, n)
    assert np.array_equal(out1, out)
    assert np.array_equal(out2, out1)
    assert 1 <= rounds <= fr.n_eligible(p.kf, p.already) + 1
    return rounds


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_known_answer(name):
    p, exp = CASES[name]
    mp0, al0 = p.frame_mp.copy(), p.already.copy()
    n, out = ref(p)
    assert n == len(exp)
    assert np.array_equal(out, fc.expected_out(p, exp))
    assert np.array_equal(p.frame_mp, mp0) and np.array_equal(p.already, al0)


def test_rotation_case_differs_only_by_the_check():
    a, b = CASES["rotation_removed"][0], CASES["rotation_unchecked"][0]
    assert np.array_equal(a.kf.mp_pos, b.kf.mp_pos) and np.array_equal(a.frame.kp, b.frame.kp)
    assert ref(a)[0] == 11 and ref(b)[0] == 12


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulation_hand_built(name):
    check_emulation(CASES[name][0])


def test_domino():
    p, exp = fc.domino(70)
    n, out = ref(p)
    assert n == 70 and np.array_equal(out, fc.expected_out(p, exp))  # MapPoint k -> feature k
    rounds = check_emulation(p)
    assert rounds == 71  # one round per displacement, one to confirm
    assert rounds <= 71


def test_emulation_golden_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "frameproj_traces.npz"))
    names = [str(s) for s in z["names"]]
    assert "domino" in names and "random_coarse" in names and "random_fine" in names
    for name in names:
        p = fc.from_arrays(z, name)
        n, out = ref(p)
        assert n == int(z[f"{name}/nmatches"]) and np.array_equal(out, z[f"{name}/out"]), name
        check_emulation(p)


@pytest.mark.parametrize("seed,n_kf,n_frame,th,orb_dist", [(1, 300, 500, 10, 100), (2, 300, 500, 3, 64),
                                                           (3, 37, 50, 10, 100), (4, 600, 1500, 10, 100)])
def test_emulation_random_crowded(seed, n_kf, n_frame, th, orb_dist):
    p = fc.random_problem(seed, n_kf, n_frame, th, orb_dist, n_clusters=8 if n_kf > 100 else 2)
    tr = {}
    ref(p, tr)
    # the greedy path is exercised: MapPoints that ended on another feature than their unconstrained best
    assert int((tr["claim"] != tr["free_best"]).sum()) >= (10 if n_kf > 100 else 2)
    check_emulation(p)


def test_no_eligible_point():
    p = fc.random_problem(5, 60, 80, 10, 100, n_clusters=2)
    p.already = np.ones(p.kf.n, np.uint8)
    assert ref(p)[0] == 0
    assert check_emulation(p) == 1


# ---- the refinement chain -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_states():
    import reloc_refine_cases as rc
    return rc.chain_states()


@pytest.mark.parametrize("branch,pose_opts", [("stage1_short", 0), ("stage1_only", 1), ("both_stages", 2)])
def test_chain_branches(chain_states, branch, pose_opts):
    s = chain_states[branch]
    mp0 = s.frame_mp.copy()
    r = fr.reloc_refine_ref(s.frame, s.kf, dict(u_right=None, bf=0.0), s.frame_mp, s.found, s.n_good_in, s.Tcw_in)
    assert np.array_equal(s.frame_mp, mp0)
    assert r["pose_opts"] == pose_opts  # the branch this state is meant to cover
    if branch == "stage1_short":  # :1298 fails: no optimisation, the entry pose and count stay
        assert r["n_additional"][0] >= 0 and r["n_additional"][0] + s.n_good_in < 50 and r["n_additional"][1] == -1
        assert r["n_good"] == s.n_good_in and np.array_equal(r["Tcw"], s.Tcw_in)
        assert int((r["frame_mp"] >= 0).sum()) == int((mp0 >= 0).sum()) + r["n_additional"][0]
    elif branch == "stage1_only":  # :1304 fails: outliers of the optimisation stay in mvpMapPoints
        assert r["n_additional"][0] + s.n_good_in >= 50 and r["n_additional"][1] == -1
        assert not 30 < r["n_good"] < 50
        assert int((r["frame_mp"] >= 0).sum()) == int((mp0 >= 0).sum()) + r["n_additional"][0]
    else:  # :1313 holds: the second optimisation ran and its outliers were removed
        assert r["n_additional"][1] >= 0
        assert int((r["frame_mp"] >= 0).sum()) <= int((mp0 >= 0).sum()) + sum(r["n_additional"])
    keep = mp0 >= 0
    if pose_opts < 2:
        assert np.array_equal(r["frame_mp"][keep], mp0[keep])  # the search never replaces a set slot
