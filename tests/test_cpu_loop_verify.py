"""The synthetic loop event of tests/loop_verify_cases.py on the CPU: the oracle's gate accepts it with fewer
than 39 matched slots, and the restatement of LoopClosing.cpp:318-320, :360-370 ends on exactly 39 matches
(rejected), exactly 40 (accepted) and more for the three MapPoint lists the GPU test runs."""
import numpy as np

import kfproj_ref as kr
import loop_verify_cases as lv


def test_event_and_lists():
    b = lv.build()
    occupied = int((b.gate["matches"] != -1).sum())
    assert occupied < 39
    totals = [x[2]["n_total"] for x in b.lists]
    assert totals[:2] == [39, 40] and totals[2] > 40
    assert [x[2]["accepted"] for x in b.lists] == [0, 1, 1]
    for p, a, exp in b.lists:
        assert exp["n_total"] == occupied + exp["n_projected"] == occupied + int((exp["projected"] >= 0).sum())
        assert not (exp["projected"][b.gate["matches"] != -1] >= 0).any()  # an occupied slot is never rewritten
    # the lists are prefixes of one another: the shorter result is the longer one restricted to its points
    short, full = b.lists[0][2]["projected"], b.lists[2][2]["projected"]
    n0 = b.lists[0][0].n
    assert np.array_equal(short, np.where(full < n0, full, -1))
    assert a.sum() > 0  # some of the matched KeyFrame's points are already in mvpCurrentMatchedPoints
    # mScw: unit rotation, translation of the composed Sim3
    T = b.lists[0][2]["Scw"].reshape(4, 4)
    assert abs(np.linalg.det(T[:3, :3].astype(np.float64)) - 1.0) < 1e-5
    assert np.array_equal(T[:3, 3], b.lists[0][2]["Scw_sim3"][4:7].astype(np.float32))
    assert kr.n_eligible(b.lists[2][0], b.lists[2][1]) > 0
