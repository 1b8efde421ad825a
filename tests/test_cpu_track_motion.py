"""Tracking::TrackWithMotionModel (src/Tracking.cpp:724-774): the sequential replay
lastproj_ref.run_track_motion_model on the frame pairs of tests/track_motion_cases.py shows every branch the
device driver is compared on (tests/test_gpu_track_motion.py), from the restatement and the oracle alone."""
import numpy as np
import pytest

import lastproj_ref as ref
import track_motion_cases as tc


@pytest.fixture(scope="module")
def replay():
    fs = tc.frames()
    return fs, {n: ref.run_track_motion_model(p, bool(ot)) for n, (p, ot, _) in fs.items()}


def test_replay_shows_every_branch(replay):
    fs, rp = replay
    for n, (p, ot, show) in fs.items():
        for k, v in show.items():
            assert rp[n][k] == v, (n, k, rp[n][k])
        assert p.frame.n <= 600
    # below 20 at th, enough at 2 * th
    assert rp["at_2th"]["nmatches_search"][0] < 20 <= rp["at_2th"]["nmatches_search"][1]
    # both searches below 20: no optimisation, the predicted pose stays
    f = rp["fails"]
    assert max(f["nmatches_search"]) < 20 and f["n_good"] == 0
    assert np.array_equal(f["Tcw"], np.asarray(fs["fails"][0].Tcw_cur, np.float32).ravel())
    s = rp["small"]      # the second search's matches stay in place
    assert 0 < s["nmatches"] < 20 and (s["out"] >= 0).sum() == s["nmatches"] and s["vo"] == 0
    # planted wrong matches are discarded, and nmatchesMap counts the kept slots with observations only
    o = rp["outliers"]
    assert (o["discarded"] >= 0).sum() >= 20 and o["nmatches_map"] < o["nmatches"] < o["nmatches_search"][0]
    assert np.isin(o["discarded"][o["discarded"] >= 0], fs["outliers"][0].wrong).mean() > 0.9
    assert not ((o["discarded"] >= 0) & (o["out"] >= 0)).any()
    # localization mode: few map matches, tracking goes on as visual odometry
    v = rp["only_tracking_vo"]
    assert v["vo"] == 1 and v["ok"] == 1 and v["nmatches_map"] < 10 and v["nmatches"] > 20
    assert rp["at_th"]["vo"] == 0 and rp["at_th"]["nmatches_map"] >= 10
