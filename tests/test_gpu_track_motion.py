"""Tracking::TrackWithMotionModel on the device (rsc_track_motion_model_many: the last-frame matcher at th, the
retry at 2 * th, PoseOptimization, the outlier discard) against the sequential replay
lastproj_ref.run_track_motion_model (the restatement of the matcher and the oracle's PoseOptimization), bit for
bit, pose included.  All frames of tests/track_motion_cases.py run in one call."""
import numpy as np
import pytest

import lastproj_ref as ref
import track_motion_cases as tc
from gpu_common import ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def replay():
    fs = tc.frames()
    return fs, {n: ref.run_track_motion_model(p, bool(ot)) for n, (p, ot, _) in fs.items()}


@pytest.fixture(scope="module")
def device(replay):
    from rsc import engine
    fs, _ = replay
    ps = [p for p, _, _ in fs.values()]
    fvs = [engine.FrameView(ctx(), p.frame) for p in ps]
    for v, p in zip(fvs, ps):
        v.set_stereo(p.frame.u_right, p.frame.mbf)
    lvs = [engine.LastFrameView(ctx(), p.last) for p in ps]
    res, out, disc = engine.track_motion_model_many(ctx(), fvs, lvs, [p.Tcw_cur for p in ps],
                                                    [p.Tcw_last for p in ps], [p.mb for p in ps], tc.TH,
                                                    [ot for _, ot, _ in fs.values()])
    return {n: (res[k], out[k], disc[k]) for k, n in enumerate(fs)}


@pytest.mark.parametrize("name", sorted(tc.frames()))
def test_driver_equals_replay(replay, device, name):
    want = replay[1][name]
    res, out, disc = device[name]
    for k in ("ok", "searches", "mode", "nmatches", "nmatches_map", "vo", "n_good"):
        assert int(res[k]) == want[k], (k, int(res[k]), want[k])
    assert list(res["nmatches_search"]) == want["nmatches_search"]
    assert np.array_equal(out, want["out"])
    assert np.array_equal(disc, want["discarded"])
    assert np.asarray(res["Tcw"], np.float32).tobytes() == np.asarray(want["Tcw"], np.float32).tobytes()


def test_count_zero_and_arguments():
    from rsc import engine
    res, out, disc = engine.track_motion_model_many(ctx(), [], [], [], [], [])
    assert len(res) == 0 and out == [] and disc == []
    p = tc.frames()["small"][0]
    bare = engine.FrameView(ctx(), p.frame)
    lv = engine.LastFrameView(ctx(), p.last)
    with pytest.raises(RuntimeError):   # no rsc_frameview_set_stereo
        engine.track_motion_model_many(ctx(), [bare], [lv], [p.Tcw_cur], [p.Tcw_last], [p.mb], tc.TH)
    bare.set_stereo(p.frame.u_right, p.frame.mbf)
    with pytest.raises(RuntimeError):   # 2 * th leaves the grid arithmetic's range although th does not
        engine.track_motion_model_many(ctx(), [bare], [lv], [p.Tcw_cur], [p.Tcw_last], [p.mb], 2.0e9)
    res, out, _ = engine.track_motion_model_many(ctx(), [bare], [lv], [p.Tcw_cur], [p.Tcw_last], [p.mb], tc.TH, [1])
    assert int(res[0]["ok"]) == 0 and int(res[0]["searches"]) == 2
