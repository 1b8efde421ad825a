"""ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) on the device (lastproj.hip) against the golden
fixture of the sequential restatement (tests/golden/lastproj_traces.npz, written by
tests/golden/make_lastproj_golden.py from tests/lastproj_ref.py), bit for bit: the hand-built cases, the domino
and the crowded problems; one launch of mixed problem sizes; argument errors."""
import os

import numpy as np
import pytest

import lastproj_cases as lc
from gpu_common import ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "lastproj_traces.npz"))


def views(ps):
    from rsc import engine
    fvs = [engine.FrameView(ctx(), p.frame) for p in ps]
    for v, p in zip(fvs, ps):
        v.set_stereo(p.frame.u_right, p.frame.mbf)
    return fvs, [engine.LastFrameView(ctx(), p.last) for p in ps]


def _inputs(p):
    return (p.frame_occ, np.asarray(p.Tcw_cur), np.asarray(p.Tcw_last), p.last.mp_state, p.last.mp_has_obs,
            p.last.mp_pos, p.frame.kp)


def run_many(ps):
    """One launch over `ps` (one th, one check_ori); checks that the inputs are unmodified."""
    from rsc import engine
    fvs, lvs = views(ps)
    ins = [[a.copy() for a in _inputs(p)] for p in ps]
    p0 = ps[0]
    assert all(p.th == p0.th and p.check_ori == p0.check_ori for p in ps)
    r = engine.search_by_projection_last_many(ctx(), fvs, lvs, [p.Tcw_cur for p in ps], [p.Tcw_last for p in ps],
                                              [p.mb for p in ps], [p.frame_occ for p in ps], p0.th,
                                              bool(p0.check_ori))
    for p, keep in zip(ps, ins):
        for a, b in zip(_inputs(p), keep):
            assert np.array_equal(a, b)
    return r


def check(r, k, golden, n):
    c = golden[f"{n}/counts"]
    assert int(r["nmatches"][k]) == int(c[0]), f"{n}: nmatches {int(r['nmatches'][k])}"
    assert int(r["mode"][k]) == int(c[1]), f"{n}: mode {int(r['mode'][k])}"
    assert np.array_equal(r["out"][k], golden[f"{n}/out"]), f"{n}: out"
    assert int(r["rounds"][k]) == int(c[2]), f"{n}: rounds {int(r['rounds'][k])}"


def by_launch(golden):
    """th and check_orientation are arguments of a launch: the fixture's problems grouped by them."""
    groups = {}
    for n in (str(s) for s in golden["names"]):
        par = golden[f"{n}/par"]
        groups.setdefault((float(par[1]), int(par[2])), []).append(n)
    return groups


def test_golden_problems_one_launch_per_th(golden):
    """Every problem of the fixture, one launch per (th, check_orientation): the hand-built cases (one per
    rule), the domino (41 rounds) and the crowded problems, one per level mode (current Frame n = 600 > the
    workgroup size, 1,500 LastFrame slots: the strided loops, the cached candidates, the 16-lane fallback walk,
    claims overwritten and the per-entry removal)."""
    groups = by_launch(golden)
    assert sorted(groups) == [(2.5, 0), (2.5, 1), (7.0, 1), (8.0, 1), (10.0, 1), (15.0, 1)]
    cs = lc.cases()
    seen = 0
    for names in groups.values():
        ps = [lc.from_arrays(golden, n) for n in names]
        r = run_many(ps)
        for k, n in enumerate(names):
            check(r, k, golden, n)
            if n in cs:  # and the answers worked out by hand
                assert np.array_equal(r["out"][k], lc.expected_out(cs[n][0], cs[n][1])), n
                assert int(r["nmatches"][k]) == cs[n][1]["nmatches"], n
                assert int(r["mode"][k]) == cs[n][1]["mode"], n
        if "domino" in names:
            d = names.index("domino")
            assert int(r["rounds"][d]) == 41 and np.array_equal(r["out"][d], np.arange(40))
            assert not np.array_equal(golden["domino/round1"], np.arange(40))  # round 1 alone is another answer
        for n in lc.RANDOM:
            if n in names:
                k = names.index(n)
                assert int(r["nmatches"][k]) >= 100 and int(r["rounds"][k]) >= 3 and (r["out"][k] == -2).any()
        seen += len(names)
    assert seen == len(golden["names"])


def _big_problem(a):
    """A current Frame with n = 8192 (the whole owner table) against 3 LastFrame slots that hit the last, a
    middle and the first feature slot."""
    rng = np.random.default_rng(8)
    n = 8192
    kp = np.stack([rng.uniform(2, 740, n), rng.uniform(2, 470, n)], 1).astype(np.float32)
    octave = rng.integers(0, 8, n)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    fr = lc.make_frame(kp, octave, desc, np.full(n, -1.0, np.float32), mbf=a.frame.mbf)
    fr.angle = np.zeros(n, np.float32)
    T = np.asarray(a.Tcw_cur, np.float64)
    hit = (n - 1, 4000, 0)
    pos = []
    for f in hit:
        Xc = np.array([(kp[f, 0] - fr.cx) / fr.fx * 4.0, (kp[f, 1] - fr.cy) / fr.fy * 4.0, 4.0])
        pos.append(T[:3, :3].T @ (Xc - T[:3, 3]))
    big = lc.from_arrays_like(a, fr, lc.last_of(octave[list(hit)], np.zeros(3), np.ones(3, np.uint8), np.array(pos),
                                               desc[list(hit)], np.ones(3, np.uint8)))
    return big, hit


def test_mixed_sizes(golden):
    """count = 1; then one launch of a crowded problem, a problem with no eligible slot (rounds == 1), and the
    n = 8192 Frame."""
    a = lc.from_arrays(golden, "random_a")
    r = run_many([a])
    check(r, 0, golden, "random_a")
    none = lc.from_arrays(golden, "random_a")
    none.last.mp_state = np.where(none.last.mp_state == 1, 2, none.last.mp_state).astype(np.uint8)
    big, hit = _big_problem(a)
    ref = lc.reference(big)
    assert ref["nmatches"] == 3 and [int(ref["out"][f]) for f in hit] == [0, 1, 2]
    r = run_many([a, none, big])
    check(r, 0, golden, "random_a")
    assert int(r["nmatches"][1]) == 0 and int(r["rounds"][1]) == 1 and (r["out"][1] == -1).all()
    assert int(r["mode"][1]) == int(golden["random_a/counts"][1])
    assert int(r["nmatches"][2]) == 3 and np.array_equal(r["out"][2], ref["out"])
    assert int(r["rounds"][2]) == ref["rounds"] and int(r["mode"][2]) == ref["mode"]


def test_argument_errors():
    from rsc import engine
    p = lc.cases()["greedy_promoted"][0]
    (fv,), (lv,) = views([p])
    call = lambda f, l, th=p.th: engine.search_by_projection_last_many(ctx(), [f], [l], [p.Tcw_cur], [p.Tcw_last],
                                                                       [p.mb], [p.frame_occ], th)
    r = engine.search_by_projection_last_many(ctx(), [], [], [], [], [])  # count = 0: RSC_OK
    assert r["out"] == [] and len(r["nmatches"]) == 0
    # a view without rsc_frameview_set_stereo
    bare = engine.FrameView(ctx(), p.frame)
    with pytest.raises(RuntimeError):
        call(bare, lv)
    # one more feature / slot than the tables hold
    rng = np.random.default_rng(1)
    n = 8193
    kp = np.stack([rng.uniform(2, 740, n), rng.uniform(2, 470, n)], 1).astype(np.float32)
    with pytest.raises(RuntimeError):
        engine.FrameView(ctx(), lc.make_frame(kp, np.zeros(n, np.int32), np.zeros((n, 32), np.uint8),
                                              np.full(n, -1.0, np.float32)))
    with pytest.raises(RuntimeError):
        engine.LastFrameView(ctx(), lc.last_of(np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.uint8),
                                               np.zeros((n, 3)), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)))
    # an octave outside the pyramid: refused on a slot with a MapPoint (an outlier included), ignored on an empty one
    for state, refused in ((1, True), (2, True), (0, False)):
        bad = lc.last_of([8, 0], [0, 0], [state, 1], p.last.mp_pos, p.last.mp_desc, [1, 1])
        bv = engine.LastFrameView(ctx(), bad)
        if refused:
            with pytest.raises(RuntimeError):
                call(fv, bv)
        else:
            assert call(fv, bv)["out"][0].tolist() == [1, -1]   # slot 1 alone takes the 2-bit feature
    neg = engine.LastFrameView(ctx(), lc.last_of([-1, 0], [0, 0], [1, 1], p.last.mp_pos, p.last.mp_desc, [1, 1]))
    with pytest.raises(RuntimeError):
        call(fv, neg)
    # th: not finite, or a radius beyond the grid arithmetic's int range (2^30 cells)
    for th in (float("nan"), float("inf"), -float("inf"), 1e10, -1e10):
        with pytest.raises(RuntimeError):
            call(fv, lv, th)
    # an empty LastFrame, and frame_occ = None (all free)
    empty = engine.LastFrameView(ctx(), lc.last_of([], [], [], np.zeros((0, 3)), np.zeros((0, 32), np.uint8), []))
    r = call(fv, empty)
    assert int(r["nmatches"][0]) == 0 and int(r["rounds"][0]) == 1 and (r["out"][0] == -1).all()
    r = engine.search_by_projection_last_many(ctx(), [fv], [lv], [p.Tcw_cur], [p.Tcw_last], [p.mb], None, p.th)
    assert r["out"][0].tolist() == [0, 1]
    # and the call still works afterwards
    r = call(fv, lv)
    assert r["out"][0].tolist() == [0, 1] and int(r["nmatches"][0]) == 2 and int(r["mode"][0]) == 0
