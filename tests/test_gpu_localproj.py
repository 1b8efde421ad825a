"""Tracking::SearchLocalPoints on the device (localproj.hip) against the golden fixture of the sequential
restatement (tests/golden/localproj_traces.npz, written by tests/golden/make_localproj_golden.py from
tests/localproj_ref.py), bit for bit: rsc_search_local_points_many (fused) and
rsc_search_by_projection_points_many (matcher-only, on the fixture's track records) on the hand-built cases,
the domino and the crowded problems; one launch of mixed problem sizes; argument errors."""
import os

import numpy as np
import pytest

import kfproj_ref as kr
import localproj_cases as lc
import localproj_ref as lr
from gpu_common import ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "localproj_traces.npz"))


def views(ps):
    from rsc import engine
    fvs = [engine.FrameView(ctx(), p.frame) for p in ps]
    for v, p in zip(fvs, ps):
        v.set_stereo(p.frame.u_right, p.frame.mbf)
    return fvs, [engine.MPView(ctx(), p.pts) for p in ps]


def run_many(ps, tracks=None):
    """fused (tracks None) or matcher-only on `tracks`; checks that the inputs are unmodified."""
    from rsc import engine
    fvs, mvs = views(ps)
    ins = [[a.copy() for a in (p.skip, p.has_obs, p.frame_occ, np.asarray(p.Tcw))] for p in ps]
    tr0 = None if tracks is None else [np.array(t, lr.TRACK) for t in tracks]
    p0 = ps[0]
    if tracks is None:
        r = engine.search_local_points_many(ctx(), fvs, mvs, [p.Tcw for p in ps], [p.skip for p in ps],
                                            [p.has_obs for p in ps], [p.frame_occ for p in ps], p0.cos_limit, p0.th,
                                            p0.nn_ratio)
    else:
        r = engine.search_by_projection_points_many(ctx(), fvs, mvs, tracks, [p.skip for p in ps],
                                                    [p.has_obs for p in ps], [p.frame_occ for p in ps], p0.th,
                                                    p0.nn_ratio)
        for t, t0 in zip(tracks, tr0):
            assert np.asarray(t, lr.TRACK).tobytes() == t0.tobytes()
    for p, keep in zip(ps, ins):
        for a, b in zip((p.skip, p.has_obs, p.frame_occ, np.asarray(p.Tcw)), keep):
            assert np.array_equal(a, b)
    return r


def check(r, k, golden, n):
    c = golden[f"{n}/counts"]
    assert int(r["nmatches"][k]) == int(c[0]), f"{n}: nmatches {int(r['nmatches'][k])}"
    assert int(r["n_to_match"][k]) == int(c[1]), f"{n}: n_to_match {int(r['n_to_match'][k])}"
    assert np.array_equal(r["out"][k], golden[f"{n}/out"]), f"{n}: out"
    assert np.asarray(r["track"][k]).tobytes() == golden[f"{n}/track"].tobytes(), f"{n}: track"
    assert int(r["rounds"][k]) == int(c[2]), f"{n}: rounds {int(r['rounds'][k])}"


def by_th(golden):
    """th is one argument of a launch: the fixture's problems grouped by it."""
    groups = {}
    for n in (str(s) for s in golden["names"]):
        groups.setdefault(float(golden[f"{n}/par"][1]), []).append(n)
    return groups


@pytest.mark.parametrize("fused", [True, False])
def test_golden_problems_one_launch(golden, fused):
    """Every problem of the fixture, one launch per th (1, 4 and 5): the hand-built cases (one per rule), the
    domino (41 rounds) and the two crowded problems (Frame n = 600 > the workgroup size, 1,500 points: the
    strided loops, the cached candidates and the fallback walk)."""
    groups = by_th(golden)
    assert sorted(groups) == [1.0, 4.0, 5.0]
    seen = 0
    for th, names in groups.items():
        ps = [lc.from_arrays(golden, n) for n in names]
        r = run_many(ps, None if fused else [golden[f"{n}/track"] for n in names])
        for k, n in enumerate(names):
            check(r, k, golden, n)
        cs = lc.cases()
        for k, n in enumerate(names):  # and the answers worked out by hand
            if n in cs:
                assert np.array_equal(r["out"][k], lc.expected_out(cs[n][0], cs[n][1])), n
                assert int(r["nmatches"][k]) == cs[n][1]["nmatches"], n
        if "domino" in names:
            d = names.index("domino")
            assert int(r["rounds"][d]) == 41 and np.array_equal(r["out"][d], np.arange(40))
            assert not np.array_equal(golden["domino/round1"], np.arange(40))  # round 1 alone is another answer
        for n in lc.RANDOM:
            if n in names:
                assert int(r["nmatches"][names.index(n)]) >= 100
        seen += len(names)
    assert seen == len(golden["names"])


def test_mixed_sizes(golden):
    """count = 1; then one launch of a crowded problem, a problem with no eligible point (rounds == 1), and a
    Frame with n = 8192 (the whole owner table) against 3 points that hit the first, a middle and the last
    feature slot."""
    a = lc.from_arrays(golden, "random_b")
    r = run_many([a])
    check(r, 0, golden, "random_b")
    none = lc.from_arrays(golden, "random_b")
    none.skip = np.ones(none.pts.n, np.uint8)
    rng = np.random.default_rng(8)
    n = 8192
    kp = np.stack([rng.uniform(2, 750, n), rng.uniform(2, 478, n)], 1).astype(np.float32)
    octave = rng.integers(0, 8, n)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    fr = lc.make_frame(kp, octave, desc, np.full(n, -1.0, np.float32), mbf=a.frame.mbf)
    T = np.asarray(a.Tcw, np.float64)
    Ow = -T[:3, :3].T @ T[:3, 3]
    pos, pdesc, dmax = [], [], []
    for f in (n - 1, 4000, 0):  # the last, a middle and the first slot of the table
        Xc = np.array([(kp[f, 0] - fr.cx) / fr.fx * 4.0, (kp[f, 1] - fr.cy) / fr.fy * 4.0, 4.0])
        Xw = T[:3, :3].T @ (Xc - T[:3, 3])
        pos.append(Xw)
        pdesc.append(desc[f])
        dmax.append(np.linalg.norm(Xw - Ow) * 1.2 ** (int(octave[f]) - 0.5) if octave[f] else np.linalg.norm(Xw - Ow))
    pos = np.array(pos)
    big = lc.from_arrays(golden, "random_b")
    big.frame = fr
    big.pts = kr.points_of(state=np.ones(3, np.uint8), pos=pos, normal=pos - Ow, dmax=np.array(dmax, np.float32),
                           dmin=np.array(dmax, np.float32) / 4.0, desc=np.array(pdesc))
    big.skip = np.zeros(3, np.uint8)
    big.has_obs = np.ones(3, np.uint8)
    big.frame_occ = np.zeros(n, np.uint8)
    ref = lc.reference(big)
    assert ref["nmatches"] == 3 and ref["out"][n - 1] == 0 and ref["out"][4000] == 1 and ref["out"][0] == 2
    r = run_many([a, none, big])
    check(r, 0, golden, "random_b")
    assert int(r["nmatches"][1]) == 0 and int(r["n_to_match"][1]) == 0 and int(r["rounds"][1]) == 1
    assert (r["out"][1] == -1).all() and not r["track"][1]["in_view"].any()
    assert int(r["nmatches"][2]) == 3 and np.array_equal(r["out"][2], ref["out"])
    assert int(r["rounds"][2]) == ref["rounds"] and r["track"][2].tobytes() == ref["track"].tobytes()


def test_argument_errors():
    from rsc import engine
    p = lc.cases()["earlier_blocks"][0]
    (fv,), (mv,) = views([p])
    args = ([p.skip], [p.has_obs], [p.frame_occ])
    r = engine.search_local_points_many(ctx(), [], [], [], [], [], [])  # count = 0: RSC_OK
    assert r["out"] == [] and len(r["nmatches"]) == 0
    r = engine.search_by_projection_points_many(ctx(), [], [], [], [], [], [])
    assert r["out"] == []
    # a view without rsc_frameview_set_stereo
    bare = engine.FrameView(ctx(), p.frame)
    with pytest.raises(RuntimeError):
        engine.search_local_points_many(ctx(), [bare], [mv], [p.Tcw], *args)
    tr = lc.reference(p)["track"]
    with pytest.raises(RuntimeError):
        engine.search_by_projection_points_many(ctx(), [bare], [mv], [tr], *args)
    # one more feature than the owner table holds
    rng = np.random.default_rng(1)
    n = 8193
    kp = np.stack([rng.uniform(2, 750, n), rng.uniform(2, 478, n)], 1).astype(np.float32)
    with pytest.raises(RuntimeError):
        big = engine.FrameView(ctx(), lc.make_frame(kp, np.zeros(n, np.int32), np.zeros((n, 32), np.uint8),
                                                    np.full(n, -1.0, np.float32)))
        big.set_stereo(np.full(n, -1.0, np.float32), 40.0)
        engine.search_local_points_many(ctx(), [big], [mv], [p.Tcw], [p.skip], [p.has_obs], [np.zeros(n, np.uint8)])
    # a track level outside the pyramid on a point in view
    bad = tr.copy()
    bad["level"][0] = 8
    with pytest.raises(RuntimeError):
        engine.search_by_projection_points_many(ctx(), [fv], [mv], [bad], *args)
    # an empty point list
    empty = engine.MPView(ctx(), kr.points_of(state=[], pos=[], normal=[], dmax=[], dmin=[], desc=[]))
    z = np.zeros(0, np.uint8)
    r = engine.search_local_points_many(ctx(), [fv], [empty], [p.Tcw], [z], [z], [p.frame_occ])
    assert int(r["nmatches"][0]) == 0 and int(r["n_to_match"][0]) == 0 and int(r["rounds"][0]) == 1
    assert (r["out"][0] == -1).all() and len(r["track"][0]) == 0
    # and the call still works afterwards
    r = engine.search_local_points_many(ctx(), [fv], [mv], [p.Tcw], *args)
    assert r["out"][0].tolist() == [0, 1] and int(r["nmatches"][0]) == 2
