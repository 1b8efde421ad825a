"""ORBmatcher::SearchForTriangulation and the pair geometry of CreateNewMapPoints on the device (triang.hip) against
the golden fixture of the sequential restatement (tests/golden/triang_traces.npz, written by
tests/golden/make_triang_golden.py from tests/triang_ref.py), bit for bit: matches12, nmatches, den_zero, the slot
flags, status codes and x3D bits; launches that mix problem sizes; argument errors."""
import os

import numpy as np
import pytest

import triang_cases as tc
import triang_gpu as tg
from gpu_common import ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "triang_traces.npz"))


@pytest.fixture(scope="module")
def problems():
    return tc.fixture_problems()


def run_many(ps):
    """One matcher launch over problems that share check_ori (bOnlyStereo is per problem), then one triangulation
    launch over their matches; checks that the inputs are unmodified."""
    from rsc import engine
    kfs = [k for p in ps for k in p[:2]]
    snap = tg.snapshot(kfs)
    v1, v2 = [tg.views(p[0]) for p in ps], [tg.views(p[1]) for p in ps]
    r = engine.search_for_triangulation_many(ctx(), [v[0] for v in v1], [v[1] for v in v1], [v[0] for v in v2],
                                             [v[1] for v in v2], [p[2] for p in ps], only_stereo=[p[3] for p in ps],
                                             check_orientation=bool(ps[0][4]))
    pairs = [np.array([(i, v) for i, v in enumerate(m) if v >= 0], np.int32).reshape(-1, 2) for m in r["matches12"]]
    st, x = engine.triangulate_pairs_many(ctx(), [v[1] for v in v1], [v[1] for v in v2], pairs)
    assert tg.unchanged(kfs, snap)
    return r, pairs, st, x


def check(r, pairs, st, x, k, golden, n):
    c = golden[f"{n}/counts"]
    assert np.array_equal(r["matches12"][k], golden[f"{n}/matches12"]), f"{n}: matches12"
    assert int(r["nmatches"][k]) == int(c[0]) and int(r["den_zero"][k]) == int(c[1]), f"{n}: counts"
    assert np.array_equal(r["den_zero_slot"][k], golden[f"{n}/den_zero_slot"]), f"{n}: den_zero_slot"
    assert np.array_equal(pairs[k], golden[f"{n}/pairs"]), f"{n}: pairs"
    assert np.array_equal(st[k], golden[f"{n}/status"]), f"{n}: status"
    assert np.array_equal(x[k].view(np.uint32), golden[f"{n}/x3d"].view(np.uint32)), f"{n}: x3D bits"


def test_golden_problems(golden, problems):
    """Every problem of the fixture, one launch per check_orientation, each mixing problem sizes and both bOnlyStereo
    values (the orientation check is a member of the reference's matcher object, one value per launch): the
    hand-built cases, the winner
    positions (position 0, the last, across a group edge, ties on two lanes), KeyFrame-2 nodes of 1, 2, 63 / 64 /
    65, 255 / 256 / 257 and 700 features, KeyFrame-1 nodes of 1 and 65, and the 8192-feature view of single-feature
    nodes."""
    groups = {}
    for n in (str(s) for s in golden["names"]):
        groups.setdefault(problems[n][4], []).append(n)
    assert sorted(groups) == [0, 1] and all({problems[n][3] for n in g} == {0, 1} for g in groups.values())
    cases = tc.matcher_cases()
    for names in groups.values():
        r, pairs, st, x = run_many([problems[n] for n in names])
        for k, n in enumerate(names):
            check(r, pairs, st, x, k, golden, n)
            if n in cases and cases[n][5] is not None:  # and the answers worked out by hand
                assert r["matches12"][k].tolist() == cases[n][5], n
                assert (int(r["nmatches"][k]), int(r["den_zero"][k])) == cases[n][6:8], n
    assert tc.winner_positions()[2] == golden["winner_positions/matches12"].tolist()


def test_per_call_flags_and_count_one(golden, problems):
    """count = 1, and has_mp1 / has_mp2 given per call: the view's own flags passed explicitly give the same answer,
    all-ones flags on KeyFrame 2 leave no candidate."""
    from rsc import engine
    n = "shapes_64_s0o0"
    k1, k2, F = problems[n][:3]
    (b1, v1), (b2, v2) = tg.views(k1), tg.views(k2)
    for h1, h2, same in (([k1.mp_state != 0], [k2.mp_state != 0], True), (None, [np.ones(k2.n, np.uint8)], False),
                         ([None], None, True)):
        r = engine.search_for_triangulation_many(ctx(), [b1], [v1], [b2], [v2], [F], has_mp1=h1, has_mp2=h2)
        if same:
            assert np.array_equal(r["matches12"][0], golden[f"{n}/matches12"])
            assert int(r["nmatches"][0]) == int(golden[f"{n}/counts"][0])
        else:
            assert int(r["nmatches"][0]) == 0 and (r["matches12"][0] == -1).all()


def test_pair_cases(golden):
    """Every hand-built pair case in one launch: each status code, the `else if` stereo-cosine quirk, the mbf quirk,
    temp(3) == 0, the NaN error that passes."""
    from rsc import engine
    cs = tc.pair_cases()
    names = list(cs)
    v1 = [tg.views(cs[n][0])[1] for n in names]
    v2 = [tg.views(cs[n][1])[1] for n in names]
    st, x = engine.triangulate_pairs_many(ctx(), v1, v2, [[[cs[n][2], cs[n][3]]] for n in names])
    for k, n in enumerate(names):
        assert int(st[k][0]) == int(golden[f"pair/{n}/status"]) == cs[n][4], (n, int(st[k][0]))
        assert np.array_equal(x[k][0].view(np.uint32), golden[f"pair/{n}/x3d"].view(np.uint32)), n


def test_argument_errors(problems):
    from rsc import engine
    k1, k2, F = problems["tie_later"][:3]
    (b1, v1), (b2, v2) = tg.views(k1), tg.views(k2)
    call = lambda a=b1, b=v1, c=b2, d=v2, f=F: engine.search_for_triangulation_many(ctx(), [a], [b], [c], [d], [f])
    r = engine.search_for_triangulation_many(ctx(), [], [], [], [], [])  # count = 0: RSC_OK
    assert r["matches12"] == [] and len(r["nmatches"]) == 0
    assert engine.triangulate_pairs_many(ctx(), [], [], []) == ([], [])
    # a view without rsc_kfview_set_triangulation, on either side and in the geometry
    bare = tg.views(k2, triangulation=False)[1]
    for kw in (dict(d=bare), dict(b=tg.views(k1, triangulation=False)[1])):
        with pytest.raises(RuntimeError):
            call(**kw)
    with pytest.raises(RuntimeError):
        engine.triangulate_pairs_many(ctx(), [v1], [bare], [[[0, 0]]])
    # non-finite F12
    for bad in (np.nan, np.inf, -np.inf):
        Fb = np.array(F, np.float32)
        Fb[1, 2] = bad
        with pytest.raises(RuntimeError):
            call(f=Fb)
    # an octave outside [0, n_levels) on a KeyFrame-2 feature
    for o in (8, -1):
        kb = tc.make_kf(k2.kp, [11, 11], desc=k2.desc, octave=[0, o], tcw=(0, 0, 1))
        bb, vb = tg.views(kb)
        with pytest.raises(RuntimeError):
            call(c=bb, d=vb)
    # the bow view and the kfview of one KeyFrame differ in size
    with pytest.raises(RuntimeError):
        call(c=b1)
    # more than 8192 keypoints
    n = 8193
    big = tc.make_kf(np.zeros((n, 2)), np.full(n, 11))
    vbig = engine.KFView(ctx(), big)
    vbig.set_triangulation(big)
    with pytest.raises(RuntimeError):
        engine.triangulate_pairs_many(ctx(), [vbig], [v2], [[[0, 0]]])
    # a pair index out of range
    for pr in ([[1, 0]], [[0, 2]], [[-1, 0]]):
        with pytest.raises(RuntimeError):
            engine.triangulate_pairs_many(ctx(), [v1], [v2], [pr])
    # and the call still works afterwards
    assert call()["matches12"][0].tolist() == [1]
