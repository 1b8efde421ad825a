"""ORBmatcher::SearchByProjection(Frame&, KeyFrame, sAlreadyFound, th, ORBdist) on the device
(rsc_search_by_projection_many, frameproj.hip) against the sequential Python reference
(tests/frameproj_ref.py), bit for bit: the hand-built cases and the domino, one launch of mixed problem
sizes, and random crowded problems with both parameter sets of Tracking::Relocalization."""
import numpy as np
import pytest

import frameproj_cases as fc
import frameproj_ref as fr
from gpu_common import ctx

pytestmark = pytest.mark.gpu


def ref(p, trace=None):
    return fr.search_by_projection(p.frame, p.kf, p.Tcw, p.already, p.frame_mp, p.th, p.orb_dist,
                                   p.check_orientation, trace)


def views(p, angles=True):
    from rsc import engine
    kv = engine.KFView(ctx(), p.kf)
    if angles:
        kv.set_angles(p.kf.angle)
    return engine.FrameView(ctx(), p.frame), kv


def run_many(ps, th, orb_dist, check_orientation):
    """One launch over the problems; checks out / nmatches / rounds against the reference and that the
    inputs are unchanged."""
    from rsc import engine
    vs = [views(p) for p in ps]
    mp0 = [p.frame_mp.copy() for p in ps]
    al0 = [p.already.copy() for p in ps]
    outs, nm, rounds = engine.search_by_projection_many(ctx(), [v[0] for v in vs], [v[1] for v in vs],
                                                        [p.Tcw for p in ps], [p.already for p in ps],
                                                        [p.frame_mp for p in ps], th, orb_dist, check_orientation)
    for k, p in enumerate(ps):
        n, out = ref(p)
        assert int(nm[k]) == n, f"problem {k}: nmatches {int(nm[k])} vs {n}"
        assert np.array_equal(outs[k], out), f"problem {k}: out"
        assert 1 <= int(rounds[k]) <= fr.n_eligible(p.kf, p.already) + 1, f"problem {k}: rounds {int(rounds[k])}"
        assert np.array_equal(p.frame_mp, mp0[k]) and np.array_equal(p.already, al0[k])
    return outs, nm, rounds


def test_hand_built_cases_and_domino():
    cs = fc.cases()
    names = sorted(cs)
    dom, dom_exp = fc.domino(70)
    for chk in (True, False):  # one launch per orientation setting
        sel = [n for n in names if cs[n][0].check_orientation == chk]
        ps = [cs[n][0] for n in sel] + ([dom] if chk else [])
        outs, nm, rounds = run_many(ps, fc.TH, fc.ORB_DIST, chk)
        for k, n in enumerate(sel):  # and the answers worked out by hand
            assert np.array_equal(outs[k], fc.expected_out(cs[n][0], cs[n][1])), n
        if chk:
            assert np.array_equal(outs[-1], fc.expected_out(dom, dom_exp)) and int(nm[-1]) == 70
            assert int(rounds[-1]) <= 71


def test_mixed_sizes_one_launch():
    """KeyFrame n in {37, 600} (600 > the workgroup size: the strided loops), Frame n in {50, 1500}, and a
    problem without an eligible MapPoint."""
    ps = [fc.random_problem(20 + k, n_kf, n_frame, 10, 100, n_clusters=2 if n_kf < 100 else 6)
          for k, (n_kf, n_frame) in enumerate([(37, 50), (37, 1500), (600, 50), (600, 1500)])]
    none = fc.random_problem(30, 600, 1500, 10, 100)
    none.already = np.ones(none.kf.n, np.uint8)
    ps.append(none)
    outs, nm, rounds = run_many(ps, 10, 100, True)
    assert int(nm[-1]) == 0 and int(rounds[-1]) == 1 and (outs[-1] == -1).all()
    assert int(nm[3]) > 100


@pytest.mark.parametrize("th,orb_dist", [(10, 100), (3, 64)])
def test_random_crowded(th, orb_dist):
    ps = [fc.random_problem(40 + k, 600, 1500, th, orb_dist, n_clusters=8) for k in range(3)]
    for p in ps:  # the greedy path is exercised
        tr = {}
        ref(p, tr)
        assert int((tr["claim"] != tr["free_best"]).sum()) >= 10
    run_many(ps, th, orb_dist, True)


def test_argument_errors():
    from rsc import engine
    L = engine.load_library()
    p = fc.cases()["greedy_order"][0]
    fv, kv = views(p)
    args = lambda: (ctx(), [fv], [kv], [p.Tcw], [p.already], [p.frame_mp])
    with pytest.raises(RuntimeError):
        engine.search_by_projection_many(*args(), 10, 256, True)       # the reference would index -1
    with pytest.raises(RuntimeError):
        engine.search_by_projection_many(*args(), 10, -1, True)
    _, kv_plain = views(p, angles=False)
    with pytest.raises(RuntimeError):
        engine.search_by_projection_many(ctx(), [fv], [kv_plain], [p.Tcw], [p.already], [p.frame_mp], 10, 100, True)
    outs, nm, _ = engine.search_by_projection_many(ctx(), [fv], [kv_plain], [p.Tcw], [p.already], [p.frame_mp], 10,
                                                   100, False)      # no check: no angles needed
    assert int(nm[0]) == 2
    outs, nm, rounds = engine.search_by_projection_many(ctx(), [], [], [], [], [], 10, 100, True)  # count = 0: RSC_OK
    assert outs == [] and len(nm) == 0 and len(rounds) == 0
    z = np.zeros((1, 16), np.float32)
    i1 = np.zeros(1, np.int32)
    assert L.rsc_search_by_projection_many(ctx().h, None, None, 0, z, None, None, 10.0, 100, 1, None, i1, i1) == 0
    assert L.rsc_search_by_projection_many(ctx().h, None, None, 0, z, None, None, 10.0, 256, 1, None, i1, i1) == -1
