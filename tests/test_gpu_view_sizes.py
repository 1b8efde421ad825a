"""The resident views at the sizes where a one-byte-per-element piece of their device image ends just before, on
and just after a 256-byte boundary (n = 255, 256, 257, and n = 1): each view kind (KeyFrame, with and without
triangulation data, Frame, MapPoints, LastFrame, BoW) is built at that size from the existing case builders and
goes through one matcher call, compared bit for bit with the matcher's sequential restatement (kfproj_ref,
fusekf_ref, localproj_ref, lastproj_ref, triang_ref) or, for SearchByBoW, the oracle.  And the view fact that
rsc_kfview_create works out once: a KeyFrame view with an octave equal to n_levels is refused by the two
matchers that index by octave, with the status they have always given, and the same KeyFrame still goes through
SearchBySim3."""
import functools

import numpy as np
import pytest

import fusekf_cases as fc
import fusekf_ref as fr
import kfproj_cases as kc
import kfproj_ref as kr
import lastproj_cases as lac
import localproj_cases as loc
import sim3match_ref as sr
import triang_cases as tc
import triang_gpu as tg
import triang_ref as tr
from gpu_common import ctx

pytestmark = pytest.mark.gpu
SIZES = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def loop_problem(n):
    """n keypoints, n MapPoints, one point per keypoint (no clusters: the sizes are what is under test)."""
    return kc.random_problem(100 + n, n_kf=n, n_points=n, n_clusters=0)


@functools.lru_cache(maxsize=None)
def fuse_problem(n):
    """loop_problem's KeyFrame with a third of its keypoints stereo, as fusekf_cases.random_problem makes them."""
    p = loop_problem(n)
    rng = np.random.default_rng(200 + n)
    ur = p.kf.kp[:, 0] - fc.MBF / rng.uniform(3, 9, n) + rng.normal(0, 1.5, n)
    ur = np.where(rng.random(n) < 0.3, np.maximum(ur, 0.0), -1.0).astype(np.float32)
    kf = fc.make_kf(p.kf.kp, p.kf.octave, p.kf.desc, ur, p.kf.Rcw, p.kf.tcw)
    return kf, p.pts, (rng.random(n) < 0.08).astype(np.uint8)


@pytest.mark.parametrize("n", SIZES)
def test_keyframe_and_mappoints(n):
    from test_gpu_kfproj import run_many
    p = loop_problem(n)
    n_ref, out_ref = kr.search_by_projection_kf(p.kf, p.pts, p.Scw, p.already, p.occupied, p.th)
    outs, nm, _ = run_many([p])
    assert np.array_equal(outs[0], out_ref) and int(nm[0]) == n_ref
    assert n == 1 or n_ref > n // 4  # the views were read, not skipped


@pytest.mark.parametrize("n", SIZES)
def test_keyframe_with_triangulation_data_fuse(n):
    from rsc import engine
    kf, pts, skip = fuse_problem(n)
    want = fr.fuse_kf(kf, pts, skip, fc.TH)
    kv = engine.KFView(ctx(), kf)
    kv.set_triangulation(kf)
    best, nf = engine.fuse_kf_many(ctx(), [kv], [engine.MPView(ctx(), pts)], [skip], fc.TH)
    assert np.array_equal(best[0], want) and int(nf[0]) == int((want >= 0).sum())
    assert n == 1 or int(nf[0]) > n // 4


@pytest.mark.parametrize("n", SIZES)
def test_frame_and_mappoints(n):
    from test_gpu_localproj import run_many
    p = loc.random_problem(300 + n, 5.0, n_frame=n, n_points=n, n_pairs=n // 4, n_clusters=0)
    want = loc.reference(p)
    r = run_many([p])
    assert np.array_equal(r["out"][0], want["out"])
    assert np.asarray(r["track"][0]).tobytes() == np.asarray(want["track"]).tobytes()
    assert (int(r["nmatches"][0]), int(r["n_to_match"][0]), int(r["rounds"][0])) == \
        (int(want["nmatches"]), int(want["n_to_match"]), int(want["rounds"]))


@pytest.mark.parametrize("n", SIZES)
def test_frame_and_lastframe(n):
    from test_gpu_lastproj import run_many
    p = lac.random_problem(400 + n, 7.0, 0, n_frame=n, n_last=n, n_clusters=0)
    want = lac.reference(p)
    r = run_many([p])
    assert np.array_equal(r["out"][0], want["out"])
    assert (int(r["nmatches"][0]), int(r["mode"][0]), int(r["rounds"][0])) == \
        (int(want["nmatches"]), int(want["mode"]), int(want["rounds"]))


@pytest.mark.parametrize("n", SIZES)
def test_bow_and_triangulation_views(n):
    """SearchForTriangulation reads the BoW view and the KeyFrame view of each side, the pair geometry the
    triangulation data; one node of n features on each side, shared."""
    from test_gpu_triang import run_many
    k1, k2 = tc.random_pair(np.random.default_rng(500 + n), n, n, [n], [n])
    want = tr.search_for_triangulation(k1, k2, tc.F_HORIZ, 0, 0, all_den_zero=True)
    r, pairs, st, x = run_many([(k1, k2, tc.F_HORIZ, 0, 0)])
    assert np.array_equal(r["matches12"][0], want["matches12"])
    assert (int(r["nmatches"][0]), int(r["den_zero"][0])) == (int(want["nmatches"]), int(want["den_zero"]))
    assert np.array_equal(r["den_zero_slot"][0], want["den_zero_slot"])
    assert pairs[0].tolist() == [list(q) for q in tr.matched_pairs(want["matches12"])]
    for k, (a, b) in enumerate(pairs[0]):
        s, x3d, _ = tr.triangulate_pair(k1, k2, a, b)
        assert int(st[0][k]) == s and np.array_equal(x[0][k].view(np.uint32), x3d.view(np.uint32)), (a, b)


@pytest.mark.parametrize("n", SIZES)
def test_bow_search(n):
    from rsc import synth
    from test_gpu_orbmatch import check_batch
    rng = np.random.default_rng(600 + n)
    F = synth.make_bow_view(rng, n)
    K = synth.make_bow_related(rng, F, n, 0.6, 30.0)
    check_batch(F, [K], True)
    check_batch(F, [K], False)


def test_octave_at_n_levels():
    """n_levels is 8.  Fuse indexes mvInvLevelSigma2 by the KeyFrame's octaves and SearchForTriangulation
    mvScaleFactors by KeyFrame 2's: both refuse the view (RSC_ERR_ARG, -1).  SearchBySim3 never indexes by octave."""
    from rsc import engine
    p = fc.cases()["no_claims"][0]
    q = fc.cases()["no_claims"][0]
    q.kf.octave = np.array([0, 8], np.int32)
    bad = engine.KFView(ctx(), q.kf)
    bad.set_triangulation(q.kf)
    with pytest.raises(RuntimeError, match=r"rsc_fuse_kf_many: invalid argument \(-1\)"):
        engine.fuse_kf_many(ctx(), [bad], [engine.MPView(ctx(), p.pts)], [p.skip], fc.TH)
    k1, k2, F = tc.matcher_cases()["tie_later"][:3]
    kb = tc.make_kf(k2.kp, [11, 11], desc=k2.desc, octave=[0, 8], tcw=(0, 0, 1))
    (b1, v1), (bb, vb) = tg.views(k1), tg.views(kb)
    with pytest.raises(RuntimeError, match=r"rsc_search_for_triangulation_many: invalid argument \(-1\)"):
        engine.search_for_triangulation_many(ctx(), [b1], [v1], [bb], [vb], [F])
    R12, t12, m12 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.full(q.kf.n, -1, np.int32)
    n_ref, out_ref = sr.py_search(q.kf, q.kf, R12, t12, m12)
    out, nfound = engine.search_by_sim3_many(ctx(), [(q.kf, q.kf, R12, t12, m12)])
    assert np.array_equal(out[0], out_ref) and int(nfound[0]) == n_ref
