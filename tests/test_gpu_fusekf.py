"""ORBmatcher::Fuse(pKF, vpMapPoints, th) on the device (fusekf.hip, rsc_fuse_kf_many) against the golden fixture of
the sequential restatement (tests/golden/fusekf_traces.npz, written by tests/golden/make_fusekf_golden.py from
tests/fusekf_ref.py), bit for bit: every hand-built case and the random crowded problems in one launch, one launch
of mixed problem sizes and shared views, and the argument checks."""
import os

import numpy as np
import pytest

import fusekf_cases as fc
import fusekf_ref as fr
from gpu_common import ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "fusekf_traces.npz"))


@pytest.fixture(scope="module")
def randoms():
    return {name: fc.random_problem(seed) for name, seed in fc.RANDOM_SEEDS.items()}


def kview(kf, triangulation=True):
    from rsc import engine
    v = engine.KFView(ctx(), kf)
    if triangulation:
        v.set_triangulation(kf)
    return v


def mview(pts):
    from rsc import engine
    return engine.MPView(ctx(), pts)


def subset(pts, sel):
    return fr.kr.points_of(state=pts.state[sel], pos=pts.pos[sel], normal=pts.normal[sel], dmax=pts.dmax[sel],
                           dmin=pts.dmin[sel], desc=pts.desc[sel])


def test_golden_problems_one_launch(golden, randoms):
    """Every case (one per rule, each with its own KeyFrame and th = 3 but for window_edge) and the six random
    (pose, 1,500 points) problems, three poses sharing each point view.  th is one value per launch, so the th = 2
    case goes in a launch of its own."""
    from rsc import engine
    cs = fc.cases()
    names = [n for n in sorted(cs) if cs[n][0].th == fc.TH]
    kvs = [kview(cs[n][0].kf) for n in names]
    mvs = [mview(cs[n][0].pts) for n in names]
    skips = [cs[n][0].skip for n in names]
    want = [golden[f"{n}/best_idx"] for n in names]
    for name in sorted(randoms):
        pts, kfs, sk = randoms[name]
        mv = mview(pts)
        for k, kf in enumerate(kfs):
            kvs.append(kview(kf))
            mvs.append(mv)
            skips.append(sk[k])
            want.append(golden[f"{name}/{k}/best_idx"])
    skip0 = [s.copy() for s in skips]
    best, nf = engine.fuse_kf_many(ctx(), kvs, mvs, skips, fc.TH)
    labels = names + [f"{n}/{k}" for n in sorted(randoms) for k in range(3)]
    for c, label in enumerate(labels):
        assert np.array_equal(best[c], want[c]), label
        assert int(nf[c]) == int((want[c] >= 0).sum()), label
        assert np.array_equal(skips[c], skip0[c])
    for n, b in zip(names, best):  # and the answers worked out by hand
        assert b.tolist() == cs[n][1], n
    assert all(int(x) >= 100 for x in nf[len(names):])
    rest = [n for n in sorted(cs) if cs[n][0].th != fc.TH]
    assert rest == ["window_edge"]
    p, exp = cs["window_edge"]
    best, nf = engine.fuse_kf_many(ctx(), [kview(p.kf)], [mview(p.pts)], [p.skip], p.th)
    assert best[0].tolist() == exp and int(nf[0]) == 2


def test_mixed_launch(golden, randoms):
    """Point counts 0, 1, 17 and 1,500 in one launch; one view shared by five KeyFrames next to per-problem views; a
    KeyFrame with n = 8192 whose first, middle and last slots are matched.  No pair depends on another, so a
    subset of a fixture problem's points has the fixture's answers."""
    from rsc import engine
    pts_a, kfs_a, sk_a = randoms["random_a"]
    pts_b, kfs_b, sk_b = randoms["random_b"]
    gold_b = golden["random_b/0/best_idx"]
    hit, miss = np.nonzero(gold_b >= 0)[0], np.nonzero(gold_b < 0)[0]
    sel17 = np.sort(np.concatenate([hit[:9], miss[:8]]))
    sel1 = hit[5:6]
    empty = fr.kr.points_of(state=[], pos=[], normal=[], dmax=[], dmin=[], desc=np.zeros((0, 32), np.uint8))
    # the big KeyFrame: identity pose, three points on keypoints n - 1, 4000 and 0 with their descriptors
    rng = np.random.default_rng(8)
    n = 8192
    kp = np.stack([rng.uniform(2, 750, n), rng.uniform(2, 478, n)], 1).astype(np.float32)
    big = fc.make_kf(kp, rng.integers(0, 8, n), rng.integers(0, 256, (n, 32), dtype=np.uint8), np.full(n, -1.0))
    pos, dmax, desc = [], [], []
    for f in (n - 1, 4000, 0):
        X = np.array([(kp[f, 0] - big.cx) / big.fx * 4.0, (kp[f, 1] - big.cy) / big.fy * 4.0, 4.0])
        pos.append(X)
        dmax.append(np.linalg.norm(X) * 1.2 ** (int(big.octave[f]) - 0.5))
        desc.append(big.desc[f])
    pts3 = fr.kr.points_of(state=np.ones(3, np.uint8), pos=pos, normal=pos, dmax=np.array(dmax, np.float32),
                           dmin=np.array(dmax, np.float32) / 4.0, desc=np.array(desc))
    want3 = fr.fuse_kf(big, pts3, np.zeros(3, np.uint8), fc.TH)
    assert want3.tolist() == [n - 1, 4000, 0]
    mv_a = mview(pts_a)
    order = [0, 1, 2, 1, 0]  # five KeyFrame views on one point view
    kvs = [kview(kfs_a[k]) for k in order] + [kview(kfs_b[0]) for _ in range(3)] + [kview(big)]
    mvs = [mv_a] * 5 + [mview(empty), mview(subset(pts_b, sel1)), mview(subset(pts_b, sel17)), mview(pts3)]
    skips = [sk_a[k] for k in order] + [np.zeros(0, np.uint8), sk_b[0][sel1], sk_b[0][sel17], np.zeros(3, np.uint8)]
    want = [golden[f"random_a/{k}/best_idx"] for k in order] + [np.zeros(0, np.int32), gold_b[sel1], gold_b[sel17],
                                                                  want3]
    best, nf = engine.fuse_kf_many(ctx(), kvs, mvs, skips, fc.TH)
    for c in range(len(kvs)):
        assert np.array_equal(best[c], want[c]), c
        assert int(nf[c]) == int((want[c] >= 0).sum()), c
    assert [len(b) for b in best[5:]] == [0, 1, 17, 3] and int(nf[6]) == 1 and int(nf[7]) == 9


def test_timing_reports_the_kernel(randoms):
    from rsc import engine
    pts, kfs, sk = randoms["random_a"]
    c = ctx()
    c.enable_timing(True)
    try:
        engine.fuse_kf_many(c, [kview(kfs[0])], [mview(pts)], [sk[0]], fc.TH)
        assert c.last_timing()["refine_ms"] > 0.0
    finally:
        c.enable_timing(False)


def test_argument_errors(randoms):
    from rsc import engine
    p = fc.cases()["no_claims"][0]
    kv, mv = kview(p.kf), mview(p.pts)
    best, nf = engine.fuse_kf_many(ctx(), [], [], [], fc.TH)  # count = 0: RSC_OK
    assert best == [] and len(nf) == 0
    empty = mview(fr.kr.points_of(state=[], pos=[], normal=[], dmax=[], dmin=[], desc=np.zeros((0, 32), np.uint8)))
    best, nf = engine.fuse_kf_many(ctx(), [kv, kv], [empty, empty], [np.zeros(0, np.uint8)] * 2, fc.TH)
    assert [len(b) for b in best] == [0, 0] and nf.tolist() == [0, 0]
    ok = lambda: engine.fuse_kf_many(ctx(), [kv], [mv], [p.skip], fc.TH)
    assert ok()[0][0].tolist() == [0, 0]
    with pytest.raises(RuntimeError):  # no rsc_kfview_set_triangulation: no u_right, mbf, Ow
        engine.fuse_kf_many(ctx(), [kv, kview(p.kf, triangulation=False)], [mv, mv], [p.skip, p.skip], fc.TH)
    rng = np.random.default_rng(1)
    n = 8193  # one more keypoint than a KeyFrame view may hold for the matchers
    kp = np.stack([rng.uniform(2, 750, n), rng.uniform(2, 478, n)], 1).astype(np.float32)
    big = kview(fc.make_kf(kp, np.zeros(n, np.int32), np.zeros((n, 32), np.uint8), np.full(n, -1.0)))
    with pytest.raises(RuntimeError):
        engine.fuse_kf_many(ctx(), [big], [mv], [p.skip], fc.TH)
    for octave in (8, -1):  # outside [0, n_levels): the index of mvInvLevelSigma2
        q = fc.cases()["no_claims"][0]
        q.kf.octave = np.array([0, octave], np.int32)
        with pytest.raises(RuntimeError):
            engine.fuse_kf_many(ctx(), [kview(q.kf)], [mv], [p.skip], fc.TH)
    for th in (np.nan, np.inf, -np.inf, 1e10, -1e10):  # non-finite, and th * 1.2^7 / 10 >= 2^30 cells
        with pytest.raises(RuntimeError):
            engine.fuse_kf_many(ctx(), [kv], [mv], [p.skip], th)
    assert ok()[0][0].tolist() == [0, 0]  # the refused calls left the context usable
