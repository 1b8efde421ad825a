"""The loop-closing matchers on the device (kfproj.hip) against the golden fixture of the sequential
restatement (tests/golden/kfproj_traces.npz, written by tests/golden/make_kfproj_golden.py from
tests/kfproj_ref.py), bit for bit: rsc_search_by_projection_kf_many on the hand-built cases, the domino and
the random crowded problems, one launch of mixed problem sizes, and rsc_fuse_sim3_many with five KeyFrames
against the 1,500-point set."""
import os

import numpy as np
import pytest

import kfproj_cases as kc
import kfproj_ref as kr
from gpu_common import ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "kfproj_traces.npz"))


def run_many(ps):
    from rsc import engine
    kvs = [engine.KFView(ctx(), p.kf) for p in ps]
    mvs = [engine.MPView(ctx(), p.pts) for p in ps]
    oc0 = [p.occupied.copy() for p in ps]
    al0 = [p.already.copy() for p in ps]
    outs, nm, rounds = engine.search_by_projection_kf_many(ctx(), kvs, mvs, [p.Scw for p in ps],
                                                           [p.already for p in ps], [p.occupied for p in ps], ps[0].th)
    for k, p in enumerate(ps):
        assert np.array_equal(p.occupied, oc0[k]) and np.array_equal(p.already, al0[k])
    return outs, nm, rounds


def test_golden_problems_one_launch(golden):
    """Every problem of the fixture in one launch: the hand-built cases (one per rule), the domino (41 rounds)
    and the two crowded problems (KeyFrame n = 600 > the workgroup size, 1,500 points: the strided loops, the
    cached candidates and the fallback walk)."""
    names = [str(s) for s in golden["names"]]
    ps = [kc.from_arrays(golden, n) for n in names]
    outs, nm, rounds = run_many(ps)
    for k, n in enumerate(names):
        assert int(nm[k]) == int(golden[f"{n}/nmatches"][0]), f"{n}: nmatches {int(nm[k])}"
        assert np.array_equal(outs[k], golden[f"{n}/out"]), f"{n}: out"
        assert int(rounds[k]) == int(golden[f"{n}/rounds"][0]), f"{n}: rounds {int(rounds[k])}"
    cs = kc.cases()
    for k, n in enumerate(names):  # and the answers worked out by hand
        if n in cs:
            assert np.array_equal(outs[k], kc.expected_out(cs[n][0], cs[n][1])), n
    d = names.index("domino")
    assert int(rounds[d]) == 41 and np.array_equal(outs[d], np.arange(40))
    assert not np.array_equal(golden["domino/round1"], np.arange(40))  # round 1 alone is another answer
    for n in ("random_a", "random_b"):
        assert int(nm[names.index(n)]) >= 100


def test_mixed_sizes(golden):
    """count = 1; then one launch of a crowded problem, a problem with no eligible point, and a KeyFrame with
    n = 8192 (the whole owner table) against 3 points."""
    a = kc.from_arrays(golden, "random_b")
    outs, nm, rounds = run_many([a])
    assert int(nm[0]) == int(golden["random_b/nmatches"][0]) and np.array_equal(outs[0], golden["random_b/out"])
    assert int(rounds[0]) == int(golden["random_b/rounds"][0])
    none = kc.from_arrays(golden, "random_a")
    none.already = np.ones(none.pts.n, np.uint8)
    rng = np.random.default_rng(8)
    n = 8192
    kp = np.stack([rng.uniform(2, 750, n), rng.uniform(2, 478, n)], 1).astype(np.float32)
    big = kc.random_problem(9, 100, 200, n_clusters=4)
    big.kf = kc.make_kf(kp, rng.integers(0, 8, n), rng.integers(0, 256, (n, 32), dtype=np.uint8))
    big.occupied = np.zeros(n, np.uint8)
    T = big.Scw.astype(np.float64)
    pos, desc, dmax = [], [], []
    for f in (n - 1, 4000, 0):  # the last, a middle and the first slot of the table
        Xc = np.array([(kp[f, 0] - big.kf.cx) / big.kf.fx * 4.0, (kp[f, 1] - big.kf.cy) / big.kf.fy * 4.0, 4.0])
        Xw = T[:3, :3].T @ (Xc - T[:3, 3])
        pos.append(Xw)
        desc.append(big.kf.desc[f])
        dmax.append(np.linalg.norm(Xw + T[:3, :3].T @ T[:3, 3]) * 1.2 ** (int(big.kf.octave[f]) - 0.5))
    pos = np.array(pos)
    nrm = pos + T[:3, :3].T @ T[:3, 3]
    big.pts = kr.points_of(state=np.ones(3, np.uint8), pos=pos, normal=nrm, dmax=np.array(dmax, np.float32),
                           dmin=np.array(dmax, np.float32) / 4.0, desc=np.array(desc))
    big.already = np.zeros(3, np.uint8)
    n_ref, out_ref = kr.search_by_projection_kf(big.kf, big.pts, big.Scw, big.already, big.occupied, big.th)
    assert n_ref == 3 and out_ref[n - 1] == 0 and out_ref[4000] == 1 and out_ref[0] == 2
    outs, nm, rounds = run_many([a, none, big])
    assert int(nm[0]) == int(golden["random_b/nmatches"][0]) and np.array_equal(outs[0], golden["random_b/out"])
    assert int(nm[1]) == 0 and int(rounds[1]) == 1 and (outs[1] == -1).all()
    assert int(nm[2]) == 3 and np.array_equal(outs[2], out_ref) and int(rounds[2]) == 2


def test_fuse_batch(golden):
    from rsc import engine
    p = kc.from_arrays(golden, "random_a")
    k = len(golden["fuse/Scw"])
    assert k == 5 and p.pts.n == 1500
    kvs = [engine.KFView(ctx(), kc.make_kf(p.kf.kp, p.kf.octave, p.kf.desc, golden["fuse/mp_state"][c]))
           for c in range(k)]
    mv = engine.MPView(ctx(), p.pts)
    best, nf = engine.fuse_sim3_many(ctx(), kvs, mv, golden["fuse/Scw"], list(golden["fuse/in_kf"]),
                                     float(golden["fuse/th"][0]))
    for c in range(k):
        assert int(nf[c]) == int(golden["fuse/nfused"][c]) >= 100, c
        assert np.array_equal(best[c], golden["fuse/best_idx"][c]), c
    # the hand-built Fuse cases, each alone (their KeyFrames differ)
    for name, (q, exp) in sorted(kc.fuse_cases().items()):
        b, n1 = engine.fuse_sim3_many(ctx(), [engine.KFView(ctx(), q.kf)], engine.MPView(ctx(), q.pts), [q.Scw],
                                      [q.in_kf], float(q.th))
        assert b[0].tolist() == exp["best_idx"] and int(n1[0]) == sum(x >= 0 for x in exp["best_idx"]), name


def test_argument_errors():
    from rsc import engine
    p = kc.cases()["greedy_order"][0]
    kv, mv = engine.KFView(ctx(), p.kf), engine.MPView(ctx(), p.pts)
    outs, nm, rounds = engine.search_by_projection_kf_many(ctx(), [], [], [], [], [])  # count = 0: RSC_OK
    assert outs == [] and len(nm) == 0
    rng = np.random.default_rng(1)
    n = 8193  # one more keypoint than the owner table holds
    kp = np.stack([rng.uniform(2, 750, n), rng.uniform(2, 478, n)], 1).astype(np.float32)
    big = engine.KFView(ctx(), kc.make_kf(kp, np.zeros(n, np.int32), np.zeros((n, 32), np.uint8)))
    with pytest.raises(RuntimeError):
        engine.search_by_projection_kf_many(ctx(), [big], [mv], [p.Scw], [p.already], [np.zeros(n, np.uint8)])
    with pytest.raises(RuntimeError):
        engine.fuse_sim3_many(ctx(), [big], mv, [p.Scw], [p.already], 4.0)
    empty = engine.MPView(ctx(), kr.points_of(state=[], pos=[], normal=[], dmax=[], dmin=[], desc=[]))
    outs, nm, rounds = engine.search_by_projection_kf_many(ctx(), [kv], [empty], [p.Scw], [np.zeros(0, np.uint8)],
                                                           [p.occupied])
    assert int(nm[0]) == 0 and int(rounds[0]) == 1 and (outs[0] == -1).all()
    best, nf = engine.fuse_sim3_many(ctx(), [kv], empty, [p.Scw], [np.zeros(0, np.uint8)], 4.0)
    assert len(best[0]) == 0 and int(nf[0]) == 0
