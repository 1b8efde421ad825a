"""GPU parity of the PnP scan's two-segment counting (kernels.hip pnp_scan_kernel, rsc_scanbound.h): a
hypothesis that cannot reach mRansacMinInliers after segment A (the first kA = min(N, 128 PPT) points)
is not counted over segment B, and its stored count is its count over A.

Everything bit for bit against OraclePnP: ok, n_inliers, iterations, T and vbInliers of the result; the
parity hook's counts (rsc_pnp_last_hypotheses, which counts the round again with the bound off) against
check_inliers of every hypothesis' pose, and the poses against compute_pose of the hypothesis' sample.
The raw counts (rsc_pnp_last_counts_raw: what the round itself left) must be the exact count, or else
raw < exact < min_inliers and raw + (N - kA) < min_inliers; they are also compared with the rule's own
prediction (the count over A for a hypothesis the rule rejects).

Scenes are noise-free (synth.make_pnp_scene(noise=False)) with a chosen inlier set: the other points'
observations are moved at least 60 px away, so a sample of four inliers reproduces exactly that set
(unless its four-point EPnP solution is a mirror pose).  The seeds below put such samples where a case
wants them (found with the oracle; each case asserts what it relies on)."""
import dataclasses

import numpy as np
import pytest

from gpu_common import assert_pnp_equal, bits
import oracle_lib as ol
from rsc import synth
from test_gpu_scan_requalify import _f32, _zc

pytestmark = pytest.mark.gpu


def ppt_for(n):
    need, p = (n + 255) // 256, 1
    while p < need:
        p *= 2
    return p


def seg_a_points(n, ppt):
    return min(n, 128 * ppt) if ppt >= 2 else n


def make_scene(n, inliers, rs):
    """Noise-free scene of n correspondences whose inlier set is exactly `inliers` (bool [n])."""
    rng = np.random.default_rng(rs)
    sc = synth.make_pnp_scene(rng, n, 1.0, noise=False)
    out = ~np.asarray(inliers, bool)
    p2d = sc.p2d.copy()
    ang = rng.uniform(0, 2 * np.pi, n)
    r = rng.uniform(60.0, 300.0, n)
    p2d[out, 0] += (r * np.cos(ang))[out].astype(np.float32)
    p2d[out, 1] += (r * np.sin(ang))[out].astype(np.float32)
    return dataclasses.replace(sc, p2d=p2d, inlier_true=~out)


def split_inliers(n, ka, a, b, rs):
    """a inliers among the first ka points and b among the rest."""
    rng = np.random.default_rng(rs)
    m = np.zeros(n, bool)
    m[rng.choice(ka, a, replace=False)] = True
    if b:
        m[ka + rng.choice(n - ka, b, replace=False)] = True
    return m


def all_inlier_hyps(seed, sc, H):
    """Hypotheses of the first H of srand(seed)'s stream whose four samples are all inliers."""
    ss = ol.sample_stream(int(seed), sc.n, 4, H)
    return np.flatnonzero(sc.inlier_true[ss].all(1))


def same_floats(a, b):
    """Bit for bit, a NaN matching any NaN (sign and payload of a NaN are not part of the contract)."""
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def run_round(c, scenes, seeds, params, budget, round_n=None):
    """One iterate(budget) of the scenes' solvers in one round on context c, checked against the
    oracle.  Returns per solver (raw, exact, first-segment count, min_inliers, kA, oracle result)."""
    from rsc import engine
    budget = np.broadcast_to(np.asarray(budget, np.int32), (len(scenes),))
    params = params if isinstance(params, list) else [params] * len(scenes)
    gs = [engine.PnPSolver(c, sc, int(s)) for sc, s in zip(scenes, seeds)]
    for g, p in zip(gs, params):
        g.set_ransac_parameters(*p)
    if len(gs) == 1:
        got = [gs[0].iterate(int(budget[0]))]
    else:
        raw_res = engine.SolverBatch(gs).iterate_raw(budget)
        got = []
        for g, rec in zip(gs, raw_res):
            inl = g.last_inliers() if rec["ok"] else None
            got.append(dict(ok=bool(rec["ok"]), no_more=bool(rec["no_more"]), n_inliers=int(rec["n_inliers"]),
                            iterations=int(rec["iterations"]), T=np.array(rec["T"], np.float32).reshape(4, 4),
                            inliers=inl if inl is not None else np.zeros(0, bool)))
    ppt = ppt_for(round_n if round_n else max(sc.n for sc in scenes))
    # what the round itself left, of every solver, before the first hook call counts the round again
    raws = [g.last_counts_raw(4096) for g in gs]
    out = []
    for i, (g, sc, s, p) in enumerate(zip(gs, scenes, seeds, params)):
        where = f"solver {i} N={sc.n}"
        o = ol.OraclePnP(sc, int(s))
        o.set_ransac_parameters(*p)
        ro = o.iterate(int(budget[i]))
        assert_pnp_equal(got[i], ro, where)
        assert got[i]["iterations"] == ro["iterations"], f"{where} iterations"
        mi = o.info()["min_inliers"]
        raw = raws[i]
        cnt, pos = g.last_hypotheses(4096)
        cnt2, pos2 = g.last_hypotheses(4096)
        assert np.array_equal(cnt, cnt2) and same_floats(pos, pos2), f"{where} second hook call"
        smp = g.last_samples(4096)
        assert len(raw) == len(cnt) == len(smp) > 0, where
        ka = seg_a_points(sc.n, ppt)
        x = ol.OraclePnP(sc, int(s))
        x.set_ransac_parameters(*p)
        exact = np.zeros(len(cnt), np.int32)
        c1 = np.zeros(len(cnt), np.int32)
        # the hook shows the solver's LAST launch: after a failed Refine the rest of the round is
        # speculated again, with the EPnP rows the Refine left (Q6), which a fresh oracle does not have
        first_launch = len(cnt) == int(budget[i])
        for k in range(len(cnt)):
            if first_launch:
                R, t, _ = x.compute_pose(smp[k, :4])
                assert same_floats(np.concatenate([R.ravel(), t]), pos[k]), f"{where} pose {k}"
            n_in, mask = x.check_inliers(pos[k, :9].reshape(3, 3), pos[k, 9:], sc.n)
            exact[k], c1[k] = n_in, int(mask[:ka].sum())
        assert np.array_equal(cnt, exact), f"{where} hook counts\n{cnt}\n{exact}"
        out.append(dict(raw=raw, exact=exact, c1=c1, mi=mi, ka=ka, n=sc.n, ro=ro, g=g))
    return out


def check_raw(r, bound=True):
    """The raw counts of one solver's round against the rule."""
    raw, exact, c1, mi, rest = r["raw"], r["exact"], r["c1"], r["mi"], r["n"] - r["ka"]
    if not bound:
        assert np.array_equal(raw, exact), f"bound off: raw {raw} exact {exact}"
        return 0
    same = raw == exact
    cut = (raw < exact) & (exact < mi) & (raw + rest < mi)
    assert (same | cut).all(), f"raw {raw}\nexact {exact}\nmin_inliers {mi} rest {rest}"
    # the rule's own prediction: a hypothesis it rejects keeps its count over A
    reject = (rest > 0) & (c1 + rest < mi)
    assert np.array_equal(raw, np.where(reject, c1, exact)), f"raw {raw}\nmodel {np.where(reject, c1, exact)}"
    return int((raw < exact).sum())


def close(rs):
    for r in rs:
        r["g"].close()


@pytest.fixture(scope="module")
def own_ctx():
    from rsc import engine
    c = engine.Context(0)
    yield c
    c.close()


EPS5 = (0.99, 10, 1, 4, 0.5, 5.991)  # minInliers = max(10, N / 2); max iterations 1: the budget sets H


def _boundary(c, a, seed, budget):
    """N = 600 (PPT 4, kA = 512), minInliers 300: a inliers among the first 512 points, all 88 after."""
    sc = make_scene(600, split_inliers(600, 512, a, 88, 31), 32)
    rs = run_round(c, [sc], [seed], EPS5, budget)
    r = rs[0]
    assert r["mi"] == 300 and r["ka"] == 512 and len(r["raw"]) == budget
    # the hypothesis whose pose reproduces the inlier set (an all-inlier sample; a four-point EPnP
    # solution can also be a mirror pose with fewer inliers)
    ks = np.flatnonzero(r["exact"] == a + 88)
    assert len(ks) and ks[0] in all_inlier_hyps(seed, sc, budget), "no hypothesis reproduces the inlier set"
    k = int(ks[0])
    assert r["c1"][k] == a, r["c1"][k]
    n_cut = check_raw(r)
    return r, k, n_cut, rs


def test_boundary_passes_segment_a_without_slack(own_ctx):
    """212 + 88 = 300 = minInliers: 212 + (600 - 512) >= 300 holds with equality, the hypothesis is
    counted over B, qualifies, is adopted and refined.  (The Refine finds 300 inliers, which is not
    more than minInliers, so iterate() goes on; the qualifier is the budget's last hypothesis, so the
    launch the hook shows is the one it was counted in, and the result is the adopted hypothesis.)"""
    r, k, _, rs = _boundary(own_ctx, 212, 7001, 8)
    assert k == 7 and r["raw"][k] == 300 and r["ro"]["ok"] and r["ro"]["n_inliers"] == 300
    assert r["ro"]["inliers"].sum() == 300 and not (r["exact"][:k] >= 300).any()
    close(rs)


def test_boundary_one_short_is_rejected_after_a(own_ctx):
    """211 + 88 = 299: rejected after A (raw count 211), never qualifies."""
    r, k, n_cut, rs = _boundary(own_ctx, 211, 7001, 24)
    assert r["raw"][k] == 211 and r["exact"][k] == 299 and n_cut >= 1
    assert not r["ro"]["ok"] and not (r["exact"] >= 300).any()
    close(rs)


@pytest.mark.parametrize("n,ratio,seed", [(300, 0.6, 7010), (300, 0.4, 7011), (200, 0.6, 7012), (200, 0.4, 7013),
                                          (2000, 0.6, 7014), (2100, 0.6, 7017), (2100, 0.4, 7018)])
def test_sizes(own_ctx, n, ratio, seed):
    """PPT 2 (N = 300, kA = 256), PPT 1 (N = 200: no segments), PPT 8 (N = 2000), PPT 16 (N = 2100,
    kA = 2048, 52 points in B), with 60 % inliers (all-inlier samples qualify) and 40 % (none does)."""
    ppt = ppt_for(n)
    ka = seg_a_points(n, ppt)
    sc = make_scene(n, split_inliers(n, n, int(round(ratio * n)), 0, seed), seed + 100)
    rs = run_round(own_ctx, [sc], [seed], EPS5, 24)
    r = rs[0]
    assert r["ka"] == ka and r["mi"] == n // 2
    n_cut = check_raw(r)
    if ppt == 1:
        assert n_cut == 0
    assert r["ro"]["ok"] == (ratio > 0.5)
    close(rs)


def test_n2000_40_percent_cuts_hypotheses_short(own_ctx):
    """The headline's shape: N = 2000, 40 % inliers, minInliers 1000.  At least one hypothesis must show
    raw < exact, so the test cannot pass with the bound silently off; with the switch off raw == exact."""
    sc = make_scene(2000, split_inliers(2000, 2000, 800, 0, 41), 42)
    rs = run_round(own_ctx, [sc], [7015], EPS5, 40)
    assert rs[0]["ka"] == 1024 and rs[0]["mi"] == 1000
    assert check_raw(rs[0]) >= 1
    assert not rs[0]["ro"]["ok"]
    close(rs)
    own_ctx.set_scan_bound(False)
    try:
        rs = run_round(own_ctx, [sc], [7015], EPS5, 40)
        assert check_raw(rs[0], bound=False) == 0
        close(rs)
    finally:
        own_ctx.set_scan_bound(True)


def test_shared_ppt_leaves_a_small_problem_without_segment_b(own_ctx):
    """A round's PPT is its largest problem's: N = 200 beside N = 600 runs PPT 4 with kA = 200 = N, so
    B is empty, nothing continues and every count is exact although some reach minInliers."""
    big = make_scene(600, split_inliers(600, 512, 212, 88, 31), 32)
    small = make_scene(200, split_inliers(200, 200, 120, 0, 51), 52)
    rs = run_round(own_ctx, [big, small], [7001, 7020], EPS5, 24)
    assert rs[1]["ka"] == 200 and rs[1]["n"] == 200
    assert np.array_equal(rs[1]["raw"], rs[1]["exact"]) and (rs[1]["exact"] >= rs[1]["mi"]).any()
    for r in rs:
        check_raw(r)
    assert rs[0]["ro"]["ok"] and rs[1]["ro"]["ok"]
    close(rs)


def test_min_inliers_equal_to_n(own_ctx):
    """minInliers == N on an all-inlier scene: only a count of all N points qualifies, and
    c1 + (N - kA) >= N needs every point of A."""
    sc = make_scene(600, np.ones(600, bool), 61)
    rs = run_round(own_ctx, [sc], [7030], (0.99, 600, 1, 4, 0.5, 5.991), 16)
    assert rs[0]["mi"] == 600
    check_raw(rs[0])
    assert rs[0]["ro"]["ok"] and rs[0]["ro"]["n_inliers"] == 600
    close(rs)


def test_min_inliers_too_small_to_reject(own_ctx):
    """epsilon 0.02 with the floor 10: minInliers = 12 <= N - kA = 88, so nothing can be rejected."""
    sc = make_scene(600, split_inliers(600, 600, 240, 0, 71), 72)
    rs = run_round(own_ctx, [sc], [7040], (0.99, 10, 1, 4, 0.02, 5.991), 24)
    assert rs[0]["mi"] == 12
    assert check_raw(rs[0]) == 0 and np.array_equal(rs[0]["raw"], rs[0]["exact"])
    close(rs)


def _chunk_scene():
    return make_scene(600, split_inliers(600, 512, 230, 80, 81), 82)


@pytest.mark.parametrize("seed,want", [(7100, "rejected_before"), (7101, "later_chunk"), (7142, "two_in_chunk")])
def test_qualifier_positions_in_chunks(own_ctx, seed, want):
    """40 hypotheses = five scan chunks of 8: hypotheses rejected after A ahead of the chunk's first
    qualifier; the first qualifier in a later chunk than the first; two qualifiers in one chunk."""
    sc = _chunk_scene()
    rs = run_round(own_ctx, [sc], [seed], EPS5, 40)
    r = rs[0]
    check_raw(r)
    q = np.flatnonzero(r["exact"] >= r["mi"])
    assert len(q) and r["ro"]["ok"]
    k = int(q[0])
    rejected = (r["c1"] + (r["n"] - r["ka"]) < r["mi"])
    if want == "rejected_before":
        assert k % 8 >= 1 and rejected[k - k % 8:k].any()
    elif want == "later_chunk":
        assert k >= 8
    else:
        assert any(a // 8 == b // 8 for a, b in zip(q[:-1], q[1:]))
    close(rs)


def _many(c, n_solvers, budget):
    scenes = [make_scene(300, split_inliers(300, 300, 180 if i % 2 else 120, 0, 900 + i), 1000 + i) for i in range(n_solvers)]
    seeds = [7200 + i for i in range(n_solvers)]
    rs = run_round(c, scenes, seeds, EPS5, budget)
    cut = sum(check_raw(r) for r in rs)
    ok = sum(int(r["ro"]["ok"]) for r in rs)
    close(rs)
    return cut, ok


def test_argument_path_and_blob_path(own_ctx):
    """N = 300 (PPT 2): 8 solvers on the argument path, the same with the switch off (blob path), and
    more than 64 solvers (blob path whatever the switch); all fused rounds."""
    p0 = own_ctx.round_paths()
    cut, ok = _many(own_ctx, 8, 16)
    p1 = own_ctx.round_paths()
    assert p1["args"] > p0["args"] and ok >= 1
    own_ctx.set_round_args(False)
    try:
        assert _many(own_ctx, 8, 16) == (cut, ok)
    finally:
        own_ctx.set_round_args(True)
    p2 = own_ctx.round_paths()
    assert p2["blob"] > p1["blob"]
    _many(own_ctx, 66, 16)
    assert own_ctx.round_paths()["blob"] > p2["blob"]


def test_round_beyond_the_fused_limit(own_ctx):
    """66 solvers x 64 hypotheses = 4,224 > 4,096: no device-side selection, the host replay reads the
    counts and fetches the masks; the recount rewrites them for the hook."""
    cut, ok = _many(own_ctx, 66, 64)
    assert ok >= 1


def test_camera_plane_point_in_segment_b(own_ctx):
    """A point of segment B (index >= 512) on the camera plane of the first qualifying hypothesis'
    pose: that hypothesis survives A on the fast path and takes the IEEE redo in B only."""
    sc = _chunk_scene()
    seed, budget = 7100, 24
    o = ol.OraclePnP(sc, seed)
    o.set_ransac_parameters(*EPS5)
    ss = ol.sample_stream(seed, sc.n, 4, budget)
    k = R = t = None
    for k in range(budget):  # the first qualifying hypothesis
        R, t, _ = o.compute_pose(ss[k])
        if o.check_inliers(R, t, sc.n)[0] >= 300:
            break
    assert o.check_inliers(R, t, sc.n)[0] >= 300
    R = R.ravel()
    used = set(ss.ravel().tolist())
    i = next(j for j in range(512, sc.n) if not sc.inlier_true[j] and j not in used)
    z = _f32(-t[2] / R[8])
    cand, lo, hi = [z], z, z
    for _ in range(64):
        lo, hi = np.nextafter(lo, _f32(-np.inf)), np.nextafter(hi, _f32(np.inf))
        cand += [lo, hi]
    zs = [cz for cz in cand if _zc(R, t, (_f32(0), _f32(0), cz)) == 0.0]
    assert zs, "no float Z with fl(R8 Z) == -t2 near -t2 / R8"
    p3 = sc.p3dw.copy()
    p3[i] = (0.0, 0.0, zs[0])
    sc2 = dataclasses.replace(sc, p3dw=p3)
    rs = run_round(own_ctx, [sc2], [seed], EPS5, budget)
    r = rs[0]
    check_raw(r)
    assert r["exact"][k] >= r["mi"] and r["raw"][k] == r["exact"][k] and r["ro"]["ok"]
    assert _zc(R, t, p3[i]) == 0.0
    close(rs)


def test_nan_poses(own_ctx):
    """Exactly coplanar map points: the hypotheses' poses are NaN, every count is 0, nothing continues."""
    sc = synth.make_planar_pnp_scene(np.random.default_rng(91), 600, 0.6, "floor")
    rs = run_round(own_ctx, [sc], [7300], EPS5, 16)
    check_raw(rs[0])
    assert not rs[0]["ro"]["ok"]
    close(rs)


def test_iterate_after_the_hook(own_ctx):
    """The hook (twice) between two iterate() calls changes nothing: the second call's result is the
    oracle's, as it is without the hook."""
    from rsc import engine
    sc = make_scene(2000, split_inliers(2000, 2000, 800, 0, 41), 42)
    params = (0.99, 10, 300, 4, 0.5, 5.991)
    res = []
    for hook in (True, False):
        g = engine.PnPSolver(own_ctx, sc, 7400)
        g.set_ransac_parameters(*params)
        a = g.iterate(20)
        if hook:
            raw = g.last_counts_raw(64)
            c1, _ = g.last_hypotheses(64)
            c2, _ = g.last_hypotheses(64)
            assert np.array_equal(c1, c2) and (raw <= c1).all() and (raw < c1).any()
            assert np.array_equal(g.last_counts_raw(64), c1)  # recounted: the buffer now holds the full counts
        b = g.iterate(20)
        res.append((a, b, g.state()))
        g.close()
    o = ol.OraclePnP(sc, 7400)
    o.set_ransac_parameters(*params)
    oa, ob = o.iterate(20), o.iterate(20)
    for a, b, _ in res:
        assert_pnp_equal(a, oa, "first iterate")
        assert_pnp_equal(b, ob, "second iterate")
        assert a["iterations"] == oa["iterations"] and b["iterations"] == ob["iterations"]
    assert res[0][2] == res[1][2]


def test_hook_after_a_solver_of_the_round_is_closed(own_ctx):
    """The recount reads the correspondences of every solver of the round, which go with the solver:
    once one is closed, the hook on another launches nothing and reports an error for that round, the raw
    counts stay readable, and the next round is served as usual.  A round already recounted, and a round
    with the bound off, have nothing left to launch and are still served."""
    from rsc import engine
    params = (0.99, 10, 300, 4, 0.5, 5.991)
    scs = [make_scene(2000, split_inliers(2000, 2000, 800, 0, 41 + i), 42 + i) for i in range(2)]

    def full_counts(sc, seed, pos):
        x = ol.OraclePnP(sc, seed)
        x.set_ransac_parameters(*params)
        return np.array([x.check_inliers(p[:9].reshape(3, 3), p[9:], sc.n)[0] for p in pos], np.int32)

    def pair():
        gs = [engine.PnPSolver(own_ctx, sc, 7400 + i) for i, sc in enumerate(scs)]
        for g in gs:
            g.set_ransac_parameters(*params)
        engine.SolverBatch(gs).iterate_raw(np.array([20, 20], np.int32))
        return gs

    a, b = pair()
    raw = b.last_counts_raw(64)
    a.close()
    with pytest.raises(RuntimeError, match="destroyed"):
        b.last_hypotheses(64)
    with pytest.raises(RuntimeError, match="destroyed"):  # the round stays lost, it is not served raw later
        b.last_hypotheses(64)
    assert np.array_equal(b.last_counts_raw(64), raw)
    # the context's next round: the hook works again and is exact
    b.iterate(20)
    raw2 = b.last_counts_raw(64)
    cnt, pos = b.last_hypotheses(64)
    assert len(cnt) == 20 and np.array_equal(cnt, full_counts(scs[1], 7401, pos))
    assert (raw2 <= cnt).all()
    b.close()

    # recounted before the close: the buffer already holds the full counts
    a, b = pair()
    cnt, pos = b.last_hypotheses(64)
    a.close()
    cnt2, _ = b.last_hypotheses(64)
    assert np.array_equal(cnt, cnt2) and np.array_equal(cnt, full_counts(scs[1], 7401, pos))
    b.close()

    # bound off: every round's counts are full as they stand
    own_ctx.set_scan_bound(False)
    try:
        a, b = pair()
        a.close()
        cnt, pos = b.last_hypotheses(64)
        assert np.array_equal(cnt, full_counts(scs[1], 7401, pos))
        b.close()
    finally:
        own_ctx.set_scan_bound(True)
