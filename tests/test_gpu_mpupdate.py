"""MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth on the device (mpupdate.hip,
rsc_update_map_points_many) against the sequential restatement (tests/mpupdate_ref.py) and its golden fixture
(tests/golden/mpupdate_traces.npz), bit for bit (a NaN matches any NaN: mpupdate_ref.same_floats): every hand-built
case in one call, the random problems with both size classes and the 64 / 65 boundary in one call, for what = 1, 2
and 3; the argument checks; and the write-through into a resident MapPoint view."""
import copy
import os
import types

import numpy as np
import pytest

import fusekf_cases as fc
import mpupdate_cases as mc
import mpupdate_ref as mr
from gpu_common import ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("desc", "best_obs", "normal", "dmax", "dmin", "updated")
f32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "mpupdate_traces.npz"))


def kviews(kfs, triangulation=True):
    """KFViews of a problem's KeyFrames: the keypoint positions are drawn (the update reads none of them)."""
    from rsc import engine
    rng = np.random.default_rng(3)
    out = []
    for v in kfs:
        kp = np.stack([rng.uniform(2, 750, v.n), rng.uniform(2, 478, v.n)], 1).astype(f32)
        kf = fc.make_kf(kp, v.octave, v.desc, np.full(v.n, -1.0), Ow=v.Ow)
        kv = engine.KFView(ctx(), kf)
        if triangulation:
            kv.set_triangulation(kf)
        out.append(kv)
    return out


def merge(problems):
    """Several problems as one call: KeyFrame indices and observation offsets shifted."""
    kfs, parts, k0, o0 = [], [], 0, 0
    for p in problems:
        u = p.upd
        parts.append((u.skip, u.pos, u.obs_begin[1:] + o0, u.obs_kf + k0, u.obs_idx, u.kf_bad, u.ref_kf + k0, u.ref_idx))
        kfs += p.kfs
        k0 += len(p.kfs)
        o0 += int(u.obs_begin[-1])
    cat = lambda i, dt: np.concatenate([np.asarray(x[i], dt) for x in parts])
    upd = types.SimpleNamespace(n_points=sum(p.upd.n_points for p in problems), skip=cat(0, np.uint8), pos=cat(1, f32),
                                obs_begin=np.concatenate([[0], cat(2, np.int32)]).astype(np.int32),
                                obs_kf=cat(3, np.int32), obs_idx=cat(4, np.int32), kf_bad=cat(5, np.uint8),
                                ref_kf=cat(6, np.int32), ref_idx=cat(7, np.int32))
    return types.SimpleNamespace(kfs=kfs, upd=upd)


def cut(golden, name, what):
    r = {k: golden[f"{name}/{k}"].copy() for k in FIELDS}
    if not what & 1:
        r["desc"][:] = mr.FILL["desc"]
        r["best_obs"][:] = mr.FILL["best_obs"]
    if not what & 2:
        for k in ("normal", "dmax", "dmin"):
            r[k][:] = mr.FILL[k]
    r["updated"] &= what
    return r


@pytest.fixture(scope="module")
def all_cases():
    cs = mc.cases()
    names = sorted(cs)
    p = merge([cs[n][0] for n in names])
    assert p.upd.n_points <= 64
    return names, cs, p, kviews(p.kfs)


@pytest.mark.parametrize("what", [1, 2, 3])
def test_hand_built_cases_one_call(all_cases, golden, what):
    from rsc import engine
    names, cs, p, kvs = all_cases
    got = engine.update_map_points_many(ctx(), kvs, p.upd, what)
    assert mr.same_result(got, mr.update(p, what)) == ""
    at = 0
    for n in names:  # each case against the fixture, and for what = 3 against the answers worked out by hand
        m = cs[n][0].upd.n_points
        part = {k: got[k][at:at + m] for k in FIELDS}
        assert mr.same_result(part, cut(golden, n, what)) == "", n
        if what == 3:
            exp = cs[n][1]
            assert part["best_obs"].tolist() == [mr.FILL["best_obs"] if b is None else b for b in exp["best_obs"]], n
            for i, a in enumerate(exp["desc"]):
                assert np.array_equal(part["desc"][i], np.full(32, mr.FILL["desc"], np.uint8) if a is None else mc.bits(a))
            for k in ("normal", "dmax", "dmin"):
                if k in exp:
                    assert mr.same_floats(part[k], np.array(exp[k], f32)), (n, k)
            if "nan_normal" in exp:
                assert np.isnan(part["normal"]).all(axis=1).tolist() == exp["nan_normal"]
        at += m


@pytest.fixture(scope="module")
def randoms():
    ps = {name: mc.random_problem(seed) for name, seed in mc.RANDOM_SEEDS.items()}
    return {name: (p, kviews(p.kfs)) for name, p in ps.items()}


@pytest.mark.parametrize("what", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(mc.RANDOM_SEEDS))
def test_random_both_classes_one_call(randoms, golden, name, what):
    """Lists of 1, 2, 3, 63, 64 | 65, 200 and 1,024 observations in one call (12 points, four KeyFrames of 1,100)."""
    from rsc import engine
    p, kvs = randoms[name]
    assert np.array_equal(p.upd.obs_idx, golden[f"{name}/obs_idx"]) and p.upd.n_points <= 64
    assert np.diff(p.upd.obs_begin).tolist()[:8] == [1, 2, 3, 63, 64, 65, 200, 1024]
    got = engine.update_map_points_many(ctx(), kvs, p.upd, what)
    assert mr.same_result(got, cut(golden, name, what)) == ""


def test_timing_reports_the_kernels(randoms):
    from rsc import engine
    p, kvs = randoms["random_a"]
    c = ctx()
    c.enable_timing(True)
    try:
        engine.update_map_points_many(c, kvs, p.upd, 3)
        assert c.last_timing()["refine_ms"] > 0.0
    finally:
        c.enable_timing(False)


def fresh_out(n):
    F = mr.FILL
    return dict(desc=np.full((n, 32), 0x5C, np.uint8), best_obs=np.full(n, -31, np.int32),
                normal=np.full((n, 3), 9.5, f32), dmax=np.full(n, 9.5, f32), dmin=np.full(n, 9.5, f32),
                updated=np.full(n, 0x77, np.uint8))


def test_argument_errors(all_cases):
    """Every refusal returns before a launch and leaves the outputs as they were; the context stays usable."""
    from rsc import engine
    cs = mc.cases()
    p = cs["ref_elsewhere"][0]  # two KeyFrames of two keypoints, one point with two observations
    kvs = kviews(p.kfs)
    good = engine.update_map_points_many(ctx(), kvs, p.upd, 3)
    assert good["best_obs"].tolist() == [0] and good["updated"].tolist() == [3]

    def refused(upd=p.upd, views=kvs, what=3, dst=None, dst_index=None):
        out, before = fresh_out(upd.n_points), fresh_out(upd.n_points)
        with pytest.raises(RuntimeError):
            engine.update_map_points_many(ctx(), views, upd, what, dst, dst_index, out=out)
        for k in out:
            assert np.array_equal(out[k], before[k]), k

    def edited(**kw):
        u = copy.copy(p.upd)
        for k, v in kw.items():
            setattr(u, k, np.asarray(v, getattr(p.upd, k).dtype))
        return u

    for what in (0, 4, -1, 7):
        refused(what=what)
    refused(edited(obs_kf=[0, 2]))
    refused(edited(obs_kf=[-1, 1]))
    refused(edited(obs_idx=[0, 2]))
    refused(edited(obs_idx=[-1, 0]))
    refused(edited(ref_kf=[2]))
    refused(edited(ref_kf=[-1]))
    refused(edited(ref_idx=[2]))
    refused(edited(ref_idx=[-1]))
    refused(edited(obs_begin=[0, -1]))
    refused(edited(obs_begin=[1, 0]))
    # a list of 1,025 observations; 1,024 is served (tests/test_cpu_mpupdate.py runs it through the emulation)
    long = edited(obs_begin=[0, 1025], obs_kf=[0] * 1025, obs_idx=[0] * 1025)
    refused(long)
    long.skip = np.ones(1, np.uint8)  # the list of a skipped point is not read
    assert engine.update_map_points_many(ctx(), kvs, long, 3)["updated"].tolist() == [0]
    # what & 2 needs the camera centre: a view without rsc_kfview_set_triangulation is refused, what = 1 is served
    bare = kviews(p.kfs, triangulation=False)
    refused(views=[kvs[0], bare[1]])
    refused(views=[bare[0], kvs[1]], what=2)
    assert engine.update_map_points_many(ctx(), bare, p.upd, 1)["updated"].tolist() == [1]
    # octave[ref_idx] outside [0, n_levels): the index of mvScaleFactors
    for octave in (8, -1):
        q = copy.deepcopy(p)
        q.kfs[1].octave = np.array([1, octave], np.int32)
        refused(q.upd, kviews(q.kfs))
        assert engine.update_map_points_many(ctx(), kviews(q.kfs), q.upd, 1)["updated"].tolist() == [1]
    # dst: a slot out of range, one slot named twice, a view of another context
    two = merge([p, p])
    kv2 = kvs + kvs
    pts = types.SimpleNamespace(n=3, state=np.ones(3, np.uint8), pos=np.zeros((3, 3), f32), normal=np.zeros((3, 3), f32),
                                dmax=np.ones(3, f32), dmin=np.ones(3, f32), desc=np.zeros((3, 32), np.uint8))
    dst = engine.MPView(ctx(), pts)
    for idx in ([0, 3], [-2, 0], [1, 1]):
        refused(two.upd, kv2, dst=dst, dst_index=idx)
    other = engine.Context(0)
    refused(two.upd, kv2, dst=engine.MPView(other, pts), dst_index=[0, 1])
    back = dst.download()
    assert not back.desc.any() and not back.normal.any()  # the refused calls wrote nothing into the view
    # RSC_OK: no points, and nothing but empty lists
    none = types.SimpleNamespace(n_points=0, skip=[], pos=[], obs_begin=[0], obs_kf=[], obs_idx=[], kf_bad=None,
                                 ref_kf=[], ref_idx=[])
    assert len(engine.update_map_points_many(ctx(), kvs, none, 3)["updated"]) == 0
    empty = edited(obs_begin=[0, 0], obs_kf=[], obs_idx=[])
    r = engine.update_map_points_many(ctx(), kvs, empty, 3)
    assert r["updated"].tolist() == [0] and r["best_obs"].tolist() == [mr.FILL["best_obs"]]
    again = engine.update_map_points_many(ctx(), kvs, p.upd, 3)
    assert mr.same_result(again, good) == ""


@pytest.fixture(scope="module")
def fuse_scene():
    """The first random problem of the Fuse tests (1,500 points, three KeyFrames of 600) with an update problem on
    40 of the points its first KeyFrame matches: each observes a keypoint in every one of the three KeyFrames."""
    pts, kfs, skips = fc.random_problem(fc.RANDOM_SEEDS["random_a"])
    rng = np.random.default_rng(9)
    fused = np.load(os.path.join(ROOT, "tests", "golden", "fusekf_traces.npz"))["random_a/0/best_idx"]
    sel = np.sort(rng.choice(np.nonzero(fused >= 0)[0], 40, replace=False))  # points the first KeyFrame matches
    b = mc.Builder()
    b.kfs = [types.SimpleNamespace(n=k.n, desc=np.asarray(k.desc, np.uint8), octave=np.asarray(k.octave, np.int32),
                                   scale=mc.SF, Ow=np.asarray(k.Ow, f32), bad=False) for k in kfs]
    for i in sel:
        obs = [(k, int(rng.integers(0, kfs[k].n))) for k in rng.permutation(3)]
        b.point(pts.pos[i], obs, ref=obs[int(rng.integers(0, 3))])
    return pts, kfs, skips, sel, b.problem()


def test_dst_view_receives_the_fields(fuse_scene):
    """What the call writes lands in the resident view's slots as well; other slots, slots of points with
    dst_index = -1 and fields the call does not write keep their bytes."""
    from rsc import engine
    pts, kfs, skips, sel, p = fuse_scene
    kvs = []
    for kf in kfs:
        kv = engine.KFView(ctx(), kf)
        kv.set_triangulation(kf)
        kvs.append(kv)
    want = mr.update(p, 3)
    assert (want["updated"] == 3).all()
    idx = sel.astype(np.int32)
    idx[::5] = -1  # every fifth point stays out of the view
    for what in (1, 2, 3):
        dst = engine.MPView(ctx(), pts)
        got = engine.update_map_points_many(ctx(), kvs, p.upd, what, dst, idx)
        exp = mr.update(p, what)
        assert mr.same_result(got, exp) == ""
        back = dst.download()
        model = {k: np.array(getattr(pts, k), copy=True) for k in ("state", "pos", "normal", "dmax", "dmin", "desc")}
        for j, s in enumerate(idx):
            if s < 0:
                continue
            if what & 1:
                model["desc"][s] = exp["desc"][j]
            if what & 2:
                model["normal"][s], model["dmax"][s], model["dmin"][s] = exp["normal"][j], exp["dmax"][j], exp["dmin"][j]
        for k, a in model.items():
            assert np.array_equal(np.ascontiguousarray(getattr(back, k)).view(np.uint8),
                                  np.ascontiguousarray(a).view(np.uint8)), (what, k)
        changed = [s for s in idx if s >= 0]
        assert not np.array_equal(back.desc[changed], pts.desc[changed]) or not what & 1
    # Fuse on the updated view and on a fresh view uploaded from the host outputs: the same best_idx
    dst = engine.MPView(ctx(), pts)
    got = engine.update_map_points_many(ctx(), kvs, p.upd, 3, dst, sel.astype(np.int32))
    host = copy.copy(pts)
    for k in ("desc", "normal", "dmax", "dmin"):
        a = np.array(getattr(pts, k), copy=True)
        a[sel] = got[k]
        setattr(host, k, a)
    fresh = engine.MPView(ctx(), host)
    best_dst, _ = engine.fuse_kf_many(ctx(), kvs, [dst] * 3, skips, fc.TH)
    best_new, _ = engine.fuse_kf_many(ctx(), kvs, [fresh] * 3, skips, fc.TH)
    best_old, _ = engine.fuse_kf_many(ctx(), kvs, [engine.MPView(ctx(), pts)] * 3, skips, fc.TH)
    for c in range(3):
        assert np.array_equal(best_dst[c], best_new[c]), c
    assert any(not np.array_equal(a, b) for a, b in zip(best_dst, best_old))  # the update shows in the matcher
