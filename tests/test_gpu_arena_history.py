"""History independence of every entry point that stages through an arena or an LM staging pair: the
device buffers and their pinned mirrors only grow and are never cleared (rsc_arena.h: the scratch section is
"never copied"), so a kernel that read a word it had not written, or a host driver that read a mirror byte the
device had not written, would see what an earlier call left there; in the suite's fixed order that is usually
the same kernel's own sentinels.  Here every staging buffer is filled with a pattern between two runs of an entry
point's case set (rsc_diag_fill_staging / Context.fill_staging):

    0x00  claims, matches and counts read as 0, a legal index
    0x01  words read as 0x01010101, flags as 1
    0xFF  ints read as -1 (every "empty" sentinel), floats as NaN

and the run after the fill is compared, bit for bit, with the reference the entry point's own GPU test uses
(golden fixture, numpy restatement or oracle): that test's functions are called as they stand, so count words,
`rounds` and `track` records are part of the comparison.  Who initialises and who reads each scratch and output
piece of every arena is tabulated in DESIGN.md section 2.8.2 ("Initialisers of the staging pieces").

Then three sequences after a 0x01 fill: batches with an empty problem in the middle and all-empty batches (the
Fuse calls then skip the download: their outputs are the documented ones, not mirror bytes); A -> B -> A on the
shared arena with a smaller problem last; and the outputs documented as left untouched."""
import functools
import os
import types

import numpy as np
import pytest

import fusekf_cases as fkc
import kfproj_ref as kr
import lastproj_cases as lsc
import localproj_cases as lc
import mpupdate_cases as mc
import mpupdate_ref as mr
import stereo_cases as stc
import stereo_ref as sr
import test_gpu_bow_walk as g_bow
import test_gpu_bowvoc as g_voc
import test_gpu_create_map_points as g_cnmp
import test_gpu_frameproj as g_fp
import test_gpu_fusekf as g_fkf
import test_gpu_kfproj as g_kfp
import test_gpu_lastproj as g_last
import test_gpu_lm_edges as g_lm
import test_gpu_localproj as g_local
import test_gpu_mpupdate as g_mp
import test_gpu_poseopt as g_po
import test_gpu_sim3match_cases as g_s3m
import test_gpu_sim3opt as g_so
import test_gpu_stereo as g_st
import test_gpu_triang as g_tri
import triang_cases as tc
from gpu_common import ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = (0x00, 0x01, 0xFF)
_ran = set()


@functools.lru_cache(maxsize=None)
def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", f"{name}_traces.npz"))


# ---- what the fixtures of the entry points' own modules build, once ----
@functools.lru_cache(maxsize=None)
def mp_all_cases():
    cs = mc.cases()
    names = sorted(cs)
    p = g_mp.merge([cs[n][0] for n in names])
    return names, cs, p, g_mp.kviews(p.kfs)


@functools.lru_cache(maxsize=None)
def mp_random():
    p = mc.random_problem(mc.RANDOM_SEEDS["random_a"])
    return {"random_a": (p, g_mp.kviews(p.kfs))}


@functools.lru_cache(maxsize=None)
def fkf_randoms():
    return {name: fkc.random_problem(seed) for name, seed in fkc.RANDOM_SEEDS.items()}


@functools.lru_cache(maxsize=None)
def tri_problems():
    return tc.fixture_problems()


@functools.lru_cache(maxsize=None)
def st_randoms():
    return {name: (fr, sr.compute(fr)) for name, fr in stc.random_frames().items()}


# ---- one runner per entry point: its smallest existing case set against its own reference ----
def run_update_map_points():
    g_mp.test_hand_built_cases_one_call(mp_all_cases(), golden("mpupdate"), 3)
    g_mp.test_random_both_classes_one_call(mp_random(), golden("mpupdate"), "random_a", 3)


def run_projection_frame():
    g_fp.test_hand_built_cases_and_domino()
    g_fp.run_many([g_fp.fc.random_problem(20, 37, 50, 10, 100, n_clusters=2)], 10, 100, True)


def run_projection_kf():
    g_kfp.test_golden_problems_one_launch(golden("kfproj"))


def run_projection_last():
    g_last.test_golden_problems_one_launch_per_th(golden("lastproj"))


def run_local_points_fused():
    g_local.test_golden_problems_one_launch(golden("localproj"), True)


def run_local_points_matcher_only():
    g_local.test_golden_problems_one_launch(golden("localproj"), False)


def run_fuse_kf():
    g_fkf.test_golden_problems_one_launch(golden("fusekf"), fkf_randoms())


def run_fuse_sim3():
    g_kfp.test_fuse_batch(golden("kfproj"))


def run_triangulation():
    """rsc_search_for_triangulation_many and rsc_triangulate_pairs_many."""
    g_tri.test_golden_problems(golden("triang"), tri_problems())
    g_tri.test_pair_cases(golden("triang"))


def run_create_new_map_points():
    """The driver: the matcher in its speculative form (a problem with den_zero keeps its matches)."""
    g_cnmp.test_driver_cases()


def run_stereo():
    g_st.test_hand_built_cases_one_call(golden("stereo"))
    name = min(st_randoms(), key=lambda n: len(st_randoms()[n][0].kp) * len(st_randoms()[n][0].r_kp))
    fr, want = st_randoms()[name]
    _, res = g_st.run([fr], set_stereo=False)
    assert sr.same(res[0], want) == [] and sr.same(res[0], g_st.from_golden(golden("stereo"), name)) == [], name


def run_search_by_sim3():
    for group in g_s3m.GROUPS:
        g_s3m.test_group_parity(group)


def _bow(frame):
    n = 0
    for group in ("exact", "ori"):
        for b in g_bow.bc.batches(group):
            if b.frame == frame:
                n += int(g_bow.check_batch(b, 0.9, True)[1].sum())
    assert n > 100


def run_search_by_bow_frame():
    _bow(True)


def run_search_by_bow_kf():
    _bow(False)


def run_compute_bow():
    for n in (0, 1, 63, 64, 65):
        g_voc.test_basic_sizes(n)
    g_voc.test_batch_of_views()


def run_pose_optimization():
    for case in g_lm.POSE_CASES:
        g_lm.run_pose_between_regulars(case.problem, case.name)
    g_po.test_small_and_degenerate_frames()


def _optimize_sim3(helpers):
    c = ctx()
    c.set_sim3opt_helpers(helpers)
    try:
        for case in g_lm.SIM3_CASES:
            g_lm.run_sim3_between_regulars(c, case.problem, f"{case.name} ({helpers} helpers)")
        g_so.test_rules_and_degenerate_pairs()
    finally:
        c.set_sim3opt_helpers(-1)


def run_optimize_sim3_one_workgroup():
    _optimize_sim3(0)


def run_optimize_sim3_seven_helpers():
    _optimize_sim3(7)


ENTRY_POINTS = {
    "update_map_points": run_update_map_points,
    "projection_frame": run_projection_frame,
    "projection_kf": run_projection_kf,
    "projection_last": run_projection_last,
    "local_points_fused": run_local_points_fused,
    "local_points_matcher_only": run_local_points_matcher_only,
    "fuse_kf": run_fuse_kf,
    "fuse_sim3": run_fuse_sim3,
    "triangulation": run_triangulation,
    "create_new_map_points": run_create_new_map_points,
    "stereo": run_stereo,
    "search_by_sim3": run_search_by_sim3,
    "search_by_bow_frame": run_search_by_bow_frame,
    "search_by_bow_kf": run_search_by_bow_kf,
    "compute_bow": run_compute_bow,
    "pose_optimization": run_pose_optimization,
    "optimize_sim3_one_workgroup": run_optimize_sim3_one_workgroup,
    "optimize_sim3_seven_helpers": run_optimize_sim3_seven_helpers,
}


def fill(pattern):
    n = ctx().fill_staging(pattern)
    assert n > 0
    return n


@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda b: f"0x{b:02X}")
@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
def test_result_does_not_depend_on_what_the_staging_held(entry, pattern):
    run = ENTRY_POINTS[entry]
    run()  # the buffers have their capacity
    fill(pattern)
    run()
    _ran.add((entry, pattern))


def test_fill_reaches_every_buffer():
    """The filled byte count grows when an arena grows, repeats when nothing ran in between, and the pattern is
    checked (0..255)."""
    from rsc import engine
    run_stereo()
    run_compute_bow()
    a = fill(0x01)
    assert fill(0xFF) == a
    with pytest.raises(RuntimeError):
        ctx().fill_staging(256)
    with pytest.raises(RuntimeError):
        ctx().fill_staging(-1)
    fresh = engine.Context(0)
    assert fresh.fill_staging(0x01) == 0  # nothing allocated yet
    fresh.close()
    # the device side, read back: SearchBySim3's scratch (vnMatch1 / vnMatch2) holds the pattern after a fill
    th, cases = g_s3m.GROUPS["agree"]
    c = cases[0][1]
    s = engine.Sim3Search(ctx(), [(c.kf1, c.kf2, c.R12, c.t12, c.m12)], th)
    s.run()
    before = s.directions(0)
    fill(0x01)
    m1, m2 = s.directions(0)
    assert len(m1) and (m1 == 0x01010101).all() and (m2 == 0x01010101).all()
    s.run()
    assert all(np.array_equal(a, b) for a, b in zip(s.directions(0), before))
    run_stereo()  # and the calls work after the fills


# ---- sequences, each after a 0x01 fill ----
def _empty_points():
    return kr.points_of(state=[], pos=[], normal=[], dmax=[], dmin=[], desc=np.zeros((0, 32), np.uint8))


def test_empty_problem_in_the_middle_and_all_empty_batches():
    from rsc import engine
    z8 = np.zeros(0, np.uint8)
    # local-map matcher: zero points between two regular problems
    cs = lc.cases()
    a, b = cs["promoted"][0], cs["veto_lifted"][0]
    mid = types.SimpleNamespace(frame=a.frame, pts=_empty_points(), Tcw=a.Tcw, skip=z8, has_obs=z8, frame_occ=a.frame_occ,
                                cos_limit=a.cos_limit, th=a.th, nn_ratio=a.nn_ratio)
    fill(0x01)
    r = g_local.run_many([a, mid, b])
    for k, p in ((0, a), (2, b)):
        ref = lc.reference(p)
        assert np.array_equal(r["out"][k], ref["out"]) and r["track"][k].tobytes() == ref["track"].tobytes()
        assert (int(r["nmatches"][k]), int(r["n_to_match"][k]), int(r["rounds"][k])) == \
            (ref["nmatches"], ref["n_to_match"], ref["rounds"])
    assert (int(r["nmatches"][1]), int(r["n_to_match"][1]), int(r["rounds"][1])) == (0, 0, 1)
    assert (r["out"][1] == -1).all() and len(r["track"][1]) == 0
    # last-frame matcher: an empty LastFrame in the middle
    ls = lsc.cases()
    a, b = ls["greedy_promoted"][0], ls["two_claimers_kept"][0]
    mid = lsc.from_arrays_like(a, a.frame, lsc.last_of([], [], [], np.zeros((0, 3)), np.zeros((0, 32), np.uint8), []))
    fill(0x01)
    r = g_last.run_many([a, mid, b])
    for k, p in ((0, a), (2, b)):
        ref = lsc.reference(p)
        assert np.array_equal(r["out"][k], ref["out"])
        assert (int(r["nmatches"][k]), int(r["mode"][k]), int(r["rounds"][k])) == (ref["nmatches"], ref["mode"], ref["rounds"])
    assert int(r["nmatches"][1]) == 0 and int(r["rounds"][1]) == 1 and (r["out"][1] == -1).all()
    # stereo: a left frame with no feature and a right frame with no keypoint between the random frames
    fill(0x01)
    g_st.test_random_frames_one_call(golden("stereo"), st_randoms(), False)
    # KeyFrame Fuse: zero points between two cases, then nothing but empty point lists (no download)
    fc = fkc.cases()
    names = [n for n in sorted(fc) if fc[n][0].th == fkc.TH][:2]
    kvs = [g_fkf.kview(fc[n][0].kf) for n in names]
    mvs = [g_fkf.mview(fc[n][0].pts) for n in names]
    empty = g_fkf.mview(_empty_points())
    fill(0x01)
    best, nf = engine.fuse_kf_many(ctx(), [kvs[0], kvs[1], kvs[1]], [mvs[0], empty, mvs[1]],
                                   [fc[names[0]][0].skip, z8, fc[names[1]][0].skip], fkc.TH)
    assert best[0].tolist() == fc[names[0]][1] and best[2].tolist() == fc[names[1]][1]
    assert len(best[1]) == 0 and int(nf[1]) == 0
    assert [int(nf[0]), int(nf[2])] == [sum(x >= 0 for x in fc[n][1]) for n in names]
    fill(0x01)
    best, nf = engine.fuse_kf_many(ctx(), kvs, [empty, empty], [z8, z8], fkc.TH)
    assert [len(x) for x in best] == [0, 0] and [int(x) for x in nf] == [0, 0]
    # loop Fuse: an empty point view against two KeyFrames (no download)
    fill(0x01)
    best, nf = engine.fuse_sim3_many(ctx(), kvs, empty, [np.eye(4, dtype=np.float32)] * 2, [z8, z8], 3.0)
    assert [len(x) for x in best] == [0, 0] and [int(x) for x in nf] == [0, 0]
    # triangulation: no pair in the middle
    ps = tri_problems()
    g = golden("triang")
    names = [n for n in (str(s) for s in g["names"]) if ps[n][4] == 0][:3]
    r, pairs, st, x = g_tri.run_many([ps[n] for n in names])
    v1 = [g_tri.tg.views(ps[n][0])[1] for n in names]
    v2 = [g_tri.tg.views(ps[n][1])[1] for n in names]
    fill(0x01)
    st2, x2 = engine.triangulate_pairs_many(ctx(), v1, v2, [pairs[0], np.zeros((0, 2), np.int32), pairs[2]])
    assert len(st2[1]) == 0 and len(x2[1]) == 0
    for k in (0, 2):
        assert np.array_equal(st2[k], g[f"{names[k]}/status"])
        assert np.array_equal(x2[k].view(np.uint32), g[f"{names[k]}/x3d"].view(np.uint32))
    # MapPoint update: no point at all, then a point with an empty list
    cs = mc.cases()
    p = cs["ref_elsewhere"][0]
    kv = g_mp.kviews(p.kfs)
    none = types.SimpleNamespace(n_points=0, skip=[], pos=[], obs_begin=[0], obs_kf=[], obs_idx=[], kf_bad=None,
                                 ref_kf=[], ref_idx=[])
    fill(0x01)
    assert len(engine.update_map_points_many(ctx(), kv, none, 3)["updated"]) == 0
    e = types.SimpleNamespace(**vars(p.upd))
    e.obs_begin, e.obs_kf, e.obs_idx = np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    fill(0x01)
    r = engine.update_map_points_many(ctx(), kv, e, 3)
    assert r["updated"].tolist() == [0] and r["best_obs"].tolist() == [mr.FILL["best_obs"]]
    assert (r["desc"] == mr.FILL["desc"]).all()


def test_a_b_a_on_the_shared_arena():
    """The arena keeps the first call's layout in its bytes: a smaller problem of the same matcher afterwards, with
    another matcher's call in between, reads none of it."""
    fill(0x01)
    run_local_points_fused()          # 1,500 points, 600 features
    run_stereo()
    cs = lc.cases()
    names = [n for n in sorted(cs) if cs[n][0].th == 1.0]
    r = g_local.run_many([cs[n][0] for n in names])
    for k, n in enumerate(names):
        assert np.array_equal(r["out"][k], lc.expected_out(cs[n][0], cs[n][1])), n
        ref = lc.reference(cs[n][0])
        assert r["track"][k].tobytes() == ref["track"].tobytes(), n
        assert (int(r["nmatches"][k]), int(r["n_to_match"][k]), int(r["rounds"][k])) == \
            (ref["nmatches"], ref["n_to_match"], ref["rounds"]), n
    fill(0x01)
    run_triangulation()
    run_update_map_points()
    run_create_new_map_points()       # smaller than the fixture's problems
    run_triangulation()


def test_outputs_left_untouched_keep_the_callers_fill():
    from rsc import engine
    # MapPoint update: a skipped point, an empty list and the fields a call does not write keep ANY caller fill
    names, cs, p, kvs = mp_all_cases()
    n = p.upd.n_points
    fill(0x01)
    mine = g_mp.fresh_out(n)
    before = g_mp.fresh_out(n)
    got = engine.update_map_points_many(ctx(), kvs, p.upd, 3, out=mine)
    std = engine.update_map_points_many(ctx(), kvs, p.upd, 3)
    assert mr.same_result(std, mr.update(p, 3)) == ""
    untouched = 0
    for k in ("desc", "best_obs", "normal", "dmax", "dmin"):
        a, b, f = got[k][:n], std[k], before[k][:n]
        written = (a == b) | ((a != a) & (b != b))
        kept = (a == f) & (b == mr.FILL[k])
        assert (written | kept).all(), k
        untouched += int((kept & ~written).sum())
    assert untouched > 0 and np.array_equal(got["updated"][:n], std["updated"])
    assert (np.asarray(p.upd.skip) != 0).any()
    # the frustum records of the points that did not run: skipped, bad, behind the camera
    l = lc.cases()
    fill(0x01)
    sel = ["skipped_points", "z_negative", "bound_outside"]
    r = g_local.run_many([l[s][0] for s in sel])
    for k, s in enumerate(sel):
        assert r["track"][k]["in_view"].tolist() == l[s][1]["in_view"], s
        assert r["track"][k].tobytes() == lc.reference(l[s][0])["track"].tobytes(), s
    # the refusals leave the outputs as they were
    fill(0x01)
    g_mp.test_argument_errors(mp_all_cases())
    fill(0x01)
    g_st.test_argument_errors(st_randoms())


def test_every_listed_entry_point_ran_under_every_pattern():
    """Run with the whole module: each entry point of the list was run after each of the three fills (counted
    when its second run passed)."""
    want = {(e, b) for e in ENTRY_POINTS for b in PATTERNS}
    assert len(ENTRY_POINTS) == 18 and len(want) == 54
    assert _ran == want, sorted(want - _ran, key=str)
