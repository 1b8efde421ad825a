"""GPU: rsc_pose_optimization_many and rsc_optimize_sim3_many on the MI355X == the oracle on the
inputs of tests/lm_edge_cases.py — the exits of g2o's Levenberg-Marquardt loop that the frustum scenes
of test_gpu_poseopt.py / test_gpu_sim3opt.py never reach (an LDLT that is not positive with the stale
_x reused and tempChi = DBL_MAX, non-finite chi2, NaN rho, rho == 0, no active edge; the branch each
case takes is proved from the oracle's record in test_cpu_lm_edges.py), and the sizes where the
kernels change path (full last slab, chunk and slab boundaries, the 8192 limits and their rejection).

The contracts are those modules' check(): nGood / nIn, pose / g2oS12 bits, outlier / keep flags,
n_initial, n_correspondences, n_bad and the round, iteration and trial counts — with NaN compared as
NaN at equal positions (x86 produces the negative default NaN, gfx950 the positive one).  Every case
runs between two regular problems in one launch, which are checked too: a write past a neighbour's
flags or result record shows up there.  OptimizeSim3 runs in the one-workgroup form and in the
cooperative form with 1 and 7 helper workgroups per pair.

No case is filtered, skipped or expected to fail: the last test counts what ran against the lists."""
import functools

import numpy as np
import pytest

import lm_edge_cases as lc
import oracle_lib as ol
from gpu_common import ctx
from rsc import engine

pytestmark = pytest.mark.gpu

POSE_CASES = lc.pose_cases_c() + lc.pose_cases_d()
SIM3_CASES = lc.sim3_cases_c() + lc.sim3_cases_d()
SIM3_FORMS = (0, 1, 7)  # helper workgroups per pair (0: the one-workgroup form)
_ran = set()


def ids(cases):
    return [c.name for c in cases]


# the regular neighbours and their oracle results, computed once and shared
@functools.lru_cache(maxsize=None)
def pose_regular(k):
    f = lc.pose_regular(k)
    return f, ol.pose_optimization(f)


@functools.lru_cache(maxsize=None)
def sim3_regular(k):
    p = lc.sim3_regular(k)
    return p, ol.optimize_sim3(p)


_refs = {}


def pose_ref(f):
    """The oracle's result for a case, computed once (the Sim3 cases run in three forms)."""
    if id(f) not in _refs:
        _refs[id(f)] = ol.pose_optimization(f)
    return _refs[id(f)]


def sim3_ref(p):
    if id(p) not in _refs:
        _refs[id(p)] = ol.optimize_sim3(p)
    return _refs[id(p)]


def assert_pose(g, f, ref, where):
    """test_gpu_poseopt.check()'s contract for one Frame (ref = the oracle's result), NaN as NaN."""
    r, T, out, st = ref
    sel = f.has_mp == 1
    assert g["n_good"] == r, f"{where}: nGood {g['n_good']} vs {r}"
    assert g["n_initial"] == int(sel.sum()), where
    assert lc.nan_equal(g["Tcw"], T), f"{where}: Tcw\n{g['Tcw']}\n{T}"
    assert np.array_equal(g["outlier"][sel], out[sel]), f"{where}: outliers"
    assert (g["outlier"][~sel] == 255).all(), where
    if g["n_initial"] >= 3:
        got = [g["rounds"], g["lm_iterations"], g["lm_trials"]]
        assert got == list(st), f"{where}: stats {got} vs {list(st)}"


def assert_sim3(g, ref, where):
    """test_gpu_sim3opt.check()'s contract for one pair (ref = the oracle's result), NaN as NaN."""
    r, S, keep, st = ref
    assert g["n_inliers"] == r, f"{where}: nIn {g['n_inliers']} vs {r}"
    assert g["n_correspondences"] == st[0] and g["n_bad"] == st[1], f"{where}: {g['n_bad']} vs {st[1]}"
    assert lc.nan_equal(g["S"], S), f"{where}: S\n{g['S']}\n{S}"
    assert np.array_equal(g["keep"], keep), f"{where}: keep"
    if st[0]:
        got = [g["lm_iterations"], g["lm_trials"]]
        assert got == list(st[2:]), f"{where}: stats {got} vs {list(st[2:])}"


def run_pose_between_regulars(f, where):
    (f0, r0), (f1, r1) = pose_regular(0), pose_regular(1)
    res = engine.pose_optimization_many(ctx(), [f0, f, f1])
    assert_pose(res[1], f, pose_ref(f), where)
    assert_pose(res[0], f0, r0, f"{where}: regular frame before")
    assert_pose(res[2], f1, r1, f"{where}: regular frame after")


def run_sim3_between_regulars(c, p, where):
    (p0, r0), (p1, r1) = sim3_regular(0), sim3_regular(1)
    res = engine.optimize_sim3_many(c, [p0, p, p1])
    assert_sim3(res[1], sim3_ref(p), where)
    assert_sim3(res[0], r0, f"{where}: regular pair before")
    assert_sim3(res[2], r1, f"{where}: regular pair after")


@pytest.mark.parametrize("case", POSE_CASES, ids=ids(POSE_CASES))
def test_pose_case_between_regular_frames(case):
    _ran.add(("pose", case.name))
    run_pose_between_regulars(case.problem, case.name)


@pytest.fixture
def form_ctx():
    """The shared context in a given OptimizeSim3 form, restored to automatic afterwards."""
    c = ctx()
    yield c
    c.set_sim3opt_helpers(-1)


@pytest.mark.parametrize("helpers", SIM3_FORMS)
@pytest.mark.parametrize("case", SIM3_CASES, ids=ids(SIM3_CASES))
def test_sim3_case_between_regular_pairs(form_ctx, case, helpers):
    _ran.add(("sim3", case.name, helpers))
    form_ctx.set_sim3opt_helpers(helpers)
    run_sim3_between_regulars(form_ctx, case.problem, f"{case.name} ({helpers} helpers)")


def test_pose_more_than_8192_edges_is_rejected_and_the_context_stays_usable():
    """8193 map-point matches: RSC_ERR_UNSUPPORTED (-4), also from the middle of a batch; the next call
    on the same context is bit-exact."""
    big = lc.pose_over_limit()
    f0, r0 = pose_regular(0)
    for batch in ([big], [f0, big, f0]):
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            engine.pose_optimization_many(ctx(), batch)
    run_pose_between_regulars(POSE_CASES[0].problem, "after the rejection")


def test_sim3_more_than_8192_correspondences_is_rejected_and_the_context_stays_usable(form_ctx):
    big = lc.sim3_over_limit()
    p0, r0 = sim3_regular(0)
    for batch in ([big], [p0, big, p0]):
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            engine.optimize_sim3_many(form_ctx, batch)
    for helpers in (0, 7):
        form_ctx.set_sim3opt_helpers(helpers)
        run_sim3_between_regulars(form_ctx, SIM3_CASES[0].problem, f"after the rejection ({helpers} helpers)")


def test_every_listed_case_ran():
    """Run with the whole module: every case of the lists was launched on the device, in every form
    (a case is counted when its test starts; one that fails is reported by its own test)."""
    want = {("pose", c.name) for c in POSE_CASES} | {("sim3", c.name, h) for c in SIM3_CASES for h in SIM3_FORMS}
    assert len(POSE_CASES) == 50 and len(SIM3_CASES) == 19 and len(want) == 50 + 19 * len(SIM3_FORMS)
    assert _ran == want, sorted(want - _ran, key=str)
