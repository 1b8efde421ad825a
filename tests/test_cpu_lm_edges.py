"""CPU: the failure branches and size limits of the two Levenberg-Marquardt optimisers
(Optimizer::PoseOptimization, Optimizer::OptimizeSim3) on the inputs of tests/lm_edge_cases.py.

* The oracle (oracle/poseopt_oracle.cpp, oracle/sim3opt_oracle.cpp) equals the host build of the
  device orchestration (tests/hostemu) bit for bit on every case, NaN compared as NaN at equal
  positions.
* The oracle's LM branch record (oracle/lm_branches.h) shows that each case takes the branch it is
  named for, and that the set as a whole takes every exit of g2o's solve(): an LDLT that is not
  positive, a non-finite tempChi, NaN rho, qmax == 10, rho == 0, nBadLM >= 3, an optimize() call
  without an active edge.  The record itself changes no result.
* A few hand-worked expectations that follow from the reference text (they pin what the reference
  does with such inputs, not what one would like it to do).

tests/test_gpu_lm_edges.py runs the same cases on the device."""
import numpy as np
import pytest

import hostemu_lib as hl
import lm_edge_cases as lc
import oracle_lib as ol

POSE_C, POSE_D = lc.pose_cases_c(), lc.pose_cases_d()
SIM3_C, SIM3_D = lc.sim3_cases_c(), lc.sim3_cases_d()
_results = {}  # (optimiser, case name) -> the oracle's result with its branch record, computed once


def pose_result(case):
    if ("pose", case.name) not in _results:
        _results["pose", case.name] = ol.pose_optimization_branches(case.problem)
    return _results["pose", case.name]


def sim3_result(case):
    if ("sim3", case.name) not in _results:
        _results["sim3", case.name] = ol.optimize_sim3_branches(case.problem)
    return _results["sim3", case.name]


def ids(cases):
    return [c.name for c in cases]


def assert_pose_equal(a, b, f, where):
    """Oracle result a == host-build result b of Frame f (hostemu_lib lists the edges' flags only)."""
    sel = np.nonzero(f.has_mp)[0]
    assert a[0] == b[0], f"{where}: nGood {a[0]} vs {b[0]}"
    assert lc.nan_equal(a[1], b[1]), f"{where}: Tcw\n{a[1]}\n{b[1]}"
    assert np.array_equal(a[2][sel], b[2]), f"{where}: outliers"
    assert np.array_equal(a[3], b[3]), f"{where}: stats {a[3]} vs {b[3]}"


def assert_sim3_equal(a, b, where):
    assert a[0] == b[0], f"{where}: nIn {a[0]} vs {b[0]}"
    assert lc.nan_equal(a[1], b[1]), f"{where}: S\n{a[1]}\n{b[1]}"
    assert np.array_equal(a[2], b[2]), f"{where}: keep"
    assert list(a[3][1:]) == list(b[3][1:]), f"{where}: stats {a[3]} vs {b[3]}"


@pytest.mark.parametrize("case", POSE_C + POSE_D, ids=ids(POSE_C + POSE_D))
def test_pose_oracle_equals_host_build_and_takes_its_branch(case):
    f = case.problem
    r, T, out, st, br = pose_result(case)
    assert_pose_equal((r, T, out, st), hl.pose_optimization(f), f, case.name)
    # the record only counts: the plain entry point returns the same bits
    plain = ol.pose_optimization(f)
    assert plain[0] == r and lc.nan_equal(plain[1], T) and np.array_equal(plain[2], out)
    assert np.array_equal(plain[3], st) and br["trials"] == st[2]
    for k in case.expect:
        assert br[k] > 0, f"{case.name}: branch '{k}' not taken: {br}"


@pytest.mark.parametrize("case", SIM3_C + SIM3_D, ids=ids(SIM3_C + SIM3_D))
def test_sim3_oracle_equals_host_build_and_takes_its_branch(case):
    p = case.problem
    r, S, keep, st, br = sim3_result(case)
    assert_sim3_equal((r, S, keep, st), hl.optimize_sim3(p), case.name)
    plain = ol.optimize_sim3(p)
    assert plain[0] == r and lc.nan_equal(plain[1], S) and np.array_equal(plain[2], keep)
    assert np.array_equal(plain[3], st) and br["trials"] == st[3]
    for k in case.expect:
        assert br[k] > 0, f"{case.name}: branch '{k}' not taken: {br}"


def test_regular_neighbours_of_the_mixed_batches():
    """The regular problems the GPU module launches around each case: oracle == host build."""
    for k in range(2):
        f = lc.pose_regular(k)
        assert_pose_equal(ol.pose_optimization(f), hl.pose_optimization(f), f, f"regular frame {k}")
        p = lc.sim3_regular(k)
        assert_sim3_equal(ol.optimize_sim3(p), hl.optimize_sim3(p), f"regular pair {k}")


# ---- hand-worked expectations ---------------------------------------------------------------------
def clean_frame(seed, stereo, n=lc.N_SLOTS):
    """Exact observations of the true pose, which is also the initial pose: every edge an inlier."""
    f = lc.pose_base(seed, stereo, n, ratio=1.0, rot_noise=0.0, trans_noise=0.0, noise=False)
    f.Tcw[:3, :3] = f.R_true.astype(np.float32)
    f.Tcw[:3, 3] = f.t_true.astype(np.float32)
    return f


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
@pytest.mark.parametrize("edit", ["xw_nan", "uv_nan"])
def test_one_nan_edge_freezes_the_pose_and_flags_nothing(edit, stereo):
    """One NaN edge makes activeRobustChi2 NaN in every pass.  solve() then has rho = NaN: `rho > 0`
    is false, so the trial is popped; `rho < 0` is false, so the trial loop ends after one trial;
    qmax == 1 and `rho == 0` is false, so no Terminate; `(iniChi - currentChi) * 1e3 < iniChi` is false,
    so nBadLM stays 0 (optimization_algorithm_levenberg.cpp:90-147).  Every round therefore runs its 10
    iterations of 1 trial at the initial estimate, the pose returned is the input pose, and the NaN
    edge itself is no outlier because `chi2 > 5.991` is false for NaN (Optimizer.cpp:357)."""
    f = clean_frame(3300, stereo)
    lc.POSE_EDITS[edit](f)
    r, T, out, st = ol.pose_optimization(f)
    assert r == f.n
    assert np.array_equal(T.view(np.uint32), f.Tcw.view(np.uint32))
    assert not out.any() and out[lc.K] == 0
    assert list(st) == [4, 40, 40]
    r2, T2, out2, st2 = hl.pose_optimization(f)
    assert r2 == f.n and np.array_equal(T2.view(np.uint32), f.Tcw.view(np.uint32)) and list(st2) == [4, 40, 40]


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_zero_information_one_iteration_per_round(stereo):
    """inv_sigma2 == 0: H = 0 and b = 0, computeLambdaInit gives lambda = 0, the LDLT of the zero
    matrix is `positive` with x = 0, tempChi == currentChi == 0 and rho = 0 / 1e-3 = 0: solve() returns
    Terminate after its first trial (`rho == 0`, optimization_algorithm_levenberg.cpp:143), in each of
    the four rounds.  chi2 = 0 for every edge: nothing is an outlier and the pose is the input pose."""
    f = lc.pose_base(3301, stereo)
    lc.po_inv_zero(f)
    r, T, out, st, br = ol.pose_optimization_branches(f)
    assert list(st) == [4, 4, 4] and r == f.n and not out.any()
    assert br["end_rho0"] == 4 and br["rejected"] == 4 and br["not_ok2"] == 0
    assert np.abs(T - f.Tcw).max() < 1e-6  # the quaternion round trip of the float pose


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_nan_pose_in_gives_nan_pose_out(stereo):
    """NaN in Tcw: Converter::toSE3Quat's quaternion is NaN, no trial is ever accepted, and the pose
    written back is that NaN estimate; no edge is an outlier (NaN chi2)."""
    f = lc.pose_base(3302, stereo)
    lc.po_tcw_nan(f)
    r, T, out, st = ol.pose_optimization(f)
    assert np.isnan(T[:3, :3]).any() and r == f.n and not out.any()
    assert list(st) == [4, 40, 40]
    assert list(T[3]) == [0.0, 0.0, 0.0, 1.0]


def test_sim3_all_outliers_returns_zero_untouched():
    """Every e12 edge 500 px off: all correspondences are removed after optimize(5), fewer than 10
    stay, OptimizeSim3 returns 0 before the second optimize() and leaves g2oS12 as it came
    (Optimizer.cpp:1201-1202)."""
    p = lc.sim3_base(4300)
    lc.so_shift_500(p)
    r, S, keep, st = ol.optimize_sim3(p)
    assert r == 0 and np.array_equal(S, p.S0) and st[1] == st[0] == int(p.valid.sum())
    assert not keep[p.valid == 1].any() and keep[p.valid == 0].all()


def test_sim3_zero_information_one_iteration_per_optimize():
    """inv1 = inv2 = 0: as PoseOptimization's, one trial and Terminate (rho == 0) in each of the two
    optimize() calls; chi2 = 0 everywhere, so every correspondence stays."""
    p = lc.sim3_base(4301)
    lc.so_inv_zero(p)
    r, S, keep, st, br = ol.optimize_sim3_branches(p)
    assert list(st[1:]) == [0, 2, 2] and r == st[0] and keep.all()
    assert br["end_rho0"] == 2 and np.array_equal(S, p.S0)


def test_sim3_nan_estimate_in_stays():
    """NaN in g2oS12's translation: no trial is accepted (NaN rho), the estimate returned is the NaN
    one given, and no correspondence is removed (NaN chi2 compares false against th2)."""
    p = lc.sim3_base(4302)
    lc.so_s0_t_nan(p)
    r, S, keep, st = ol.optimize_sim3(p)
    assert r == st[0] and st[1] == 0 and keep.all() and list(st[2:]) == [10, 10]
    assert lc.nan_equal(S, p.S0)


# ---- coverage of the branches ---------------------------------------------------------------------
def _sum(opt, field):
    if opt == "pose":
        return sum(pose_result(c)[4][field] for c in POSE_C + POSE_D)
    return sum(sim3_result(c)[4][field] for c in SIM3_C + SIM3_D)


def test_every_branch_is_taken_somewhere():
    """Each counter of the record is non-zero over the set; the LDLT failure, the non-finite tempChi
    and the optimize() call without an active edge are reached for both optimisers."""
    for field in ol.LM_BRANCH_FIELDS:
        assert _sum("pose", field) + _sum("sim3", field) > 0, field
    for opt in ("pose", "sim3"):
        for field in ("not_ok2", "tempchi_nonfinite", "no_active_edge"):
            assert _sum(opt, field) > 0, (opt, field)


def test_case_lists_are_complete():
    """The lists hold what they are meant to: every PoseOptimization case in both forms, the sizes."""
    assert len(POSE_C) == 2 * len(lc.POSE_EDITS) == 40 and len(SIM3_C) == len(lc.SIM3_EDITS) == 12
    assert [int(c.problem.has_mp.sum()) for c in POSE_D] == list(lc.POSE_SIZES) + [8192]
    assert POSE_D[-1].problem.n > 8192
    assert [int(c.problem.valid.sum()) for c in SIM3_D] == list(lc.SIM3_SIZES)
    assert int(lc.pose_over_limit().has_mp.sum()) == 8193 and int(lc.sim3_over_limit().valid.sum()) == 8193
    for c in POSE_C:
        stereo = c.problem.u_right is not None and bool((c.problem.u_right >= 0).any())
        assert stereo == c.name.endswith("-stereo"), c.name
    for c in POSE_D:
        ur = c.problem.u_right[c.problem.has_mp == 1]
        assert c.problem.n < 10 or ((ur >= 0).any() and (ur < 0).any()), c.name  # mono and stereo mixed
