"""TEST-ONLY: named, seeded inputs that drive Optimizer::PoseOptimization and Optimizer::OptimizeSim3
through the exits of g2o's Levenberg-Marquardt loop that rsc/synth.py's frustum scenes never reach
(an LDLT that is not positive, non-finite chi2, NaN rho, no active edge), and through the sizes where
the kernels change path (the 256-edge slab of poseopt.hip, the 64-edge chunk and 192-edge slab of
sim3opt.hip, the 8192 limits of rsc_optim.cpp).  Shared by tests/test_cpu_lm_edges.py (oracle == host
build, branch record) and tests/test_gpu_lm_edges.py (device == oracle).

Every case is a rsc.synth frame / problem with fields edited; nothing here is an output of the oracle.
A case names the counters of the oracle's LM branch record (oracle/lm_branches.h,
oracle_lib.LM_BRANCH_FIELDS) that it must make non-zero: `expect`, fixed by reasoning from the
reference's control flow (the comment of each case), not read off a run.

Case list C: about 120 slots, so the 4 rounds and the `< 10 edges` rule behave as in a real Frame.
Case list D: sizes."""
from __future__ import annotations

import dataclasses

import numpy as np

from rsc import synth

N_SLOTS = 120
NAN, INF = np.float32(np.nan), np.float32(np.inf)


@dataclasses.dataclass
class Case:
    name: str
    problem: object          # rsc.synth.PoseOptFrame or rsc.synth.Sim3OptProblem
    expect: tuple = ()       # LM branch counters the oracle must report non-zero for this input


# ---- Optimizer::PoseOptimization ------------------------------------------------------------------
def pose_base(seed: int, stereo: bool, n: int = N_SLOTS, **kw):
    """A regular Frame: 80 % inliers, a RANSAC-like initial pose; stereo: 80 % stereo slots."""
    return synth.make_poseopt_frame(np.random.default_rng(seed), n, kw.pop("ratio", 0.8),
                                    stereo_frac=0.8 if stereo else 0.0, **kw)


def _to_camera_frame(f):
    """Tcw = I: the map points expressed in the true camera frame, so the scene stays the same."""
    Xc = f.Xw.astype(np.float64) @ f.R_true.T + f.t_true
    f.Xw = Xc.astype(np.float32)
    f.Tcw = np.eye(4, dtype=np.float32)


def _set_camera_point(f, i, pc):
    """Slot i's map point placed at pc in the camera frame of the initial pose f.Tcw."""
    R, t = f.Tcw[:3, :3].astype(np.float64), f.Tcw[:3, 3].astype(np.float64)
    f.Xw[i] = ((np.asarray(pc, np.float64) - t) @ R).astype(np.float32)


def _camera_point(f, i):
    R, t = f.Tcw[:3, :3].astype(np.float64), f.Tcw[:3, 3].astype(np.float64)
    return R @ f.Xw[i].astype(np.float64) + t


# Each edit takes a regular frame and makes it the case.  K = the slot edited by the one-edge cases.
K = 7


def po_xw_nan(f):
    # chi2 of edge K is NaN in every pass: activeRobustChi2, H and b are NaN, so currentChi, tempChi
    # and rho are NaN; `rho > 0` and `rho < 0` are false: one rejected trial per iteration, no Terminate
    f.Xw[K, 1] = NAN


def po_xw_inf(f):
    # map(+Inf) has Inf - Inf = NaN components (the quaternion rotation sums products of both signs)
    f.Xw[K] = INF


def po_uv_nan(f):
    f.uv[K, 0] = NAN


def po_identity_one_z0(f):
    # p = (x, y, 0): x / 0 = +-Inf, the error and chi2 are Inf, sqrt(Inf) = Inf in the Huber kernel;
    # currentChi and tempChi are both Inf (or NaN once Inf meets 0 * Inf in H), so rho = Inf - Inf = NaN
    _to_camera_frame(f)
    f.Xw[K, 2] = 0.0


def po_identity_one_origin(f):
    # p = (0, 0, 0): 0 / 0 = NaN
    _to_camera_frame(f)
    f.Xw[K] = 0.0


def po_identity_all_z0(f):
    _to_camera_frame(f)
    f.Xw[:, 2] = 0.0


def po_tcw_nan(f):
    # a NaN rotation entry: the initial quaternion is NaN, every error is NaN, the pose out is NaN
    f.Tcw[1, 2] = NAN


def po_behind_camera(f):
    # z < 0: a finite edge with a mirrored projection (the reference has no cheirality test here)
    pc = _camera_point(f, K)
    _set_camera_point(f, K, [pc[0], pc[1], -pc[2]])


def po_z_1e6(f):
    # z = 1e-6 in the camera frame of the initial pose: errors ~1e8 px, Jacobian entries ~1e14, finite
    pc = _camera_point(f, K)
    _set_camera_point(f, K, [pc[0], pc[1], 1e-6])


def po_xw_1e30(f):
    # every Xw * 1e30: the translation columns of J are ~1e-28, the rotation columns ordinary
    f.Xw = (f.Xw.astype(np.float64) * 1e30).astype(np.float32)


def po_inv_3e38(f):
    # the largest float information: chi2 and H ~1e42, finite in double
    f.inv_sigma2[:] = np.float32(3e38)


def po_z_1e30_xy_1e15(f):
    # Tcw = I, slot K at (x 1e15, y 1e15, 1e-30): x / z ~1e45, J ~1e92, H terms ~1e185: finite in
    # double, far above every other term of the folds
    _to_camera_frame(f)
    f.Xw[K] = np.array([f.Xw[K, 0] * 1e15, f.Xw[K, 1] * 1e15, 1e-30], np.float32)


def po_same_point(f):
    # every slot the same edge: H = n * one edge's rank-2 J^T W J, regularised by lambda only
    j = 0 if f.u_right is None else int(np.argmax(f.u_right >= 0))  # a stereo slot in the stereo form
    f.Xw[:] = f.Xw[j]
    f.uv[:] = f.uv[j]
    f.inv_sigma2[:] = f.inv_sigma2[j]
    if f.u_right is not None:
        f.u_right[:] = f.u_right[j]


def po_collinear(f):
    # points on a line through the frustum, observed exactly: H has the rotation about the line free
    s = np.linspace(-1.0, 1.0, f.n)
    Xc = np.stack([0.8 * s, 0.5 * s, 4.0 + 1.5 * s], 1)
    f.Xw = ((Xc - f.t_true) @ f.R_true).astype(np.float32)
    f.uv = np.stack([float(f.fx) * Xc[:, 0] / Xc[:, 2] + float(f.cx),
                     float(f.fy) * Xc[:, 1] / Xc[:, 2] + float(f.cy)], 1).astype(np.float32)
    if f.u_right is not None:
        ur = f.uv[:, 0].astype(np.float64) - float(f.bf) / Xc[:, 2]
        f.u_right = np.where(f.u_right >= 0, ur, -1.0).astype(np.float32)


def po_shift_500(f):
    # every observation 500 px off: every edge is an outlier after round 0, so the optimize() calls of
    # rounds 1..3 find no level-0 edge (sparse_optimizer.cpp: "0 vertices to optimize")
    f.uv = (f.uv + np.float32(500.0)).astype(np.float32)
    if f.u_right is not None:
        f.u_right = np.where(f.u_right >= 0, f.u_right + np.float32(500.0), f.u_right).astype(np.float32)


def po_inv_zero(f):
    # information 0: chi2 = 0, H = 0, b = 0, lambda = 1e-5 * 0; the LDLT of the zero matrix stops at
    # its first pivot and counts as positive, x = 0, rho = 0 / 1e-3 = 0: Terminate after one trial
    f.inv_sigma2[:] = 0.0


def po_focal_zero(f):
    # fx = fy = 0: every edge is an outlier (error = uv - (cx, cy)), so rounds 1..3 have no active edge.
    # Mono: J = 0, so H = 0 and b = 0 with a non-zero chi2, and rho = 0 again.  Stereo: the third row
    # keeps its bf terms (J[2][0] = -bf y / z^2, ...), so H != 0 and the LM runs
    f.fx = np.float32(0.0)
    f.fy = np.float32(0.0)


def po_inv_negated(f):
    # H is a sum of PSD terms for every input ORB-SLAM produces (mvInvLevelSigma2 > 0), so H + lambda I
    # is positive and the LDLT never fails there.  The ABI takes the information as given, though: a
    # negative inv_sigma2 makes H negative (semi)definite, LDLT::isPositive() false, and solve() reuses
    # the stale _x with tempChi = DBL_MAX.  The only input found that reaches `!ok2`.  With H negative,
    # scale = x.(lambda x + b) is negative as well, so rho = (currentChi - DBL_MAX) / scale > 0 and,
    # DBL_MAX being finite, the reference accepts such a trial (`not_ok2_accepted`): the stale _x and
    # the substitution then show in the pose.
    f.inv_sigma2 = (-f.inv_sigma2).astype(np.float32)


def po_inv_negated_alternate(f):
    # every second slot negated: H indefinite
    f.inv_sigma2[1::2] = -f.inv_sigma2[1::2]


def po_twelve_identical(f):
    # 12 slots, one edge: above the 10-edge mark, so all four rounds run
    po_same_point(f)


# (name, edit, expected branch counters, slots[, counters expected of the mono form only])
_POSE_C = [
    ("xw_nan", po_xw_nan, ("tempchi_nonfinite", "rho_nan", "currentchi_nonfinite", "rejected"), N_SLOTS),
    ("xw_inf", po_xw_inf, ("tempchi_nonfinite", "rho_nan", "currentchi_nonfinite"), N_SLOTS),
    ("uv_nan", po_uv_nan, ("tempchi_nonfinite", "rho_nan", "currentchi_nonfinite"), N_SLOTS),
    ("identity_one_z0", po_identity_one_z0, ("tempchi_nonfinite", "rho_nan", "currentchi_nonfinite"), N_SLOTS),
    ("identity_one_origin", po_identity_one_origin, ("tempchi_nonfinite", "rho_nan", "currentchi_nonfinite"),
     N_SLOTS),
    ("identity_all_z0", po_identity_all_z0, ("tempchi_nonfinite", "rho_nan", "currentchi_nonfinite"), N_SLOTS),
    ("tcw_nan", po_tcw_nan, ("tempchi_nonfinite", "rho_nan", "currentchi_nonfinite"), N_SLOTS),
    ("behind_camera", po_behind_camera, (), N_SLOTS),
    ("z_1e-6", po_z_1e6, (), N_SLOTS),
    ("xw_1e30", po_xw_1e30, (), N_SLOTS),
    ("inv_3e38", po_inv_3e38, (), N_SLOTS),
    ("z_1e-30_xy_1e15", po_z_1e30_xy_1e15, (), N_SLOTS),
    ("same_point", po_same_point, (), N_SLOTS),
    ("collinear", po_collinear, (), N_SLOTS),
    ("twelve_identical", po_twelve_identical, (), 12),
    ("shift_500", po_shift_500, ("no_active_edge",), N_SLOTS),
    ("inv_zero", po_inv_zero, ("end_rho0", "rejected"), N_SLOTS),
    ("focal_zero", po_focal_zero, ("no_active_edge",), N_SLOTS, ("end_rho0",)),
    ("inv_negated", po_inv_negated, ("not_ok2", "not_ok2_accepted", "rejected"), N_SLOTS),
    ("inv_negated_alternate", po_inv_negated_alternate, ("not_ok2", "not_ok2_accepted", "rejected"), N_SLOTS),
]
POSE_EDITS = {c[0]: c[1] for c in _POSE_C}


def pose_cases_c():
    """Case list C, PoseOptimization: every case in a mono and in a stereo_frac = 0.8 form."""
    out = []
    for k, (name, edit, expect, n, *mono_only) in enumerate(_POSE_C):
        for stereo in (False, True):
            f = pose_base(3000 + k, stereo, n)
            edit(f)
            exp = expect + (mono_only[0] if mono_only and not stereo else ())
            out.append(Case(f"{name}-{'stereo' if stereo else 'mono'}", f, exp))
    return out


POSE_SIZES = (3, 255, 256, 257, 511, 512, 513, 8191, 8192)


def pose_cases_d():
    """Case list D, PoseOptimization: edge counts around the 256-edge slab and at the 8192-edge limit
    (mono and stereo slots mixed), and a Frame with more than 8192 slots of which 8192 hold a map
    point (the limit counts edges)."""
    out = []
    for k, n in enumerate(POSE_SIZES):
        f = synth.make_poseopt_frame(np.random.default_rng(3100 + k), n, 0.8, stereo_frac=0.5)
        out.append(Case(f"edges_{n}", f))
    f = synth.make_poseopt_frame(np.random.default_rng(3120), 8300, 0.8, stereo_frac=0.5)
    drop = np.random.default_rng(3121).choice(8300, 8300 - 8192, replace=False)
    f.has_mp[drop] = 0
    f.Xw[drop] = 0.0
    out.append(Case("slots_8300_edges_8192", f))
    return out


def pose_over_limit():
    """8193 edges: rsc_pose_optimization_many returns RSC_ERR_UNSUPPORTED."""
    return synth.make_poseopt_frame(np.random.default_rng(3130), 8193, 0.8, stereo_frac=0.5)


def pose_regular(k: int):
    """The regular neighbours of the mixed batches."""
    return synth.make_poseopt_frame(np.random.default_rng(3200 + k), 150 + 37 * k, 0.7, no_mp_frac=0.2,
                                    stereo_frac=0.5 * (k % 2))


# ---- Optimizer::OptimizeSim3 ----------------------------------------------------------------------
def sim3_base(seed: int, n: int = N_SLOTS, **kw):
    return synth.make_sim3opt_problem(np.random.default_rng(seed), n, **kw)


def _first_valid(p):
    return int(np.nonzero(p.valid)[0][3])


def so_x2w_nan(p):
    # e12 of one correspondence has a NaN point: chi2, H, b NaN in every pass, rho NaN
    p.X2w[_first_valid(p), 0] = NAN


def so_uv1_inf(p):
    # an infinite observation: error, chi2 and the Huber rho Inf, so currentChi and tempChi are Inf and
    # rho = Inf - Inf = NaN (the numeric J of that edge is Inf - Inf = NaN as well)
    p.uv1[_first_valid(p), 1] = INF


def so_s0_t_nan(p):
    p.S0[5] = np.nan


def so_s0_scale_zero(p):
    # s = 0: inverse() divides by it (-1 / 0 = -Inf, Inf * 0 = NaN in the e21 edges)
    p.S0[7] = 0.0


def so_same_point(p):
    for a in (p.X1w, p.X2w, p.uv1, p.uv2, p.inv1, p.inv2):
        a[:] = a[0]


def so_points_1e30(p):
    # camera-frame points ~1e30 (the float transform R X + t absorbs t): projections keep their size,
    # the translation columns of the numeric J vanish (1e-9 / 1e30 is below the rounding of 1e30)
    p.X1w = (p.X1w.astype(np.float64) * 1e30).astype(np.float32)
    p.X2w = (p.X2w.astype(np.float64) * 1e30).astype(np.float32)


def so_shift_500(p):
    # every e12 edge 500 px off: every correspondence is removed after optimize(5), fewer than 10
    # stay and OptimizeSim3 returns 0 with g2oS12 untouched
    p.uv1 = (p.uv1 + np.float32(500.0)).astype(np.float32)


def so_inv_zero(p):
    # information 0: H = 0, b = 0, lambda = 0, x = 0, rho = 0: Terminate after one trial
    p.inv1[:] = 0.0
    p.inv2[:] = 0.0


def so_inv_negated(p):
    # as po_inv_negated: the only input found that makes H + lambda I non-positive (ORB-SLAM's
    # mvInvLevelSigma2 is positive; the ABI takes the information as given)
    p.inv1 = (-p.inv1).astype(np.float32)
    p.inv2 = (-p.inv2).astype(np.float32)


def so_inv1_negated_alternate(p):
    p.inv1[1::2] = -p.inv1[1::2]


def so_inv_negated_most(p):
    # 70 % of the correspondences negated: H indefinite, a part of the correspondences is removed after
    # optimize(5) and the second optimize(10) runs on the rest, with failing LDLTs in both
    m = np.random.default_rng(4050).random(p.n) < 0.7
    p.inv1[m] = -p.inv1[m]
    p.inv2[m] = -p.inv2[m]


# The `!ok2` pairs start further from the solution (more outliers, a larger pose perturbation): there
# a failed LDLT is followed by an accepted trial — with H negative, scale = x.(lambda x + b) < 0, so
# rho = (currentChi - DBL_MAX) / scale > 0 and DBL_MAX is finite — which makes both the reuse of the
# stale _x and the DBL_MAX substitution visible in the result (`not_ok2_accepted` in the record; on
# scratch copies of the oracle with either rule altered, each of the three results changes).
_NOT_OK2_BASE = dict(seed=5002, outlier_frac=0.3, pose_noise=0.03)


def so_no_correspondence(p):
    # no valid slot: the optimize() call finds no edge (the device call returns before any launch)
    p.valid[:] = 0


_SIM3_C = [
    ("x2w_nan", so_x2w_nan, ("tempchi_nonfinite", "rho_nan", "currentchi_nonfinite", "rejected")),
    ("uv1_inf", so_uv1_inf, ("tempchi_nonfinite", "rho_nan", "currentchi_nonfinite")),
    ("s0_t_nan", so_s0_t_nan, ("tempchi_nonfinite", "rho_nan", "currentchi_nonfinite")),
    ("s0_scale_zero", so_s0_scale_zero, ("tempchi_nonfinite", "rho_nan", "currentchi_nonfinite")),
    ("same_point", so_same_point, ()),
    ("points_1e30", so_points_1e30, ()),
    ("shift_500", so_shift_500, ()),
    ("inv_zero", so_inv_zero, ("end_rho0", "rejected")),
    ("inv_negated", so_inv_negated, ("not_ok2", "not_ok2_accepted", "rejected"), _NOT_OK2_BASE),
    ("inv1_negated_alternate", so_inv1_negated_alternate, ("not_ok2", "not_ok2_accepted"), _NOT_OK2_BASE),
    ("inv_negated_most", so_inv_negated_most, ("not_ok2", "not_ok2_accepted"), _NOT_OK2_BASE),
    ("no_correspondence", so_no_correspondence, ("no_active_edge",)),
]
SIM3_EDITS = {c[0]: c[1] for c in _SIM3_C}


def sim3_cases_c():
    out = []
    for k, (name, edit, expect, *base) in enumerate(_SIM3_C):
        p = sim3_base(**base[0]) if base else sim3_base(4000 + k)
        edit(p)
        out.append(Case(name, p, expect))
    return out


SIM3_SIZES = (31, 32, 33, 95, 96, 97, 8191)


def sim3_with_valid(seed: int, m: int, extra: int = 9):
    """A pair with exactly m valid correspondences among m + extra slots."""
    p = synth.make_sim3opt_problem(np.random.default_rng(seed), m + extra, valid_frac=1.0, outlier_frac=0.15)
    p.valid[:] = 1
    p.valid[np.random.default_rng(seed + 1).choice(m + extra, extra, replace=False)] = 0
    assert int(p.valid.sum()) == m
    return p


def sim3_cases_d():
    """Case list D, OptimizeSim3: valid-correspondence counts at the 64-edge chunk of the cooperative
    form (32 correspondences), the 192-edge slab of the one-workgroup form (96) and below the limit."""
    return [Case(f"corr_{m}", sim3_with_valid(4100 + 2 * k, m)) for k, m in enumerate(SIM3_SIZES)]


def sim3_over_limit():
    """8193 valid correspondences: rsc_optimize_sim3_many returns RSC_ERR_UNSUPPORTED."""
    return sim3_with_valid(4130, 8193, extra=0)


def sim3_regular(k: int):
    return synth.make_sim3opt_problem(np.random.default_rng(4200 + k), 140 + 53 * k, outlier_frac=0.2)


# ---- comparison ----------------------------------------------------------------------------------
def nan_equal(a, b):
    """Bitwise equal, except that NaN matches NaN at the same position (the sign and payload of a
    NaN are not IEEE-specified results: x86 produces the negative default NaN, gfx950 the positive)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.dtype in (np.float32, np.float64)
    if a.shape != b.shape:
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))
