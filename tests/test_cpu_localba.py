"""LocalBundleAdjustment on the host, without a GPU: the sequential restatement of g2o's control flow
(tests/localba_emu mode 0) against the kernels' decomposition with the lanes run one after another (mode 1), byte for
byte on every case of tests/localba_cases.py; the branch record; noise-free known answers; planted outliers; the
stale-chi2 quirk; agreement with the independent numpy solver (tests/localba_ref.py); the reduced solve alone; and
the stand-alone program under the host sanitizers.

Bounds: the elimination orders of the restatement and of numpy.linalg differ and the outputs are
rounded to float, so the bounds are 8x the largest deviation measured over the case list (the margin covers libm and
BLAS differences between machines).  Measured: against the truth on the noise-free scenes, poses 4.13e-6 and points
2.27e-5; against localba_ref.py over REGULAR, poses 2.78e-5 and points 1.44e-4 (both on `outliers`; the other
scenes stay under 5.3e-7 and 2.4e-6)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import localba_cases as lc
import localba_emu_lib as le
import localba_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam2-optimized_amd", "lib")

TRUTH_POSE_BOUND, TRUTH_POINT_BOUND = 8 * 4.13e-6, 8 * 2.27e-5
REF_POSE_BOUND, REF_POINT_BOUND = 8 * 2.78e-5, 8 * 1.44e-4
# where the independent solver legitimately takes another number of trials: name -> reason
REF_DIFFERS = {
    "outliers": "at the 7th iteration of the second optimize() the chi2 gain of a trial is 2e-5 of 41, under the steps "
                "that the stereo projection's float invz puts into chi2; the two solvers stand 1e-7 apart there and "
                "the sign of rho differs, so the numpy solver rejects six trials that the restatement's last one "
                "accepts.  Flags, iterations and the estimates (within the bound) agree.",
}

_runs = {}


def both(name):
    if name not in _runs:
        p = lc.build(name)
        s0, a = le.run(p, 0)
        s1, b = le.run(p, 1)
        assert s0 == 0 and s1 == 0, (name, s0, s1)
        _runs[name] = (p, a, b)
    return _runs[name]


def same_double(v, w):
    return np.float64(v).tobytes() == np.float64(w).tobytes()


@pytest.mark.parametrize("name", list(lc.CASES))
def test_sequential_equals_decomposed(name):
    p, a, b = both(name)
    for k in ("Tcw", "pos", "edge_flags", "erase"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (name, k)
    for k in ("n_erase", "n_level1", "status", "branches"):
        assert a[k] == b[k], (name, k, a[k], b[k])
    for i in range(2):
        for k, v in a["phase"][i].items():
            w = b["phase"][i][k]
            assert same_double(v, w) if isinstance(v, np.float64) else v == w, (name, i, k, v, w)


def test_every_reachable_branch_is_taken():
    """Every counter of the branch record is raised by some case, except the zero pivot: the reduced system's diagonal
    carries lambda = 1e-5 max|diag H| > 0 unless every diagonal entry of H is zero, and then (Hll + lambda I) is the zero
    matrix, its cofactor inverse is NaN and so is every pivot — never 0.  The reduced solve's refusal is held by
    test_reduced_solve_forms below and by the stand-alone program."""
    total = {}
    for name in lc.CASES:
        for k, v in both(name)[1]["branches"].items():
            total[k] = total.get(k, 0) + v
    missing = [k for k, v in total.items() if v == 0]
    assert missing == ["zero_pivot"], total


def test_statuses_of_the_degenerate_cases():
    assert both("no_edges")[1]["status"] == 3 and both("no_points")[1]["status"] == 3
    assert both("no_free_kf")[1]["status"] == 4
    r = both("all_level1")[1]
    assert r["status"] == 2 and r["n_level1"] == r["n_erase"] == len(r["edge_flags"])
    assert r["phase"][1]["lm_iterations"] == 0 and r["phase"][1]["n_edges"] == 0
    # no edge: a free pose comes back as the quaternion round trip of its entry value, a fixed one as its bytes
    p, a, _ = both("no_edges")
    fixed = p["fixed"] == 1
    assert np.array_equal(a["Tcw"][fixed].view(np.uint32), p["Tcw"][fixed].view(np.uint32))
    assert np.allclose(a["Tcw"][~fixed], p["Tcw"][~fixed], atol=1e-6, rtol=0)
    assert np.array_equal(a["pos"].view(np.uint32), p["pos"].view(np.uint32))
    # a NaN in a fixed KeyFrame's pose comes back as given
    p, a, _ = both("edge_nan_fixed_pose")
    assert np.array_equal(a["Tcw"][p["fixed"] == 1].view(np.uint32), p["Tcw"][p["fixed"] == 1].view(np.uint32))


def test_exact_observations_end_each_phase_after_one_trial():
    r = both("exact")[1]
    assert [q["lm_trials"] for q in r["phase"]] == [1, 1] and r["branches"]["rho_zero"] == 2
    assert r["phase"][0]["chi2_first"] == 0.0 and r["phase"][1]["chi2_last"] == 0.0


@pytest.mark.parametrize("i", range(len(lc.KNOWN)))
def test_noise_free_known_answer(i):
    """At least two fixed KeyFrames fix the gauge; perturbed free poses and points return to the truth."""
    p = lc.known_answer(i)
    assert int(p["fixed"].sum()) >= 2
    st, r = le.run(p, 0)
    assert st == 0 and r["n_erase"] == 0
    K = len(p["kf_id"])
    d_in = np.abs(p["Tcw"].reshape(K, 4, 4) - p["true_Tcw"]).max()
    d_pose = np.abs(r["Tcw"].reshape(K, 4, 4) - p["true_Tcw"]).max()
    d_pt = np.abs(r["pos"] - p["true_pos"]).max()
    print(f"known answer {i}: pose {d_pose:.3e} (entry {d_in:.3e}) point {d_pt:.3e}")
    assert d_in > 1e-3
    assert d_pose <= TRUTH_POSE_BOUND and d_pt <= TRUTH_POINT_BOUND


def test_planted_outliers_are_erased_and_inliers_are_not():
    p, r, _ = both("outliers")
    erased = (r["edge_flags"] & 2) != 0
    assert p["outlier"].sum() >= 10
    assert np.array_equal(erased, p["outlier"] == 1)
    assert sorted(r["erase"].tolist()) == np.nonzero(erased)[0].tolist()
    mono = p["u_right"][r["erase"]] < 0  # the mono edges first, then the stereo ones, each in edge order
    nm = int(mono.sum())
    assert mono[:nm].all() and not mono[nm:].any()
    assert (np.diff(r["erase"][:nm]) > 0).all() and (np.diff(r["erase"][nm:]) > 0).all()


def test_vertices_without_level0_edges_leave_the_second_phase():
    p, r, _ = both("lose_all")
    assert r["branches"]["vertex_dropped"] >= 2
    assert r["phase"][1]["n_vertices"] < r["phase"][0]["n_vertices"]
    assert r["phase"][1]["n_points"] < r["phase"][0]["n_points"]
    e0 = list(lc.edges_of_point(p, 0))
    assert (r["edge_flags"][e0] == 3).all()


def test_bad_point_keeps_level0_and_is_never_erased():
    p, r, _ = both("bad_point")
    e = list(lc.edges_of_point(p, 3))
    assert (r["edge_flags"][e] == 0).all()
    q = dict(p)
    q["bad"] = np.zeros_like(p["bad"])
    st, g = le.run(q, 0)
    assert g["edge_flags"][e[0]] == 3  # the same observation on a good point is over the threshold


def test_stale_chi2_quirk():
    """The edge is flagged for depth alone after the first optimize() (its chi2 is far under the threshold), the
    second brings the point in front of its KeyFrame again, and the final loop — which reads the edge's first-phase
    chi2 and the final depth — leaves it out of vToErase."""
    p, r, _ = both("stale_chi2")
    e = lc.STALE_EDGE
    assert r["edge_flags"][e] == 1 and e not in r["erase"].tolist()
    assert r["branches"]["stale_kept"] == 1 and r["n_level1"] == 1 and r["n_erase"] == 0
    k = p["obs_kf"][e]
    T = p["Tcw"][k].reshape(4, 4).astype(np.float64)
    z_in = T[2, :3] @ p["pos"][0].astype(np.float64) + T[2, 3]
    z_out = T[2, :3] @ r["pos"][0].astype(np.float64) + T[2, 3]
    assert z_in < 0 < z_out
    # an edge over the chi2 threshold stays in vToErase whatever the second optimize() did
    q, g, _ = both("outliers")
    assert ((g["edge_flags"] & 1) <= (g["edge_flags"] >> 1)).all()


@pytest.mark.parametrize("name", lc.REGULAR)
def test_agrees_with_independent_solver(name):
    p, a, _ = both(name)
    r = localba_ref.solve(p)
    K = len(p["kf_id"])
    free = p["fixed"] == 0
    d_pose = np.abs(a["Tcw"].reshape(K, 4, 4)[free].astype(np.float64) - r["Tcw"][free]).max()
    d_pt = np.abs(a["pos"].astype(np.float64) - r["pos"]).max()
    print(f"{name}: pose {d_pose:.3e} point {d_pt:.3e}")
    assert d_pose <= REF_POSE_BOUND and d_pt <= REF_POINT_BOUND
    assert np.array_equal(a["edge_flags"], r["edge_flags"])
    assert [q["lm_iterations"] for q in a["phase"]] == r["iterations"]
    if name not in REF_DIFFERS:
        assert [q["lm_trials"] for q in a["phase"]] == r["trials"]


def test_list_of_differences_is_short():
    assert set(REF_DIFFERS) <= set(lc.REGULAR) and 10 * len(REF_DIFFERS) < len(lc.REGULAR)


def test_reduced_solve_forms():
    """The up-looking LDL^T of the sequential form and the right-looking one of the kernels give the same bytes, solve
    the system, read the upper triangle only, and refuse a zero pivot with x untouched."""
    L = le.lib()
    L.lbae_solve.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    rng = np.random.default_rng(7)
    for n in (1, 2, 6, 60, 66, 384):
        M = rng.normal(size=(n, n + 5))
        A = M @ M.T + n * np.eye(n)
        b = rng.normal(size=n)
        U = np.triu(A) + np.tril(rng.normal(size=(n, n)), -1)  # garbage below the diagonal
        xs = []
        for mode in (0, 1):
            x = np.full(n, 7.0)
            assert L.lbae_solve(n, U.ctypes.data, b.ctypes.data, mode, x.ctypes.data) == 1
            xs.append(x)
        assert np.array_equal(xs[0].view(np.uint64), xs[1].view(np.uint64)), n
        assert np.abs(xs[0] - np.linalg.solve(A, b)).max() <= 1e-9 * np.abs(xs[0]).max()
    A = np.array([[1.0, 1.0], [1.0, 1.0]])  # the second pivot is 1 - 1 * 1 = 0
    for mode in (0, 1):
        x = np.full(2, 7.0)
        assert L.lbae_solve(2, A.ctypes.data, np.ones(2).ctypes.data, mode, x.ctypes.data) == 0
        assert (x == 7.0).all()


def _edge(pose, cam, X, upd, dX, obs, inv, stereo, robust):
    L = le.lib()
    vp = C.c_void_p
    L.lbae_edge.argtypes = [vp, vp, vp, vp, vp, vp, C.c_double, C.c_int, C.c_int, vp, vp, vp, vp]
    L.lbae_edge.restype = None
    arrs = [np.ascontiguousarray(a, np.float64) for a in (pose, cam, X, upd, dX, obs)]
    e, A, B, t = np.zeros(3), np.zeros(9), np.zeros(18), np.zeros(72)
    L.lbae_edge(*[a.ctypes.data for a in arrs], float(inv), int(stereo), int(robust), e.ctypes.data, A.ctypes.data,
                B.ctypes.data, t.ctypes.data)
    return e, A.reshape(3, 3), B.reshape(3, 6), t


@pytest.mark.parametrize("stereo", [0, 1])
def test_edge_arithmetic_against_numpy(stereo):
    """The per-edge arithmetic is shared by the sequential form and the kernels, so it is held here on its own:
    lba_jacobians against central differences of the edge's own error (po_error) in the point and in the pose
    update, and the 72 terms of lba_quad_terms, the transposed Hpl block among them, against numpy products of
    the returned A, B and e, with and without the Huber kernel.

    Bounds.  A central difference with step h is off by eps_e / h + h^2 |e(3)| / 6.  The mono error is double
    arithmetic (eps_e ~ 1e-13 px at 500 px, h = 1e-5: 1e-8, the cubic term under 1e-7): bound 1e-6 on entries of
    size up to 1e3.  The stereo error rounds invz to float: eps_e <= 2^-24 |invz| (|x| fx + bf) per evaluation, two
    evaluations over 2 h with h = 1e-3, plus the cubic term under 1e-3: the bound is worked out per edge below.  A
    pose column carries the factor |d pc / d omega| <= |pc| < 10.  The terms are sums of at most three products of
    at most three factors: relative 1e-12 of the largest term."""
    rng = np.random.default_rng(70 + stereo)
    for trial in range(20):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = rng.uniform(0, 0.5)
        q = np.concatenate([np.sin(ang / 2) * ax, [np.cos(ang / 2)]])
        pose = np.concatenate([q, rng.normal(0, 0.3, 3)])
        cam = np.array([500.0, 480.0, 320.0, 240.0, 40.0])
        X = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 9)])
        obs = np.array([rng.uniform(0, 640), rng.uniform(0, 480), rng.uniform(0, 640)])
        inv = 0.7
        z6, z3 = np.zeros(6), np.zeros(3)
        e, A, B, _ = _edge(pose, cam, X, z6, z3, obs, inv, stereo, 0)
        D = 3 if stereo else 2
        h = 1e-3 if stereo else 1e-5
        Rq = np.array([[1 - 2 * (q[1] ** 2 + q[2] ** 2), 2 * (q[0] * q[1] - q[2] * q[3]), 2 * (q[0] * q[2] + q[1] * q[3])],
                       [2 * (q[0] * q[1] + q[2] * q[3]), 1 - 2 * (q[0] ** 2 + q[2] ** 2), 2 * (q[1] * q[2] - q[0] * q[3])],
                       [2 * (q[0] * q[2] - q[1] * q[3]), 2 * (q[1] * q[2] + q[0] * q[3]), 1 - 2 * (q[0] ** 2 + q[1] ** 2)]])
        pc = Rq @ X + pose[4:]
        assert 2 < pc[2] and np.linalg.norm(pc) < 10
        bound = 1e-6 if not stereo else 2.0 ** -24 / pc[2] * (np.abs(pc[:2]).max() * 500 + 40) / h + 1e-3
        for j in range(3):
            d = np.zeros(3)
            d[j] = h
            fd = (_edge(pose, cam, X, z6, d, obs, inv, stereo, 0)[0] - _edge(pose, cam, X, z6, -d, obs, inv, stereo, 0)[0]) / (2 * h)
            assert np.abs(fd[:D] - A[:D, j]).max() <= bound, (trial, "A", j, fd, A[:, j])
        for j in range(6):
            d = np.zeros(6)
            d[j] = h
            fd = (_edge(pose, cam, X, d, z3, obs, inv, stereo, 0)[0] - _edge(pose, cam, X, -d, z3, obs, inv, stereo, 0)[0]) / (2 * h)
            assert np.abs(fd[:D] - B[:D, j]).max() <= 10 * bound, (trial, "B", j, fd, B[:, j])
        for robust in (0, 1):
            e, A, B, t = _edge(pose, cam, X, z6, z3, obs, inv, stereo, robust)
            A, B, e = A[:D], B[:D], e[:D]
            chi2 = inv * float(e @ e)
            delta = float(np.float32(np.sqrt(7.815 if stereo else 5.991)))
            rho1 = delta / np.sqrt(chi2) if (robust and chi2 > delta * delta) else 1.0
            assert not robust or rho1 < 1.0  # random observations are far off: the kernel is active
            W = rho1 * inv * np.eye(D)
            omega_r = -rho1 * inv * e
            want = np.concatenate([(A.T @ W @ A).ravel(), A.T @ omega_r, (B.T @ W @ B).ravel(), B.T @ omega_r,
                                   (B.T @ W @ A).ravel()])
            assert np.abs(t - want).max() <= 1e-12 * np.abs(want).max(), (trial, robust)


@pytest.mark.parametrize("exe", ["localba_test", "localba_test_san"])
def test_standalone_program(exe):
    out = subprocess.run([os.path.join(LIBDIR, exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok") and "DIFFERENT" not in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
