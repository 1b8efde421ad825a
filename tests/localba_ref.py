"""An independent float64 solver of the two-phase LocalBundleAdjustment problem (Optimizer.cpp:426-787) in numpy:
dense normal equations over all free parameters (6 per free KeyFrame, 3 per point), no Schur complement, numpy.linalg
for the solve, rotation matrices instead of quaternions, numeric-free analytic Jacobians written from the camera
model.  It shares no code with csrc/rsc_localba.h; tests/test_cpu_localba.py holds the restatement against it."""
import numpy as np

CHI2 = (5.991, 7.815)
DELTA = (float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815))))


def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _exp(u):
    w, v = u[:3], u[3:]
    th = np.linalg.norm(w)
    W = _skew(w)
    if th < 1e-5:
        R = np.eye(3) + W + W @ W
        V = R
    else:
        R = np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W
    return R, V @ v


class Problem:
    def __init__(self, p):
        self.K, self.N = len(p["kf_id"]), len(p["mp_id"])
        T = np.asarray(p["Tcw"], np.float64).reshape(self.K, 4, 4)
        self.R = T[:, :3, :3].copy()
        for k in range(self.K):  # the entry rotation goes through a unit quaternion in the reference
            U, _, Vt = np.linalg.svd(self.R[k]) if np.all(np.isfinite(self.R[k])) else (self.R[k], 0, np.eye(3))
            self.R[k] = U @ Vt
        self.t = T[:, :3, 3].copy()
        self.X = np.asarray(p["pos"], np.float64).copy()
        self.cam = np.asarray(p["cam"], np.float64)
        self.fixed = np.asarray(p["fixed"]).astype(bool)
        self.bad = np.asarray(p["bad"]).astype(bool)
        begin = np.asarray(p["obs_begin"])
        self.e_pt = np.repeat(np.arange(self.N), np.diff(begin)).astype(int)
        self.e_kf = np.asarray(p["obs_kf"]).astype(int)
        self.uv = np.asarray(p["uv"], np.float64).reshape(-1, 2)
        self.ur = np.asarray(p["u_right"], np.float64)
        self.inv = np.asarray(p["inv_sigma2"], np.float64)
        self.stereo = ~(np.asarray(p["u_right"]) < 0)
        self.E = len(self.e_kf)
        self.kf_rank = np.argsort(np.argsort(np.asarray(p["kf_id"])))
        self.mp_rank = np.argsort(np.argsort(np.asarray(p["mp_id"])))

    def residual(self, e, jac=False):
        k, i = self.e_kf[e], self.e_pt[e]
        fx, fy, cx, cy, bf = self.cam[k]
        pc = self.R[k] @ self.X[i] + self.t[k]
        x, y, z = pc
        st = self.stereo[e]
        if st:
            iz = float(np.float32(1.0 / z))
            proj = np.array([x * iz * fx + cx, y * iz * fy + cy, x * iz * fx + cx - bf * iz])
            r = np.array([self.uv[e, 0], self.uv[e, 1], self.ur[e]]) - proj
        else:
            r = self.uv[e] - np.array([fx * x / z + cx, fy * y / z + cy])
        if not jac:
            return r, z
        # d proj / d pc, then the chain: pc = exp(u) T X -> d pc / d u = [-pc^, I], d pc / d X = R
        J = np.array([[fx / z, 0, -fx * x / z ** 2], [0, fy / z, -fy * y / z ** 2]])
        if st:
            J = np.vstack([J, J[0] + np.array([0, 0, bf / z ** 2])])
        Jp = -J @ self.R[k]
        Jk = -J @ np.hstack([-_skew(pc), np.eye(3)])
        return r, z, Jp, Jk


def optimize(P, active, robust, iters):
    """g2o's Levenberg loop over the edges `active` (ascending); returns (iterations, trials)."""
    if len(active) == 0:
        return 0, 0
    kfs = sorted({P.e_kf[e] for e in active if not P.fixed[P.e_kf[e]]}, key=lambda k: P.kf_rank[k])
    pts = sorted({P.e_pt[e] for e in active}, key=lambda i: P.mp_rank[i])
    ck = {k: 6 * j for j, k in enumerate(kfs)}
    cp = {i: 6 * len(kfs) + 3 * j for j, i in enumerate(pts)}
    n = 6 * len(kfs) + 3 * len(pts)

    def chi():
        c = 0.0
        for e in active:
            r, _ = P.residual(e)
            c2 = P.inv[e] * float(r @ r)
            d = DELTA[int(P.stereo[e])]
            c += c2 if (not robust[e] or c2 <= d * d) else 2 * np.sqrt(c2) * d - d * d
        return c

    lam, ni, nbad, its, trials = 0.0, 2.0, 0, 0, 0
    xs = np.zeros(n)
    for it in range(iters):
        its += 1
        cur = chi()
        ini = cur
        H = np.zeros((n, n))
        b = np.zeros(n)
        for e in active:
            r, _, Jp, Jk = P.residual(e, True)
            w = P.inv[e]
            c2 = w * float(r @ r)
            d = DELTA[int(P.stereo[e])]
            rho1 = 1.0 if (not robust[e] or c2 <= d * d) else d / np.sqrt(c2)
            cols = [(cp[P.e_pt[e]], Jp)]
            if not P.fixed[P.e_kf[e]]:
                cols.append((ck[P.e_kf[e]], Jk))
            for c0, Ja in cols:
                b[c0:c0 + Ja.shape[1]] -= rho1 * w * (Ja.T @ r)
                for c1, Jb in cols:
                    H[c0:c0 + Ja.shape[1], c1:c1 + Jb.shape[1]] += rho1 * w * (Ja.T @ Jb)
        if it == 0:
            lam, ni, nbad = 1e-5 * float(np.max(np.abs(np.diag(H)))), 2.0, 0
        q = 0
        while True:
            trials += 1
            keep = (P.R.copy(), P.t.copy(), P.X.copy())
            ok = True
            try:
                A = H + lam * np.eye(n)
                if not np.all(np.isfinite(A)) or not np.all(np.isfinite(b)):
                    raise np.linalg.LinAlgError
                xs = np.linalg.solve(A, b)
            except np.linalg.LinAlgError:
                ok = False
            for k in kfs:
                dR, dt = _exp(xs[ck[k]:ck[k] + 6])
                P.R[k], P.t[k] = dR @ P.R[k], dR @ P.t[k] + dt
            for i in pts:
                P.X[i] = P.X[i] + xs[cp[i]:cp[i] + 3]
            tmp = chi() if ok else np.finfo(np.float64).max
            scale = float(xs @ (lam * xs + b)) + 1e-3
            rho = (cur - tmp) / scale
            if rho > 0 and np.isfinite(tmp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = tmp
            else:
                lam *= ni
                ni *= 2
                P.R, P.t, P.X = keep
            q += 1
            if not (rho < 0 and q < 10):
                break
        if q == 10 or rho == 0:
            break
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            break
    return its, trials


def solve(p):
    """dict: Tcw float64 [K,4,4], pos float64 [N,3], edge_flags uint8 [E], iterations / trials per phase."""
    P = Problem(p)
    level = np.zeros(P.E, bool)
    robust = np.ones(P.E, bool)
    err = [None] * P.E
    out = dict(iterations=[0, 0], trials=[0, 0])
    flags = np.zeros(P.E, np.uint8)
    for phase in range(2):
        active = [e for e in range(P.E) if not level[e]]
        out["iterations"][phase], out["trials"][phase] = optimize(P, active, robust, 5 if phase == 0 else 10)
        for e in active:
            err[e] = P.residual(e)[0]  # of the estimates the phase leaves (the restatement: of the last trial)
        for e in range(P.E):
            if P.bad[P.e_pt[e]] or err[e] is None:
                continue
            c2 = P.inv[e] * float(err[e] @ err[e])
            over = c2 > CHI2[int(P.stereo[e])] or not (P.residual(e)[1] > 0)
            if phase == 0:
                level[e] = over
                robust[e] = False
                flags[e] |= 1 if over else 0
            elif over:
                flags[e] |= 2
    T = np.tile(np.eye(4), (P.K, 1, 1))
    T[:, :3, :3], T[:, :3, 3] = P.R, P.t
    out.update(Tcw=T, pos=P.X, edge_flags=flags)
    return out
