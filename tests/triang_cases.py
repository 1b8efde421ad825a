"""Hand-built cases for SearchForTriangulation, the pair geometry and the CreateNewMapPoints driver (TEST-ONLY), one
per rule, each with its worked answer; and the random problems of the device tests.  See tests/triang_ref.py for
the KeyFrame namespace.

Matcher cases share one frame of mind: F12 = [[0,0,0],[0,0,-1],[0,1,0]] gives the line (a, b, c) = (0, 1, -y1), so
num = y2 - y1, den = 1 and dsqr = (y2 - y1)^2; KeyFrame 2 sits at Rcw = I, tcw = (0, 0, 1) and KeyFrame 1's centre at
the origin, so the epipole is the principal point (320, 240); all keypoints are at octave 0 (sigma2 = 1, accept iff
dsqr < 3.84) unless a case says otherwise."""
from __future__ import annotations

import types

import numpy as np

import triang_ref as tr
from rsc import synth

f32 = np.float32
FX = FY = 512.0
CX, CY = 320.0, 240.0
MB = 0.1
MBF = MB * FX
F_HORIZ = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)
I3 = np.eye(3, dtype=f32)


def make_kf(kp, node, desc=None, octave=None, u_right=None, depth=None, mp_state=None, angle=None, Rcw=I3,
            tcw=(0, 0, 0), mb=MB, mbf=MBF, kp_raw=None, fx=FX, fy=FY, cx=CX, cy=CY):
    """A KeyFrame namespace: `node` is the FeatureVector node id of every feature (features of a node in index
    order, as DBoW2 adds them)."""
    kp = np.asarray(kp, f32).reshape(-1, 2)
    n = len(kp)
    k = types.SimpleNamespace(n=n, kp=kp)
    k.kp_raw = kp.copy() if kp_raw is None else np.asarray(kp_raw, f32).reshape(-1, 2)
    k.octave = np.zeros(n, np.int32) if octave is None else np.asarray(octave, np.int32)
    k.desc = np.zeros((n, 32), np.uint8) if desc is None else np.asarray(desc, np.uint8).reshape(n, 32)
    k.angle = np.zeros(n, f32) if angle is None else np.asarray(angle, f32)
    k.u_right = np.full(n, -1, f32) if u_right is None else np.asarray(u_right, f32)
    k.depth = np.full(n, -1, f32) if depth is None else np.asarray(depth, f32)
    k.mp_state = np.zeros(n, np.uint8) if mp_state is None else np.asarray(mp_state, np.uint8)
    k.mb, k.mbf = float(mb), float(mbf)
    with np.errstate(all="ignore"):  # LocalMapping.cpp:286: cos(2*atan2(mb/2, mvDepth[i])) in float
        k.cos_parallax_stereo = np.cos(f32(2.0) * np.arctan2(f32(f32(mb) / f32(2.0)), k.depth)).astype(f32)
    k.node_id, k.node_begin, k.feat = synth._feature_vector(np.asarray(node, np.uint32).reshape(n)) if n else (
        np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32))
    k.valid = np.ones(n, np.uint8)
    k.Rcw, k.tcw = np.asarray(Rcw, f32).reshape(3, 3).copy(), np.asarray(tcw, f32).reshape(3).copy()
    k.Rwc = k.Rcw.T.copy()  # Twc = Tcw.inverse() (KeyFrame.cpp:64)
    k.Ow = np.array([-tr.dot3(k.Rwc[r], k.tcw) for r in range(3)], f32)
    k.fx, k.fy, k.cx, k.cy = float(fx), float(fy), float(cx), float(cy)
    k.invfx, k.invfy = float(f32(1.0) / f32(fx)), float(f32(1.0) / f32(fy))
    k.Kinv = np.array([[k.invfx, 0, -f32(cx) * f32(k.invfx)], [0, k.invfy, -f32(cy) * f32(k.invfy)], [0, 0, 1]], f32)
    k.scale_factors = synth.scale_factors()
    k.scale_factor = float(synth.SCALE_FACTOR)
    # what rsc_kfview_create also wants (not read by the triangulation)
    k.cell_begin = np.zeros(synth.GRID_COLS * synth.GRID_ROWS + 1, np.int32)
    k.cell_feat = np.zeros(0, np.int32)
    k.mp_pos, k.mp_dmax, k.mp_dmin = np.zeros((n, 3), f32), np.ones(n, f32), np.ones(n, f32)
    k.mp_desc = np.zeros((n, 32), np.uint8)
    k.min_x, k.max_x, k.min_y, k.max_y = 0.0, 2.0 * cx, 0.0, 2.0 * cy
    return k


def bits(k):
    """A 32-byte descriptor with the first k bits set."""
    d = np.zeros(256, np.uint8)
    d[:k] = 1
    return np.packbits(d)


def _kf2(kp, node, **kw):
    return make_kf(kp, node, tcw=(0, 0, 1), **kw)


def _dsqr_edge():
    """(x2, y2, A) with F(2,0) = A (line a = A, b = 1, c = -y1 at y1 = 100) whose dsqr is exactly float(3.84) =
    3.8399999141693115: below 3.84 in double (accepted, :597), not below float(3.84) in float."""
    rng = np.random.default_rng(3)
    target = f32(3.84)
    for _ in range(200):
        A = rng.uniform(0.01, 0.5, 1 << 16).astype(f32)
        x2 = rng.uniform(400, 600, 1 << 16).astype(f32)
        den = (A * A + f32(1.0)).astype(f32)
        num0 = np.sqrt(target * den).astype(f32)  # aim num at sqrt(3.84 den)
        y2 = ((num0 - A * x2) + f32(100.0)).astype(f32)
        num = (((A * x2).astype(f32) + y2).astype(f32) + f32(-100.0)).astype(f32)
        dsqr = ((num * num).astype(f32) / den).astype(f32)
        hit = np.nonzero(dsqr == target)[0]
        if len(hit):
            return float(x2[hit[0]]), float(y2[hit[0]]), float(A[hit[0]])
    raise AssertionError("no exact dsqr found")


def matcher_cases():
    """name -> (kf1, kf2, F12, only_stereo, check_ori, expected matches12, expected nmatches, expected den_zero,
    rules whose turning off changes this case's output)."""
    c = {}
    # distances 49 / 50 / 51 (:580): 50 is kept
    c["dist_49_50_51"] = (make_kf([[500, 100], [500, 120], [500, 140]], [11, 12, 13]),
                          _kf2([[450, 100], [450, 120], [450, 140]], [11, 12, 13], desc=[bits(49), bits(50), bits(51)]),
                          F_HORIZ, 0, 0, [0, 1, -1], 2, 0, ("th_low_kept",))
    # two candidates at distance 10, both on the line: the later position wins
    c["tie_later"] = (make_kf([[500, 100]], [11]), _kf2([[450, 100], [460, 100]], [11, 11], desc=[bits(10), bits(10)]),
                      F_HORIZ, 0, 0, [1], 1, 0, ("tie_later",))
    # a nearer candidate off the line (dy = 5, dsqr = 25) is rejected and must not lower bestDist
    c["reject_keeps_best"] = (make_kf([[500, 100]], [11]),
                              _kf2([[450, 105], [460, 100]], [11, 11], desc=[bits(5), bits(20)]),
                              F_HORIZ, 0, 0, [1], 1, 0, ("reject_keeps_best",))
    # vbMatched2 is never set: two slots take the one KeyFrame-2 feature
    c["shared_feature"] = (make_kf([[500, 100], [510, 101]], [11, 11]), _kf2([[450, 100]], [11]),
                           F_HORIZ, 0, 0, [0, 0], 2, 0, ("vbmatched2_unset",))
    # bOnlyStereo with mvuRight == 0 on both sides: `>= 0` is stereo
    c["stereo_at_zero"] = (make_kf([[500, 100], [500, 120]], [11, 12], u_right=[0, -1], depth=[4, -1]),
                           _kf2([[450, 100], [450, 120]], [11, 12], u_right=[0, 0], depth=[4, 4]),
                           F_HORIZ, 1, 0, [0, -1], 1, 0, ("stereo_ge0",))
    # bOnlyStereo skips a monocular KeyFrame-2 feature (:572-574)
    c["only_stereo_kf2"] = (make_kf([[500, 100]], [11], u_right=[400], depth=[4]),
                            _kf2([[450, 100], [460, 100]], [11, 11], u_right=[350, -1], depth=[4, -1],
                                 desc=[bits(9), bits(3)]),
                            F_HORIZ, 1, 0, [0], 1, 0, ("only_stereo_kf2",))
    # the epipole disc (:585-591), both monocular, octave 0: 10^2 = 100 is not < 100 and goes on; 9.5^2 is skipped
    c["epipole_edge"] = (make_kf([[500, 240], [510, 240]], [11, 12]), _kf2([[330, 240], [329.5, 240]], [11, 12]),
                         F_HORIZ, 0, 0, [0, -1], 1, 0, ("epipole_strict", "epipole_test"))
    # dsqr against 3.84 sigma2 (:597): 1.9^2 accepted, 2^2 rejected, and float(3.84) itself accepted in double
    x2, y2, A = _dsqr_edge()
    F = F_HORIZ.copy()
    F[2, 0] = A
    c["dsqr_sides"] = (make_kf([[0, 100], [0, 100], [0, 100]], [11, 12, 13]),
                       _kf2([[400, f32(101.9) - f32(A) * f32(400)], [400, f32(102.0) - f32(A) * f32(400)], [x2, y2]],
                            [11, 12, 13]), F, 0, 0, [0, -1, 2], 2, 0, ("dsqr_double",))
    # den == 0 planted on slot 1 at (x0, y0) = (300, 200): a = x - x0, b = y - y0
    Fz = np.array([[1, 0, 0], [0, 1, 0], [-300, -200, 1]], f32)
    c["den_zero"] = (make_kf([[500, 100], [300, 200]], [11, 12]), _kf2([[450, 100], [450, 120]], [11, 12]),
                     Fz, 0, 0, [-1, -1], 0, 1, ("den_zero_return",))
    # a slot with a MapPoint (a bad one included) and a KeyFrame-2 feature with one are skipped; so is a node
    # only one FeatureVector holds
    c["eligibility"] = (make_kf([[500, 100], [500, 120], [500, 140], [500, 160]], [11, 12, 13, 14], mp_state=[2, 0, 0, 0]),
                        _kf2([[450, 100], [450, 120], [450, 140], [450, 160]], [11, 12, 13, 15], mp_state=[0, 1, 0, 0]),
                        F_HORIZ, 0, 0, [-1, -1, 2, -1], 1, 0, ())
    # orientation: 11 matches in bin 0 and one in bin 6 (rot = 180): max2 = 1 < 0.1 * 11 removes it
    n = 12
    kp1 = [[500, 100 + 10 * i] for i in range(n)]
    kp2 = [[450, 100 + 10 * i] for i in range(n)]
    c["orientation"] = (make_kf(kp1, 11 + np.arange(n), angle=[0] * 11 + [180]), _kf2(kp2, 11 + np.arange(n)),
                        F_HORIZ, 0, 1, list(range(11)) + [-1], 11, 0, ())
    return c


def _project(kf, X):
    Xc = kf.Rcw.astype(np.float64) @ np.asarray(X, np.float64) + kf.tcw.astype(np.float64)
    return [kf.fx * Xc[0] / Xc[2] + kf.cx, kf.fy * Xc[1] / Xc[2] + kf.cy], Xc[2]


def _two_views(X, t2=(-0.5, 0, 0), d1=(0, 0), d2=(0, 0), oct1=0, oct2=0, stereo1=False, stereo2=False, mbf2=MBF):
    """KeyFrame 1 at the origin, KeyFrame 2 at tcw = t2, one keypoint each: the projections of X (+ pixel offsets)."""
    k1 = make_kf([[0, 0]], [11])
    k2 = make_kf([[0, 0]], [11], tcw=t2, mbf=mbf2)
    for k, d, o, st in ((k1, d1, oct1, stereo1), (k2, d2, oct2, stereo2)):
        p, z = _project(k, X)
        k.kp[0] = [p[0] + d[0], p[1] + d[1]]
        k.kp_raw[0] = k.kp[0]
        k.octave[0] = o
        if st:
            k.depth[0] = z
            k.u_right[0] = f32(k.kp[0, 0]) - f32(f32(MBF) / f32(z))  # consistent with the CURRENT KeyFrame's mbf
            k.cos_parallax_stereo = np.cos(f32(2.0) * np.arctan2(f32(f32(k.mb) / f32(2.0)), k.depth)).astype(f32)
    return k1, k2


def _reproj_edge(X):
    """The reproj2 geometry (one pose twice, KeyFrame 1 stereo: its unprojection is the point) with KeyFrame 2's
    keypoint placed so that errX2^2 + errY2^2 is exactly float(5.991) = 5.991000175476074 at octave 0."""
    a, b = _two_views(X, t2=(0, 0, 0), stereo1=True)
    x3D = tr.unproject_stereo(a, 0)
    R, t = np.asarray(b.Rcw, f32), np.asarray(b.tcw, f32)
    z = f32(tr.dot3(R[2], x3D) + t[2])
    invz = f32(1.0 / float(z))
    u = f32(f32(f32(f32(b.fx) * f32(tr.dot3(R[0], x3D) + t[0])) * invz) + f32(b.cx))
    v = f32(f32(f32(f32(b.fy) * f32(tr.dot3(R[1], x3D) + t[1])) * invz) + f32(b.cy))
    target = f32(5.991)
    rng = np.random.default_rng(4)
    for _ in range(400):
        ang = rng.uniform(0.2, 1.3, 1 << 16)
        r = np.sqrt(float(target)) + rng.uniform(-2e-5, 2e-5, 1 << 16)
        kx, ky = (u - (r * np.cos(ang)).astype(f32)).astype(f32), (v - (r * np.sin(ang)).astype(f32)).astype(f32)
        ex, ey = (u - kx).astype(f32), (v - ky).astype(f32)
        e = ((ex * ex).astype(f32) + (ey * ey).astype(f32)).astype(f32)
        hit = np.nonzero(e == target)[0]
        if len(hit):
            b.kp[0] = b.kp_raw[0] = [kx[hit[0]], ky[hit[0]]]
            return a, b
    raise AssertionError("no exact error sum found")


def pair_cases():
    """name -> (kf1, kf2, idx1, idx2, expected status, expected branch, rules whose turning off changes the output)."""
    c = {}
    X = [0.25, 0.1, 4.0]
    c["ok_mono"] = (*_two_views(X), 0, 0, tr.OK, "svd", ())
    c["low_parallax"] = (*_two_views([0.25, 0.1, 1000.0]), 0, 0, tr.LOW_PARALLAX, "skip", ())
    # the two projections swapped: the rays meet behind the cameras
    a, b = _two_views(X)
    a.kp, b.kp = b.kp.copy(), a.kp.copy()
    c["behind1"] = (a, b, 0, 0, tr.BEHIND1, "svd", ())
    # KeyFrame 1 stereo at the principal point, depth 1; KeyFrame 2 two metres ahead: z2 = -1
    a, b = _two_views([0, 0, 1.0], t2=(0, 0, -2), stereo1=True)
    b.kp[0] = [CX, CY]
    c["behind2"] = (a, b, 0, 0, tr.BEHIND2, "stereo1", ())
    c["reproj1"] = (*_two_views(X, d1=(0, 12)), 0, 0, tr.REPROJ1, "svd", ())
    # the same pose twice, KeyFrame 1 stereo (depth 4): its unprojection is exact, KeyFrame 2's keypoint 10 px off
    c["reproj2"] = (*_two_views(X, t2=(0, 0, 0), d2=(0, 10), stereo1=True), 0, 0, tr.REPROJ2, "stereo1", ())
    # ... and a NaN error passes the `>` test: tcw2.x = NaN makes u2 NaN, z2 stays finite
    a, b = _two_views(X, t2=(0, 0, 0), d2=(0, 10), stereo1=True)
    b.tcw[0] = np.nan
    c["nan_error_passes"] = (a, b, 0, 0, tr.OK, "stereo1", ())
    # KeyFrame 2's stored centre equal to the point: dist2 == 0 (Twc is an input, :392-399)
    a, b = _two_views(X, t2=(0, 0, 0), stereo1=True)
    b.Ow = tr.unproject_stereo(a, 0)
    c["zero_dist"] = (a, b, 0, 0, tr.ZERO_DIST, "stereo1", ("zero_dist_skip",))
    c["scale"] = (*_two_views(X, oct2=7), 0, 0, tr.SCALE, "svd", ("scale_test",))
    # temp(3) == 0: both "rotations" have a zero first column, so A's first column is zero and V's last column
    # is e1 exactly (a (p, 0) block never rotates on the right: both column-0 entries are 0)
    R0 = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1]], f32)
    a = make_kf([[CX, CY]], [11], Rcw=R0, tcw=(0, 0, 0))
    b = make_kf([[CX, CY + 51.2]], [11], Rcw=R0, tcw=(0, 0.5, 0))
    c["svd_w0"] = (a, b, 0, 0, tr.SVD_W0, "svd", ("w0_skip",))
    # both stereo: cosParallaxStereo2 is not read (`else if`, :287); read, KeyFrame 2's near depth would send the
    # pair to its unprojection
    a, b = _two_views(X, stereo1=True, stereo2=True)
    a.depth[0], b.depth[0] = 40.0, 0.2
    for k in (a, b):
        k.cos_parallax_stereo = np.cos(f32(2.0) * np.arctan2(f32(f32(k.mb) / f32(2.0)), k.depth)).astype(f32)
    c["else_if_stereo"] = (a, b, 0, 0, tr.OK, "svd", ("else_if_stereo",))
    # KeyFrame 2 stereo with its own mbf twice the current KeyFrame's: :382 reads the current one, so it passes
    c["mbf_current"] = (*_two_views(X, stereo2=True, mbf2=2 * MBF), 0, 0, tr.OK, "svd", ("mbf_current",))
    # a stereo keypoint (mvuRight >= 0) with mvDepth <= 0: UnprojectStereo gives the zero vector (KeyFrame.cpp:620),
    # whose z1 is exactly 0, and `z1 <= 0` skips (:331)
    a, b = _two_views(X, t2=(0, 0, 0), stereo1=True)
    a.depth[0] = -1.0
    a.cos_parallax_stereo = np.cos(f32(2.0) * np.arctan2(f32(f32(a.mb) / f32(2.0)), a.depth)).astype(f32)
    c["unproject_nonpositive_depth"] = (a, b, 0, 0, tr.BEHIND1, "stereo1", ("unproject_depth_gate", "depth_le0"))
    # KeyFrame 1 stereo at the principal point, depth 1; KeyFrame 2 one metre ahead: z2 == 0 exactly (:335)
    with np.errstate(all="ignore"):
        a, b = _two_views([0, 0, 1.0], t2=(0, 0, -1), stereo1=True)
    b.kp[0] = b.kp_raw[0] = [CX, CY]
    c["z2_zero"] = (a, b, 0, 0, tr.BEHIND2, "stereo1", ("depth_le0",))
    # KeyFrame 2's squared error is exactly float(5.991): above 5.991 in double (:376, skipped), not above
    # float(5.991) * sigma2 in float
    c["reproj_edge"] = (*_reproj_edge(X), 0, 0, tr.REPROJ2, "stereo1", ("reproj_double",))
    # UnprojectStereo reads mvKeys, not mvKeysUn
    a, b = _two_views(X, t2=(0, 0, 0), stereo1=True)
    a.kp_raw[0] = a.kp[0] + f32(0.5)
    c["raw_keys"] = (a, b, 0, 0, tr.OK, "stereo1", ("raw_keys",))
    return c


def scene(rng, poses, n_points=40, mp_frac=0.0, node_groups=None, stereo_frac=0.0, noise=0.0, flips=0, nodes=None):
    """KeyFrames at `poses` ((Rcw, tcw) each) observing n_points world points in front of the first: feature i of
    every KeyFrame is point i; point i sits in node 11 + (i % node_groups), or in nodes[i] when given."""
    X = np.stack([rng.uniform(-1.5, 1.5, n_points), rng.uniform(-1, 1, n_points), rng.uniform(3, 8, n_points)], 1)
    desc = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    node = 11 + (np.arange(n_points) % (node_groups or n_points)) if nodes is None else np.asarray(nodes)
    kfs = []
    for R, t in poses:
        k = make_kf(np.zeros((n_points, 2)), node, Rcw=R, tcw=t)
        for i in range(n_points):
            p, z = _project(k, X[i])
            k.kp[i] = np.asarray(p) + rng.normal(0, noise, 2) if noise else p
            if rng.random() < stereo_frac and z > 0:
                k.depth[i] = z
                k.u_right[i] = f32(k.kp[i, 0]) - f32(f32(MBF) / f32(z))
        k.kp_raw = k.kp.copy()
        k.octave = rng.integers(0, 3, n_points).astype(np.int32)
        k.desc = synth._flip_bits(rng, desc, rng.integers(0, flips + 1, n_points)) if flips else desc.copy()
        k.mp_state = (rng.random(n_points) < mp_frac).astype(np.uint8)
        k.cos_parallax_stereo = np.cos(f32(2.0) * np.arctan2(f32(f32(k.mb) / f32(2.0)), k.depth)).astype(f32)
        kfs.append(k)
    return kfs, X


def driver_cases():
    """name -> (current KeyFrame, neighbours, expected new_neighbour per slot; None = not part of the worked answer)."""
    c = {}
    side, side2, fwd = (I3, (-0.5, 0, 0)), (I3, (0.5, 0, 0)), (I3, (0, 0, -1))
    rng = np.random.default_rng(5)
    # every slot matched by both neighbours: the first succeeds and fills it
    kfs, _ = scene(rng, [(I3, (0, 0, 0)), side, side2], 6)
    c["first_succeeds"] = (kfs[0], kfs[1:], [0] * 6)
    # slot 2's keypoint in the first neighbour sits at octave 7: scale consistency fails there, the second takes it
    kfs, _ = scene(rng, [(I3, (0, 0, 0)), side, side2], 6)
    for k in kfs:
        k.octave[:] = 0
    kfs[1].octave[2] = 7
    c["first_fails"] = (kfs[0], kfs[1:], [0, 0, 1, 0, 0, 0])
    # a neighbour 5 cm away, below its mb = 0.1: skipped (:232-236)
    kfs, _ = scene(rng, [(I3, (0, 0, 0)), (I3, (-0.05, 0, 0)), side], 6)
    c["short_baseline"] = (kfs[0], kfs[1:], [1] * 6)
    # pure forward motion, power-of-two intrinsics, slot 0 at the principal point (its point on the optical axis):
    # x1' F12 = (0, 0, 1) t12x K2inv = 0, den == 0, and the forward neighbour is void ...
    kfs, X = scene(rng, [(I3, (0, 0, 0)), fwd], 6)
    for k in kfs:
        k.kp[0] = k.kp_raw[0] = [CX, CY]
    c["den_zero_voids"] = (kfs[0], kfs[1:], [-1] * 6)
    # ... unless an earlier neighbour filled slot 0 (here only slots 0 and 1 are in the sideways neighbour's nodes)
    kfs, X = scene(rng, [(I3, (0, 0, 0)), side, fwd], 6)
    p, _ = _project(kfs[1], [0, 0, 4.0])
    for k in kfs:
        k.octave[:] = 0
        k.kp[0] = k.kp_raw[0] = [CX, CY]
    kfs[1].kp[0] = kfs[1].kp_raw[0] = p
    kfs[1].node_id, kfs[1].node_begin, kfs[1].feat = synth._feature_vector(np.array([11, 12, 93, 94, 95, 96], np.uint32))
    c["den_zero_filled"] = (kfs[0], kfs[1:], [0, 0, 1, None, None, None])
    return c


def random_pair(rng, n1, n2, sizes1, sizes2, shared_frac=0.5, stereo_frac=0.3, mp_frac=0.2, close_frac=0.6,
                shared=None):
    """A matcher problem with prescribed node sizes: node ids interleaved, about shared_frac of them in both views;
    KeyFrame-2 features of a shared node copy a KeyFrame-1 descriptor of that node with few flips and sit near its
    epipolar line (F_HORIZ: same y), so that winners, ties and rejections all occur."""
    def view(n, sizes, ids):
        node = np.concatenate([np.full(s, i) for s, i in zip(sizes, ids)])
        assert len(node) == n, (len(node), n)
        perm = rng.permutation(n)
        kp = np.stack([rng.uniform(20, 620, n), rng.uniform(20, 460, n)], 1)
        st = rng.random(n) < stereo_frac
        k = make_kf(kp, node[perm], desc=rng.integers(0, 256, (n, 32), dtype=np.uint8),
                    octave=rng.integers(0, 8, n), u_right=np.where(st, kp[:, 0] - 10, -1),
                    depth=np.where(st, MBF / 10, -1), mp_state=(rng.random(n) < mp_frac) * rng.integers(1, 3, n),
                    angle=rng.uniform(0, 360, n), tcw=(0, 0, 1))
        return k
    m = max(len(sizes1), len(sizes2))
    ids1 = 11 + 2 * np.arange(len(sizes1))
    ids2 = np.where(rng.random(len(sizes2)) < shared_frac, 11 + 2 * np.arange(len(sizes2)), 12 + 2 * np.arange(len(sizes2)))
    ids2[0] = 11  # the first (largest) nodes are shared
    if shared is not None:  # node k of KeyFrame 2 shares KeyFrame 1's node k exactly where shared[k]
        ids2 = np.where(np.asarray(shared, bool), 11 + 2 * np.arange(len(sizes2)), 12 + 2 * np.arange(len(sizes2)))
    k1, k2 = view(n1, sizes1, ids1), view(n2, sizes2, ids2)
    pos1 = {int(v): i for i, v in enumerate(k1.node_id)}
    for j, nid in enumerate(k2.node_id):
        if int(nid) not in pos1:
            continue
        i = pos1[int(nid)]
        f1 = k1.feat[k1.node_begin[i]:k1.node_begin[i + 1]]
        for e in k2.feat[k2.node_begin[j]:k2.node_begin[j + 1]]:
            if rng.random() < close_frac:
                s = int(rng.choice(f1))
                k2.desc[e] = synth._flip_bits(rng, k1.desc[s:s + 1], [int(rng.integers(0, 60))])[0]
                k2.kp[e, 1] = k1.kp[s, 1] + rng.choice([0, 0, 1, 2, 4])
    k2.kp_raw = k2.kp.copy()
    return k1, k2


def winner_positions():
    """One KeyFrame-2 node of 257 features (64 lanes stride it: positions 0, 64, 128, 192, 256 fall to lane 0) and one
    of 65 (16 lanes).  Slots 0-2 find their only close candidate at position 0, at the last position and just
    across a group edge (65); slot 3 has an exact tie at positions 63 and 64 (two lanes: the later wins); slots
    4-5 the same in the 65-node at positions 64 and 15 | 16."""
    rng = np.random.default_rng(11)
    n2 = 257 + 65
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    d1 = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    for slot, poss in ((0, [0]), (1, [256]), (2, [65]), (3, [63, 64]), (4, [257 + 64]), (5, [257 + 15, 257 + 16])):
        for q in poss:
            d2[q] = d1[slot]
    k1 = make_kf([[500, 100]] * 6, [11, 11, 11, 11, 12, 12], desc=d1)
    k2 = _kf2([[450, 100]] * n2, [11] * 257 + [12] * 65, desc=d2)
    return k1, k2, [0, 256, 65, 64, 257 + 64, 257 + 16]


def single_feature_nodes():
    """KeyFrame 1 with 8192 features, each alone in its node; KeyFrame 2 with 800 features in the even ones of the
    first 1600 nodes (interleaved: every other KeyFrame-1 node is shared)."""
    rng = np.random.default_rng(12)
    n1, n2 = 8192, 800
    kp1 = np.stack([rng.uniform(20, 620, n1), rng.uniform(20, 460, n1)], 1)
    k1 = make_kf(kp1, 11 + np.arange(n1), desc=rng.integers(0, 256, (n1, 32), dtype=np.uint8),
                 mp_state=rng.random(n1) < 0.1)
    src = 2 * np.arange(n2)
    k2 = _kf2(np.stack([rng.uniform(20, 620, n2), kp1[src, 1] + rng.choice([0, 1, 3], n2)], 1), 11 + src,
              desc=synth._flip_bits(rng, k1.desc[src], rng.integers(0, 70, n2)), octave=rng.integers(0, 8, n2))
    return k1, k2


def fixture_problems():
    """name -> (kf1, kf2, F12, only_stereo, check_ori): the hand-built matcher cases and the shape problems of
    tests/golden/triang_traces.npz (KeyFrame-2 node sizes 1, 2, 63 / 64 / 65, 255 / 256 / 257, 700; KeyFrame-1
    node sizes 1 and 65; n <= 800 but for the 8192 single-feature-node view; half the node ids shared)."""
    p = {n: c[:5] for n, c in matcher_cases().items()}
    k1, k2, _ = winner_positions()
    p["winner_positions"] = (k1, k2, F_HORIZ, 0, 0)
    rng = np.random.default_rng(21)
    ones = [1] * 20
    half = [True, True, True, True] + [i % 2 == 0 for i in range(20)]
    shapes = {"shapes_700": ([65, 40, 1, 1] + ones, [700, 65, 1, 2] + ones),
              "shapes_256": ([65, 1, 30, 1] + ones, [257, 256, 255, 1] + ones),
              "shapes_64": ([65, 65, 65, 1] + ones, [63, 64, 65, 2] + ones)}
    for name, (s1, s2) in shapes.items():
        for only_stereo, check_ori in ((0, 0), (1, 1)):
            a, b = random_pair(rng, sum(s1), sum(s2), s1, s2, shared=half)
            p[f"{name}_s{only_stereo}o{check_ori}"] = (a, b, F_HORIZ, only_stereo, check_ori)
    a, b = single_feature_nodes()
    p["single_feature_nodes"] = (a, b, F_HORIZ, 0, 0)
    return p
