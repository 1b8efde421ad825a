"""Hand-built problems with known answers for ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cpp:671-821),
one per rule (TEST-ONLY), shared by the CPU tests, the GPU tests and the golden fixture, and the random crowded
problems of the fixture.

Geometry that can be checked by hand (tests/kfproj_cases.py): identity pose, fx = fy = 100, cx = 300, cy = 200, so
a point (x, y, 1) projects to u = 100 x + 300, v = 100 y + 200; Ow = 0 unless the case stores another; image
[0, 700) x [0, 480); grid cells 11.75 px wide and 10 px tall, a keypoint's cell is round(x / 11.75), round(y / 10).
mbf = 40, so ur = u - 40 / z.  A point at distance d with mfMaxDistance = d * 1.2^(L - 0.5) predicts level L
(level 0: mfMaxDistance = d); th = 3, so the radius is 3 * 1.2^L and mvInvLevelSigma2[0] = 1.  Descriptors: a
point's is all zeros, a keypoint's has its first `bits` bits set, so the distance is `bits`.

Where a gate compares a computed float with a bound, the case holds the input on the bound and its neighbouring
floats; where the bound is not a float the inputs are found by stepping float by float (`last_float_where`) over
the gate's own formula written out here, with the straddle asserted."""
from __future__ import annotations

import types

import numpy as np

import kfproj_cases as kc
import kfproj_ref as kr
from rsc import synth

f32 = np.float32
FX = FY = 100.0
CX, CY = 300.0, 200.0
MAX_X = 700.0
MBF = 40.0
TH = 3.0
desc_bits = kc.desc_bits


def pt(x, y, z=1.0, level=0, state=1, skip=0, normal=(0.0, 0.0, 10.0), dmax=None, dmin=0.01, desc=None):
    return dict(pos=(x, y, z), level=level, state=state, skip=skip, normal=normal, dmax=dmax, dmin=dmin, desc=desc)


def kpt(u, v, bits, octave=0, ur=-1.0, desc=None):
    return dict(pt=(u, v), bits=bits, octave=octave, ur=ur, desc=desc)


def make_kf(kp, octave, desc, u_right, R=None, t=None, Ow=None, mbf=MBF, **kw):
    """A KeyFrame view with what rsc_kfview_set_triangulation carries.  Ow defaults to -R^T t in float64 rounded
    once (any stored value will do: the matcher reads it, it does not derive it)."""
    kf = kc.make_kf(kp, octave, desc, None, R, t, **kw)
    n = kf.n
    R64, t64 = np.asarray(kf.Rcw, np.float64), np.asarray(kf.tcw, np.float64)
    kf.u_right = np.ascontiguousarray(u_right, f32).reshape(n)
    kf.Ow = (-(R64.T @ t64)).astype(f32) if Ow is None else np.asarray(Ow, f32)
    kf.Rwc = R64.T.astype(f32)
    kf.mbf, kf.mb = float(mbf), float(mbf) / kf.fx
    kf.depth = np.where(kf.u_right >= 0, f32(4.0), f32(-1.0)).astype(f32)
    kf.kp_raw = np.asarray(kf.kp, f32).copy()
    kf.cos_parallax_stereo = np.ones(n, f32)
    kf.invfx, kf.invfy = 1.0 / kf.fx, 1.0 / kf.fy
    kf.scale_factor = float(synth.SCALE_FACTOR)
    kf.Kinv = np.array([[kf.invfx, 0, -kf.cx * kf.invfx], [0, kf.invfy, -kf.cy * kf.invfy], [0, 0, 1]], f32)
    return kf


def build(pts, kps, th=TH, **kw):
    """A problem namespace: kf, pts, skip, th."""
    n = len(pts)
    pos = np.array([p["pos"] for p in pts], f32).reshape(n, 3)
    dist = np.sqrt((pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]) + pos[:, 2] * pos[:, 2]).astype(f32)
    dmax = np.array([p["dmax"] if p["dmax"] is not None else
                     (d if p["level"] == 0 else f32(d * 1.2 ** (p["level"] - 0.5))) for d, p in zip(dist, pts)], f32)
    P = kr.points_of(state=[p["state"] for p in pts], pos=pos, normal=[p["normal"] for p in pts], dmax=dmax,
                     dmin=[p["dmin"] for p in pts],
                     desc=[np.zeros(32, np.uint8) if p["desc"] is None else p["desc"] for p in pts])
    kw.setdefault("max_x", MAX_X)
    kf = make_kf([k["pt"] for k in kps], [k["octave"] for k in kps],
                 [desc_bits(k["bits"]) if k["desc"] is None else k["desc"] for k in kps], [k["ur"] for k in kps],
                 fx=FX, fy=FY, cx=CX, cy=CY, **kw)
    return types.SimpleNamespace(kf=kf, pts=P, skip=np.array([p["skip"] for p in pts], np.uint8), th=float(th))


def last_float_where(x, towards, pred):
    """Steps x float by float towards `towards` while pred holds: (the last x where it holds, the first where not)."""
    x, towards = f32(x), f32(towards)
    assert pred(x)
    for _ in range(100000):
        y = np.nextafter(x, towards)
        if not pred(y):
            return x, y
        x = y
    raise AssertionError("no boundary within 100000 floats")


def _u(x):  # :706-709 at z = 1 (invz = 1)
    return f32(f32(f32(FX) * f32(x)) + f32(CX))


def _v(y):
    return f32(f32(f32(FY) * f32(y)) + f32(CY))


def _e2_mono(kx):  # :778-780 for a keypoint (kx, 200) against u = 300, v = 200
    ex = f32(f32(300.0) - f32(kx))
    return f32(f32(ex * ex) + f32(0.0))


def cases():
    """name -> (problem, expected best_idx list over the points).  Expected values are worked out in the comments,
    not computed."""
    out = {}
    up, down = f32(np.inf), f32(-np.inf)
    # 1. depth (:702): z < 0 skips ((0, 0, -1) would land on keypoint 0; so would the smallest negative float);
    #    z = +0: invz = +inf, (1, 0, +0) -> u = inf, (0, 0, +0) -> 0 * inf = NaN; camera z = -0 is NOT < 0: invz =
    #    -inf, u = +-inf: IsInImage is false for all of them.  A camera z of -0 needs every term of the row sum to
    #    be -0: tcw.z = -0 and the point (-1, -1, -0), whose row is 0*-1 + 0*-1 + 1*-0 + -0.  (1, 0, 1) -> u = 400
    #    takes keypoint 1
    out["z_sign"] = (build([pt(0.0, 0.0, -1.0), pt(0.0, 0.0, -1e-45), pt(1.0, 0.0, 0.0), pt(0.0, 0.0, 0.0),
                            pt(-1.0, -1.0, -0.0), pt(1.0, 0.0)],
                           [kpt(300, 200, 3), kpt(400, 200, 3)], t=(0.0, 0.0, -0.0)), [-1, -1, -1, -1, -1, 1])
    # 2. IsInImage: u = 0 = mnMinX is inside, the next x below gives u < 0: outside; u = 700 = mnMaxX is outside,
    #    the last x with u < 700 inside.  Keypoints 1 px inside either bound (ex^2 <= 2.25 passes the mono gate)
    x_lo = np.nextafter(f32(-3.0), down)
    x_hi, x_out = last_float_where(3.9999, 5.0, lambda x: _u(x) < f32(700.0))
    assert _u(-3.0) == 0.0 and _u(x_lo) < 0.0 and _u(4.0) == 700.0 and _u(x_out) >= 700.0 and _u(x_hi) > 699.9
    out["bounds_u"] = (build([pt(-3.0, 0.0), pt(x_lo, 0.0), pt(np.nextafter(f32(-3.0), up), 0.0), pt(4.0, 0.0),
                              pt(x_out, 0.0), pt(x_hi, 0.0)], [kpt(1, 200, 3), kpt(698.5, 200, 3)]),
                       [0, -1, 0, -1, -1, 1])
    y_lo = np.nextafter(f32(-2.0), down)
    #    (mnMaxY = 470 here: under 480 a keypoint within 3 px of the bound is in grid row round(47.7) = 48, which
    #    AssignFeaturesToGrid drops)
    y_hi, y_out = last_float_where(2.6999, 3.0, lambda y: _v(y) < f32(470.0))
    assert _v(-2.0) == 0.0 and _v(y_lo) < 0.0 and _v(y_out) >= 470.0 and _v(y_hi) > 469.9
    out["bounds_v"] = (build([pt(0.0, -2.0), pt(0.0, y_lo), pt(0.0, np.nextafter(f32(-2.0), up)), pt(0.0, y_out),
                              pt(0.0, y_hi)], [kpt(300, 1, 3), kpt(300, 468.5, 3)], max_y=470.0), [0, -1, 0, -1, 1])
    # 3. 0.8f*dmin <= dist3D <= 1.2f*dmax, both ends inside (the numbers of kfproj_cases: 0.8f * 2.5 rounds to 2.0,
    #    1.2f * 2.5 = 3 + 2^-23 ties to 3.0), with the next float of the bound on either side.  The dmax = 2.5
    #    point has ratio 2.5 / 3: PredictScale's ceil gives -1 or 0, clamped to level 0 (lo = -1) either way
    out["dist_edges"] = (build([pt(0.0, 0.0, 2.0, dmin=2.5), pt(0.0, 0.0, 2.0, dmin=np.nextafter(f32(2.5), up)),
                                pt(0.0, 0.0, 2.0, dmin=np.nextafter(f32(2.5), down)), pt(0.0, 0.0, 3.0, dmax=2.5),
                                pt(0.0, 0.0, 3.0, dmax=np.nextafter(f32(2.5), down)),
                                pt(0.0, 0.0, 3.0, dmax=np.nextafter(f32(2.5), up))], [kpt(300, 200, 3)]),
                         [0, -1, 0, 0, -1, 0])
    # 4. PO.dot(Pn) < 0.5*dist3D: (0, 0, 2), 0.5 * dist = 1.0; normal z = 0.5 gives exactly 1.0, not below
    out["angle_edges"] = (build([pt(0.0, 0.0, 2.0, normal=(0.0, 0.0, 0.5)),
                                 pt(0.0, 0.0, 2.0, normal=(0.0, 0.0, np.nextafter(f32(0.5), down))),
                                 pt(0.0, 0.0, 2.0, normal=(0.0, 0.0, np.nextafter(f32(0.5), up)))],
                                [kpt(300, 200, 3)]), [0, -1, 0])
    # 5. octaves [L-1, L]: L = 3 (radius 5.18) takes octaves 2 and 3; octave 4 = L + 1 and octave 1 = L - 2 carry
    #    the better descriptors and are not looked at
    #    (e2 = 7.25 on octave 2: 7.25 / 1.44^2 = 3.5 passes the mono gate)
    out["octaves"] = (build([pt(0.0, 0.0, level=3)], [kpt(301, 200, 1, octave=4), kpt(302, 200, 2, octave=1),
                                                      kpt(303, 200, 20, octave=3), kpt(302.5, 201, 9, octave=2)]), [3])
    #    L = 0: lo = -1, octave 0 only
    out["level_zero"] = (build([pt(0.0, 0.0)], [kpt(301, 200, 1, octave=1), kpt(302, 200, 20, octave=0)]), [1])
    #    mfMaxDistance = d * 1.2^9.5 predicts level 10, clamped to n_levels - 1 = 7 (radius 10.75): octaves 6 and 7
    out["level_top"] = (build([pt(0.0, 0.0, level=10)], [kpt(301, 200, 1, octave=5), kpt(302, 200, 20, octave=6),
                                                         kpt(303, 200, 30, octave=7)]), [1])
    # 6. GetFeaturesInArea's window is strict: with th = 2 (radius 2, edge e2 = 4 passes the mono gate) the
    #    keypoints at |dx| == 2 and |dy| == 2 are outside, their neighbouring floats inside
    out["window_edge"] = (build([pt(0.0, 0.0), pt(1.0, 0.0)],
                                [kpt(302, 200, 1), kpt(np.nextafter(f32(302), down), 200, 9),
                                 kpt(400, 202, 1), kpt(400, np.nextafter(f32(198), up), 9)], th=2.0), [1, 3])
    # 7. the ceil cell: (u + r) / 11.75 = 303 / 11.75 = 25.79, so the window's columns end at ceil = 26; the
    #    keypoint at x = 302 is in column round(25.70) = 26, which floor would not reach
    out["ceil_cell"] = (build([pt(0.0, 0.0)], [kpt(302, 200, 3)]), [0])
    # 8. the mono gate, e2 * 1 > 5.99: keypoint 0 at the last x with e2 <= 5.99 passes, keypoint 1 one float further
    #    out carries the better descriptor and is rejected
    kx_in, kx_out = last_float_where(300.0 - 2.4, 290.0, lambda kx: float(_e2_mono(kx)) <= 5.99)
    assert float(_e2_mono(kx_in)) <= 5.99 < float(_e2_mono(kx_out)) and kx_out == np.nextafter(kx_in, down)
    out["mono_gate"] = (build([pt(0.0, 0.0)], [kpt(kx_in, 200, 9), kpt(kx_out, 200, 1)]), [0])
    #    the stereo gate, e2 > 7.8, with er = 0 (ur = 300 - 40 = 260)
    sx_in, sx_out = last_float_where(300.0 - 2.7, 290.0, lambda kx: float(_e2_mono(kx)) <= 7.8)
    assert float(_e2_mono(sx_in)) <= 7.8 < float(_e2_mono(sx_out)) and abs(300.0 - float(sx_out)) < 3.0
    out["stereo_gate"] = (build([pt(0.0, 0.0)], [kpt(sx_in, 200, 9, ur=260.0), kpt(sx_out, 200, 1, ur=260.0)]), [0])
    #    ex = 2.5: e2 = 6.25 is between the two bounds: the monocular keypoint is rejected, the stereo one kept
    out["between_gates"] = (build([pt(0.0, 0.0)], [kpt(297.5, 200, 1), kpt(302.5, 200, 9, ur=260.0)]), [1])
    #    er alone: ex = ey = 0, ur - kpr = 3 -> e2 = 9 > 7.8 rejected; er = 2 -> 4 kept
    out["er_alone"] = (build([pt(0.0, 0.0)], [kpt(300, 200, 1, ur=257.0), kpt(300, 200, 9, ur=258.0)]), [1])
    #    mvuRight >= 0: +0 and -0 are stereo.  With ur = 260 their er = 260 rejects them although ex = 1 would pass
    #    the mono gate (a `> 0` test would take keypoint 0)
    out["uright_zero_rejects"] = (build([pt(0.0, 0.0)], [kpt(301, 200, 1, ur=0.0), kpt(299, 200, 2, ur=-0.0),
                                                         kpt(300, 201, 30)]), [2])
    #    and with mbf = 300 (ur = 0, er = 0) ex = 2.5 passes only because they are stereo
    out["uright_pzero_accepts"] = (build([pt(0.0, 0.0)], [kpt(302.5, 200, 9, ur=0.0)], mbf=300.0), [0])
    out["uright_nzero_accepts"] = (build([pt(0.0, 0.0)], [kpt(302.5, 200, 9, ur=-0.0)], mbf=300.0), [0])
    # 9. bestDist <= TH_LOW: 50 bits kept, 51 dropped
    out["cutoff"] = (build([pt(0.0, 0.0), pt(2.0, 0.0)], [kpt(300, 200, 50), kpt(500, 200, 51)]), [0, -1])
    # 10. ties go to the first keypoint in visiting order.  Level 7 (radius 10.75, invSigma2 = 0.078: e2 up to 76
    #     passes), 80 keypoints of octave 7 in row 20: 0..39 in column 25 (x < 299.6), 40..79 in column 26, so the
    #     visiting rank is the index, and a 16-lane stride gives rank k of a column to lane k % 16.  The minimum 7
    #     sits on 34 (column 25, lane 2, third trip), 41 (column 26, lane 1, first trip) and 65: the answer is 34
    def crowd(best):
        return [kpt(293 + 0.15 * k if k < 40 else 300 + 0.17 * (k - 40), 196 + 2 * (k % 5), best.get(k, 30), octave=7)
                for k in range(80)]
    out["tie_stride"] = (build([pt(0.0, 0.0, level=10)], crowd({34: 7, 41: 7, 65: 7})), [34])
    #     55 (column 26, rank 15: lane 15) and 56 (rank 16: lane 0, second trip): the answer is 55
    out["tie_lane_wrap"] = (build([pt(0.0, 0.0, level=10)], crowd({55: 7, 56: 7})), [55])
    #     across the column change: 40 (first of column 26) and 39 (last of column 25, lane 7): 39
    out["tie_column"] = (build([pt(0.0, 0.0, level=10)], crowd({40: 7, 39: 7})), [39])
    # 11. the window misses the grid: with mnMaxX = 800 the point at u = 790 is in the image, and
    #     floor((790 - 3) / 11.75) = 66 >= 64 columns; an empty window elsewhere
    out["window_off_grid"] = (build([pt(4.9, 0.0), pt(1.0, 1.0)], [kpt(300, 200, 3)], max_x=800.0), [-1, -1])
    # 12. skip (isBad() || IsInKeyFrame at launch) and a view state of 2; the third point matches
    out["skipped"] = (build([pt(0.0, 0.0, skip=1), pt(1.0, 0.0, state=2), pt(2.0, 0.0)],
                            [kpt(300, 200, 3), kpt(400, 200, 3), kpt(500, 200, 3)]), [-1, -1, 2])
    # 13. Ow is the stored camera centre: with Ow = (0, 0, -1) under the identity pose, PO = (0, 0, 2) for (0, 0, 1).
    #     Point 0 (dmax 1, the distance from -R^T t) is out of range at dist 2; point 1 (dmin 2: 0.8 dmin = 1.6) is
    #     in range at dist 2 and would be too near at dist 1
    out["ow_stored"] = (build([pt(0.0, 0.0, dmax=1.0), pt(0.0, 0.0, dmax=2.0, dmin=2.0)], [kpt(300, 200, 3)],
                              Ow=(0.0, 0.0, -1.0)), [-1, 0])
    # 14. no claims: both points take keypoint 0
    out["no_claims"] = (build([pt(0.0, 0.0), pt(0.0, 0.0)], [kpt(301, 200, 2), kpt(302, 200, 30)]), [0, 0])
    return out


# ---- random crowded problems --------------------------------------------------------------------------------
RANDOM_SEEDS = {"random_a": 21, "random_b": 22}


def random_problem(seed: int, n_kf: int = 600, n_points: int = 1500, n_poses: int = 3, stereo_frac: float = 0.3):
    """A crowded KeyFrame / point list (rsc.synth.make_loop_projection_problem), 30 % of the keypoints stereo with
    a right coordinate consistent with a depth of 3..9 m plus noise, seen from n_poses nearby poses.  Returns
    (pts, [kf per pose], skip per pose)."""
    rng = np.random.default_rng(seed)
    p = synth.make_loop_projection_problem(rng, n_kf, n_points, n_clusters=24)
    k0 = p.kf
    z = rng.uniform(3, 9, n_kf)
    ur = (k0.kp[:, 0] - MBF / z + rng.normal(0, 1.5, n_kf)).astype(f32)
    ur = np.where(rng.random(n_kf) < stereo_frac, np.maximum(ur, 0.0), -1.0).astype(f32)
    kfs, skips = [], []
    for k in range(n_poses):
        R = synth.random_rotation(rng, 0.004 * k) @ np.asarray(k0.Rcw, np.float64)
        t = np.asarray(k0.tcw, np.float64) + rng.normal(0, 0.004 * k, 3)
        kfs.append(make_kf(k0.kp, k0.octave, k0.desc, ur, R, t))
        skips.append((rng.random(n_points) < 0.08).astype(np.uint8))
    return p.pts, kfs, skips


# ---- fixture packing (tests/golden/fusekf_traces.npz) -------------------------------------------------------
_PT = ("state", "pos", "normal", "dmax", "dmin", "desc")


def pts_to_arrays(pts, prefix):
    return {f"{prefix}/pt_{k}": np.asarray(getattr(pts, k)) for k in _PT}


def pts_from_arrays(z, prefix):
    return kr.points_of(**{k: z[f"{prefix}/pt_{k}"] for k in _PT})


def kf_to_arrays(kf, prefix):
    return {f"{prefix}/kp": kf.kp, f"{prefix}/octave": kf.octave, f"{prefix}/desc": kf.desc,
            f"{prefix}/u_right": kf.u_right, f"{prefix}/Rcw": np.asarray(kf.Rcw, f32),
            f"{prefix}/tcw": np.asarray(kf.tcw, f32), f"{prefix}/Ow": np.asarray(kf.Ow, f32),
            f"{prefix}/K": np.array([kf.fx, kf.fy, kf.cx, kf.cy, kf.max_x, kf.mbf], np.float64)}


def kf_from_arrays(z, prefix, shared=None):
    """shared: the prefix whose keypoint arrays this KeyFrame uses (the random problems store them once)."""
    s = prefix if shared is None else shared
    fx, fy, cx, cy, max_x, mbf = (float(v) for v in z[f"{prefix}/K"])
    return make_kf(z[f"{s}/kp"], z[f"{s}/octave"], z[f"{s}/desc"], z[f"{s}/u_right"], z[f"{prefix}/Rcw"],
                   z[f"{prefix}/tcw"], z[f"{prefix}/Ow"], mbf, fx=fx, fy=fy, cx=cx, cy=cy, max_x=max_x)
