"""Hand-built problems with known answers for the loop-closing matchers (TEST-ONLY), one per rule of
ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cpp:241-352) and
ORBmatcher::Fuse (:823-946), shared by the CPU tests, the GPU tests and the golden fixture.

Geometry that can be checked by hand: identity Scw, fx = fy = 100, cx = 300, cy = 200, so a point (x, y, z)
projects to u = 100 x / z + 300, v = 100 y / z + 200 and Ow = 0, PO = the point itself; image
[0, 700) x [0, 480).  A point at distance d with mfMaxDistance = d * 1.2^(L - 0.5) predicts level L (level 0:
mfMaxDistance = d); the search radius is 10 * 1.2^L.  The default normal (0, 0, 10) passes the viewing-angle
test for every d <= 20.  Descriptors: a point's is all zeros, a keypoint's has its first `bits` bits set, so
the descriptor distance is `bits`.
"""
from __future__ import annotations

import types

import numpy as np

import kfproj_ref as kr
from rsc import synth

f32 = np.float32
FX = FY = 100.0
CX, CY = 300.0, 200.0
MAX_X = 700.0
TH = 10


def desc_bits(bits: int, lo: int = 0) -> np.ndarray:
    """bits [lo, lo + bits) set."""
    d = np.zeros(32, np.uint8)
    for b in range(lo, lo + bits):
        d[b // 8] |= 1 << (b % 8)
    return d


def pt(x, y, z=1.0, level=0, state=1, already=0, normal=(0.0, 0.0, 10.0), dmax=None, dmin=0.01, desc=None, in_kf=0):
    return dict(pos=(x, y, z), level=level, state=state, already=already, normal=normal, dmax=dmax, dmin=dmin,
                desc=desc, in_kf=in_kf)


def kpt(u, v, bits, octave=0, occupied=False, mp_state=0, desc=None):
    return dict(pt=(u, v), bits=bits, octave=octave, occupied=occupied, mp_state=mp_state, desc=desc)


def make_kf(kp, octave, desc, mp_state=None, R=None, t=None, **kw) -> synth.Sim3KF:
    """A KeyFrame view from its keypoint side; mp_state: the KeyFrame's own slots (Fuse's bookkeeping)."""
    kp = np.ascontiguousarray(kp, f32).reshape(-1, 2)
    n = len(kp)
    begin, feat = synth.build_grid(kp)
    kf = synth.Sim3KF(n, kp, np.ascontiguousarray(octave, np.int32), np.ascontiguousarray(desc, np.uint8).reshape(n, 32),
                      begin, feat, np.eye(3, dtype=f32) if R is None else np.asarray(R, f32),
                      np.zeros(3, f32) if t is None else np.asarray(t, f32),
                      np.zeros(n, np.uint8) if mp_state is None else np.asarray(mp_state, np.uint8),
                      np.zeros((n, 3), f32), np.zeros(n, f32), np.zeros(n, f32), np.zeros((n, 32), np.uint8),
                      np.full(n, -1, np.int64), **kw)
    return kf


def build(pts, kps, Scw=None, th=TH):
    """A problem namespace: kf, pts, Scw, already, occupied, in_kf, th."""
    n = len(pts)
    pos = np.array([p["pos"] for p in pts], f32).reshape(n, 3)
    dist = np.sqrt((pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]) + pos[:, 2] * pos[:, 2]).astype(f32)
    dmax = np.array([p["dmax"] if p["dmax"] is not None else
                     (d if p["level"] == 0 else f32(d * 1.2 ** (p["level"] - 0.5))) for d, p in zip(dist, pts)], f32)
    P = kr.points_of(state=[p["state"] for p in pts], pos=pos, normal=[p["normal"] for p in pts], dmax=dmax,
                     dmin=[p["dmin"] for p in pts],
                     desc=[np.zeros(32, np.uint8) if p["desc"] is None else p["desc"] for p in pts])
    kf = make_kf([k["pt"] for k in kps], [k["octave"] for k in kps],
                 [desc_bits(k["bits"]) if k["desc"] is None else k["desc"] for k in kps],
                 [k["mp_state"] for k in kps], fx=FX, fy=FY, cx=CX, cy=CY, max_x=MAX_X)
    return types.SimpleNamespace(kf=kf, pts=P, Scw=np.eye(4, dtype=f32) if Scw is None else np.asarray(Scw, f32),
                                 already=np.array([p["already"] for p in pts], np.uint8),
                                 occupied=np.array([int(k["occupied"]) for k in kps], np.uint8),
                                 in_kf=np.array([p["in_kf"] for p in pts], np.uint8), th=th)


def cases():
    """name -> (problem, expected {keypoint: point}).  Expected values are worked out in the comments, not
    computed."""
    out = {}
    # 1. z < 0 is rejected (:276): (0, 0, -1) would project to u = 300 where keypoint 0 waits; (1, 0, 1) -> 400
    out["z_negative"] = (build([pt(0.0, 0.0, -1.0), pt(1.0, 0.0)], [kpt(300, 200, 3), kpt(400, 200, 3)]), {1: 1})
    # 2. z == 0: invz = inf; (1, 0, 0) -> u = inf, (0, 0, 0) -> 0 * inf = NaN: IsInImage is false for both
    out["z_zero"] = (build([pt(1.0, 0.0, 0.0), pt(0.0, 0.0, 0.0), pt(1.0, 0.0)],
                           [kpt(300, 200, 3), kpt(400, 200, 3)]), {1: 2})
    # 3. IsInImage: x = 4 -> u = 700 = mnMaxX is outside (a keypoint sits 1 px left of it); x = -3 -> u = 0 =
    #    mnMinX is inside and takes the keypoint at (1, 200)
    out["bound_exclusive"] = (build([pt(4.0, 0.0), pt(-3.0, 0.0)], [kpt(699, 200, 3), kpt(1, 200, 3)]), {1: 1})
    # 4. dist in [0.8 dmin, 1.2 dmax], both ends inside.  (0, 0, 2): dist = 2; 0.8f * 2.5 = 2.00000003 rounds
    #    to 2.0 = dist: not below, accepted; with the next float above 2.5 the bound is 2.0000002 > dist
    out["dist_min_edge"] = (build([pt(0.0, 0.0, 2.0, dmin=2.5)], [kpt(300, 200, 3)]), {0: 0})
    out["dist_min_below"] = (build([pt(0.0, 0.0, 2.0, dmin=np.nextafter(f32(2.5), f32(3)))], [kpt(300, 200, 3)]), {})
    #    (0, 0, 3): dist = 3; 1.2f * 2.5 = 3 + 2^-23 exactly, a tie that rounds to even = 3.0 = dist: not above,
    #    accepted (level: ratio < 1 -> 0); with the next float below 2.5 the bound is 2.9999998 < dist
    out["dist_max_edge"] = (build([pt(0.0, 0.0, 3.0, dmax=2.5)], [kpt(300, 200, 3)]), {0: 0})
    out["dist_max_above"] = (build([pt(0.0, 0.0, 3.0, dmax=np.nextafter(f32(2.5), f32(0)))], [kpt(300, 200, 3)]), {})
    # 5. viewing angle: (0, 0, 2), 0.5 * dist = 1.0; normal (0, 0, 0.5): PO.Pn = 1.0, not below: accepted; one
    #    ulp less, 2 * 0.49999997 = 0.99999994 < 1.0: rejected
    out["angle_edge"] = (build([pt(0.0, 0.0, 2.0, normal=(0.0, 0.0, 0.5))], [kpt(300, 200, 3)]), {0: 0})
    out["angle_below"] = (build([pt(0.0, 0.0, 2.0, normal=(0.0, 0.0, np.nextafter(f32(0.5), f32(0))))],
                                [kpt(300, 200, 3)]), {})
    # 6. levels [L-1, L]: L = 0 takes octave 0 only (the better descriptor sits on octave 1)
    out["level_zero"] = (build([pt(0.0, 0.0, level=0)], [kpt(301, 200, 1, octave=1), kpt(302, 200, 20, octave=0)]),
                         {1: 0})
    #    L = 3 takes octaves 2 and 3; octave 4 = L + 1 (accepted by the Frame matcher) and octave 1 are not
    out["level_above"] = (build([pt(0.0, 0.0, level=3)],
                                [kpt(301, 200, 1, octave=4), kpt(302, 200, 9, octave=3), kpt(303, 200, 20, octave=2),
                                 kpt(304, 200, 2, octave=1)]), {1: 0})
    # 7. vpMatched[idx] set on entry: the best keypoint is skipped, the second best taken
    out["occupied_on_entry"] = (build([pt(0.0, 0.0)], [kpt(301, 200, 2, occupied=True), kpt(302, 200, 30)]), {1: 0})
    # 8. a point already in vpMatched and a bad point are skipped; the third point matches
    out["skipped_points"] = (build([pt(0.0, 0.0, already=1), pt(1.0, 0.0, state=2), pt(2.0, 0.0)],
                                   [kpt(300, 200, 3), kpt(400, 200, 3), kpt(500, 200, 3)]), {2: 2})
    # 9. bestDist <= TH_LOW: 50 bits kept, 51 dropped
    out["cutoff"] = (build([pt(0.0, 0.0), pt(2.0, 0.0)], [kpt(300, 200, 50), kpt(500, 200, 51)]), {0: 0})
    # 10. a tie goes to the first keypoint in visiting order, which is cell order, not index order: grid cells
    #     are 11.75 px wide and PosInGrid rounds, so (305, 200) is in column 26 and (295, 200) in column 25,
    #     visited first
    out["tie_visiting_order"] = (build([pt(0.0, 0.0)], [kpt(305, 200, 7), kpt(295, 200, 7)]), {1: 0})
    # 11. greedy order: both points are nearest to keypoint 0; point 0 takes it, point 1 the other
    out["greedy_order"] = (build([pt(0.0, 0.0), pt(0.0, 0.0)], [kpt(301, 200, 2), kpt(302, 200, 30)]), {0: 0, 1: 1})
    return out


def fuse_cases():
    """name -> (problem, expected dict(best_idx, replace, added) as lists over the points)."""
    out = {}
    # 1. s = 2, Scw = [2 I | (2, 0, 0)]: Rcw = I, tcw = (1, 0, 0), Ow = (-1, 0, 0).  (0, 0, 1) -> camera
    #    (1, 0, 1), u = 400; PO = (1, 0, 1), dist = sqrt(2) = mfMaxDistance.  Without the division by s the
    #    point would be at dist sqrt(5) > 1.2 sqrt(2) and be rejected
    S = np.eye(4, dtype=f32)
    S[:3, :3] *= 2.0
    S[0, 3] = 2.0
    out["scale_two"] = (build([pt(0.0, 0.0, 1.0, dmax=f32(np.sqrt(f32(2.0))))], [kpt(400, 200, 3)], Scw=S),
                        dict(best_idx=[0], replace=[-1], added=[0]))
    # 2. the slot of the best keypoint: a good MapPoint -> vpReplacePoint; a bad one -> neither, still
    #    counted; empty -> AddObservation / AddMapPoint.  A point of the KeyFrame's own and a bad one are skipped
    out["slots"] = (build([pt(0.0, 0.0), pt(1.0, 0.0), pt(2.0, 0.0), pt(3.0, 0.0, in_kf=1), pt(-1.0, 0.0, state=2)],
                          [kpt(300, 200, 3, mp_state=1), kpt(400, 200, 3, mp_state=2), kpt(500, 200, 3),
                           kpt(600, 200, 3), kpt(200, 200, 3)]),
                    dict(best_idx=[0, 1, 2, -1, -1], replace=[0, -1, -1, -1, -1], added=[-1, -1, 2, -1, -1]))
    # 3. Fuse never skips a keypoint: two points take the same best keypoint.  The first is added to the empty
    #    slot (AddMapPoint), so the second finds it there and gets it as its vpReplacePoint
    out["no_claims"] = (build([pt(0.0, 0.0), pt(0.0, 0.0)], [kpt(301, 200, 2), kpt(302, 200, 30)]),
                        dict(best_idx=[0, 0], replace=[-1, 0], added=[0, -1]))
    return out


def domino(k: int = 40):
    """k points in a row 9 px apart with keypoint j 3 px right of point j's projection: point i sees keypoints
    i - 1 (6 px left) and i (3 px right) and no other (radius 10, strict).  Keypoint j has bits [0, 3 j) set
    and point i bits [0, 3 i - 2), so point i is at distance 1 from keypoint i - 1 (its best, which point i - 1
    owns) and 2 from keypoint i (its own).  Sequentially point i ends on keypoint i; in round 1 every point
    i >= 1 chooses keypoint i - 1, and the correction moves one point per round: k + 1 rounds."""
    pts = [pt((20 + 9 * i - 300) / 100.0, 0.0, desc=desc_bits(max(3 * i - 2, 0))) for i in range(k)]
    kps = [kpt(23 + 9 * j, 200, 0, desc=desc_bits(3 * j)) for j in range(k)]
    return build(pts, kps), {j: j for j in range(k)}


def expected_out(problem, exp) -> np.ndarray:
    out = np.full(problem.kf.n, -1, np.int32)
    for f, s in exp.items():
        out[f] = s
    return out


def random_problem(seed: int, n_kf: int = 600, n_points: int = 1500, **kw):
    """A random crowded problem (rsc.synth.make_loop_projection_problem) as a problem namespace."""
    p = synth.make_loop_projection_problem(np.random.default_rng(seed), n_kf, n_points, **kw)
    return types.SimpleNamespace(kf=p.kf, pts=p.pts, Scw=p.Scw, already=p.already, occupied=p.occupied,
                                 in_kf=p.already, th=p.th)


RANDOM_SEEDS = {"random_a": 11, "random_b": 12}  # chosen so that make_kfproj_golden.py's conditions hold


def fuse_batch(p, n_kfs: int = 5, seed: int = 5):
    """n_kfs (Scw, in_kf) pairs against p.pts for one KeyFrame each: the problem's KeyFrame seen through
    s * (a small motion of Scw), s != 1.  Returns [(kf, Scw float32 [4,4], in_kf uint8)]."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_kfs):
        s = 1.0 + 0.1 * (k - 2)
        T = np.asarray(p.Scw, np.float64).copy()
        T[:3, :3] = synth.random_rotation(rng, 0.002 * k) @ T[:3, :3]
        T[:3, 3] += rng.normal(0, 0.002 * k, 3)
        T[:3, :] *= s
        kf = make_kf(p.kf.kp, p.kf.octave, p.kf.desc, (rng.random(p.kf.n) < 0.5).astype(np.uint8))
        out.append((kf, T.astype(f32), (rng.random(p.pts.n) < 0.1).astype(np.uint8)))
    return out


# ---- fixture packing (tests/golden/kfproj_traces.npz) -----------------------------------------------
_PT = ("state", "pos", "normal", "dmax", "dmin", "desc")
_KF = ("kp", "octave", "desc", "mp_state")


def to_arrays(p, prefix: str) -> dict:
    d = {f"{prefix}/pt_{k}": np.asarray(getattr(p.pts, k)) for k in _PT}
    d.update({f"{prefix}/kf_{k}": np.asarray(getattr(p.kf, k)) for k in _KF})
    d[f"{prefix}/K"] = np.array([p.kf.fx, p.kf.fy, p.kf.cx, p.kf.cy, p.kf.max_x], np.float64)
    d[f"{prefix}/Scw"] = np.asarray(p.Scw, f32)
    d[f"{prefix}/already"] = np.asarray(p.already, np.uint8)
    d[f"{prefix}/occupied"] = np.asarray(p.occupied, np.uint8)
    d[f"{prefix}/in_kf"] = np.asarray(p.in_kf, np.uint8)
    d[f"{prefix}/th"] = np.array([p.th], np.int32)
    return d


def from_arrays(z, prefix: str):
    g = lambda k: z[f"{prefix}/{k}"]
    fx, fy, cx, cy, max_x = (float(v) for v in g("K"))
    kf = make_kf(g("kf_kp"), g("kf_octave"), g("kf_desc"), g("kf_mp_state"), fx=fx, fy=fy, cx=cx, cy=cy, max_x=max_x)
    pts = kr.points_of(**{k: g(f"pt_{k}") for k in _PT})
    return types.SimpleNamespace(kf=kf, pts=pts, Scw=g("Scw"), already=g("already"), occupied=g("occupied"),
                                 in_kf=g("in_kf"), th=int(g("th")[0]))
