"""Hand-built SearchByProjection problems with known answers (TEST-ONLY), one per rule of
src/ORBmatcher.cpp:1317-1444, shared by the CPU tests, the GPU tests and the golden fixture.

Geometry that can be checked by hand: identity pose, fx = fy = 100, cx = 300, cy = 200, MapPoints at
z = +-1 so that u = 100 x + 300 and v = 100 y + 200 exactly, image [0, 700] x [0, 480].  A MapPoint at
distance d with mfMaxDistance = d * 1.2^(L - 0.5) predicts level L (ceil(L - 0.5)); the search radius is
th * 1.2^L.  Descriptors: a MapPoint's is all zeros, a feature's has its first `bits` bits set, so the
descriptor distance is `bits`.
"""
from __future__ import annotations

import types

import numpy as np

from rsc import synth

FX = FY = 100.0
CX, CY = 300.0, 200.0
MAX_X = 700.0
TH, ORB_DIST = 10.0, 100


def desc_bits(bits: int) -> np.ndarray:
    d = np.zeros(32, np.uint8)
    d[:bits // 8] = 255
    if bits % 8:
        d[bits // 8] = (1 << (bits % 8)) - 1
    return d


def mp(x, y, z=1.0, level=0, state=1, angle=0.0, already=0):
    return dict(pos=(x, y, z), level=level, state=state, angle=angle, already=already)


def feat(u, v, bits, octave=0, angle=0.0, occupied=False):
    return dict(pt=(u, v), bits=bits, octave=octave, angle=angle, occupied=occupied)


def build(mps, feats, check_orientation=True, th=TH, orb_dist=ORB_DIST):
    """A problem namespace: kf, frame, Tcw, already, frame_mp, th, orb_dist, check_orientation."""
    n = len(mps)
    pos = np.array([m["pos"] for m in mps], np.float32).reshape(n, 3)
    dist = np.sqrt((pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]) + pos[:, 2] * pos[:, 2]).astype(np.float32)
    dmax = np.array([d if m["level"] == 0 else np.float32(d * 1.2 ** (m["level"] - 0.5))
                     for d, m in zip(dist, mps)], np.float32)
    kp0 = np.zeros((n, 2), np.float32)
    begin0, feat0 = synth.build_grid(kp0)
    kf = synth.Sim3KF(n, kp0, np.zeros(n, np.int32), np.zeros((n, 32), np.uint8), begin0, feat0,
                      np.eye(3, dtype=np.float32), np.zeros(3, np.float32),
                      np.array([m["state"] for m in mps], np.uint8), pos, dmax, np.full(n, 0.01, np.float32),
                      np.zeros((n, 32), np.uint8), np.arange(n, dtype=np.int64), fx=FX, fy=FY, cx=CX, cy=CY)
    kf.angle = np.array([m["angle"] for m in mps], np.float32)
    frame = synth.make_proj_frame(np.array([f["pt"] for f in feats], np.float32).reshape(-1, 2),
                                  [f["octave"] for f in feats], [f["angle"] for f in feats],
                                  np.array([desc_bits(f["bits"]) for f in feats], np.uint8).reshape(-1, 32),
                                  fx=FX, fy=FY, cx=CX, cy=CY, max_x=MAX_X)
    frame_mp = np.array([0 if f["occupied"] else -1 for f in feats], np.int32)
    already = np.array([m["already"] for m in mps], np.uint8)
    return types.SimpleNamespace(kf=kf, frame=frame, Tcw=np.eye(4, dtype=np.float32), already=already,
                                 frame_mp=frame_mp, th=th, orb_dist=orb_dist, check_orientation=check_orientation)


def _filler(n, u0, rot=0.0):
    """n MapPoints in a row at v = 400 (y = 2) with one feature each: matches with rotation `rot`."""
    mps = [mp((u0 + 30 * k - 300) / 100.0, 2.0, angle=rot) for k in range(n)]
    feats = [feat(u0 + 30 * k, 400, 5) for k in range(n)]
    return mps, feats


def cases():
    """name -> (problem, expected {feature: KeyFrame slot}).  Expected values are worked out in the
    comments, not computed."""
    out = {}
    # 1. u == mnMaxX is inside (u > mnMaxX rejects): x = 4 -> u = 700 = MAX_X, feature 1 px left of it;
    #    x = 4.25 -> u = 725 > 700: skipped although feature 1 sits 1 px from its projection
    out["bound_inclusive"] = (build([mp(4.0, 0.0), mp(4.25, 0.0)], [feat(699, 200, 3), feat(724, 200, 3)]),
                              {0: 0})
    # 2. no z > 0 test: (-1, 0, -1) -> invz = -1, u = (100 * -1) * -1 + 300 = 400, v = 200
    out["behind_camera"] = (build([mp(-1.0, 0.0, -1.0)], [feat(400, 200, 3)]), {0: 0})
    # 3. bestDist <= ORBdist: 100 bits accepted, 101 rejected
    out["orb_dist_edge"] = (build([mp(0.0, 0.0), mp(2.0, 0.0)], [feat(300, 200, 100), feat(500, 200, 101)]),
                            {0: 0})
    # 4. level window [L-1, L+1]: L = 0 takes octaves 0 and 1, not 2 (the better descriptor sits on
    #    octave 2); L = 7 takes 6 and 7, not 5
    out["level_window_low"] = (build([mp(0.0, 0.0, level=0)],
                                     [feat(301, 200, 1, octave=2), feat(302, 200, 9, octave=1),
                                      feat(303, 200, 20, octave=0)]), {1: 0})
    out["level_window_high"] = (build([mp(0.0, 0.0, level=7)],
                                      [feat(301, 200, 1, octave=5), feat(302, 200, 9, octave=6),
                                       feat(303, 200, 20, octave=7)]), {1: 0})
    # 5. fabs(dx) < r is strict: r = 10; a feature at exactly +10 px is outside, one at +9 inside
    out["radius_strict"] = (build([mp(0.0, 0.0), mp(2.0, 0.0)], [feat(310, 200, 3), feat(509, 200, 3)]), {1: 1})
    # 6. the best feature is occupied before the call: the second best is taken
    out["occupied_best"] = (build([mp(0.0, 0.0)], [feat(301, 200, 2, occupied=True), feat(302, 200, 30)]), {1: 0})
    # 7. every candidate occupied: no match
    out["occupied_all"] = (build([mp(0.0, 0.0)], [feat(301, 200, 2, occupied=True),
                                                  feat(302, 200, 30, occupied=True)]), {})
    # 8. sAlreadyFound, NULL and bad MapPoints are skipped; the fourth point matches
    out["skipped_points"] = (build([mp(0.0, 0.0, already=1), mp(1.0, 0.0, state=0), mp(2.0, 0.0, state=2),
                                    mp(3.0, 0.0)],
                                   [feat(300, 200, 3), feat(400, 200, 3), feat(500, 200, 3), feat(600, 200, 3)]),
                             {3: 3})
    # 9. rotation check: 11 matches with rot = 0 (bin 0) and one with rot = 90 (bin round(90 / 30) = 3):
    #    max2 = 1 < 0.1 * 11, so only bin 0 survives and match 11 is removed; kept without the check
    for name, chk in (("rotation_removed", True), ("rotation_unchecked", False)):
        mps, feats = _filler(11, 30)
        mps.append(mp(0.0, 0.0, angle=90.0))
        feats.append(feat(300, 200, 3))
        exp = {k: k for k in range(11)}
        if not chk:
            exp[11] = 11
        out[name] = (build(mps, feats, check_orientation=chk), exp)
    # 10. greedy order: both MapPoints are nearest to feature 0; slot 0 takes it, slot 1 the other
    out["greedy_order"] = (build([mp(0.0, 0.0), mp(0.0, 0.0)], [feat(301, 200, 2), feat(302, 200, 30)]),
                           {0: 0, 1: 1})
    return out


def domino(k: int = 70):
    """k MapPoints on slots 0..k-1 at one position with one descriptor, k + 2 features around the
    projection whose distances are 1, 2, ...: every MapPoint prefers feature 0, then 1, ... so MapPoint
    j ends on feature j, and the fixed point needs a round per displacement (k + 1 in all)."""
    mps = [mp(0.0, 0.0) for _ in range(k)]
    feats = [feat(296 + (j % 9), 196 + (j // 9), j + 1) for j in range(k + 2)]
    return build(mps, feats), {j: j for j in range(k)}


def expected_out(problem, exp) -> np.ndarray:
    out = np.full(problem.frame.n, -1, np.int32)
    for f, s in exp.items():
        out[f] = s
    return out


# ---- fixture packing (tests/golden/frameproj_traces.npz) -------------------------------------------
_KF = ("mp_state", "mp_pos", "mp_dmax", "mp_dmin", "mp_desc", "angle")
_FR = ("kp", "octave", "angle", "desc")


def to_arrays(p, prefix: str) -> dict:
    d = {f"{prefix}/kf_{k}": np.asarray(getattr(p.kf, k)) for k in _KF}
    d.update({f"{prefix}/fr_{k}": np.asarray(getattr(p.frame, k)) for k in _FR})
    d[f"{prefix}/K"] = np.array([p.frame.fx, p.frame.fy, p.frame.cx, p.frame.cy, p.frame.max_x], np.float64)
    d[f"{prefix}/Tcw"] = np.asarray(p.Tcw, np.float32)
    d[f"{prefix}/already"] = np.asarray(p.already, np.uint8)
    d[f"{prefix}/frame_mp"] = np.asarray(p.frame_mp, np.int32)
    d[f"{prefix}/call"] = np.array([p.th, p.orb_dist, int(p.check_orientation)], np.float64)
    return d


def from_arrays(z, prefix: str):
    g = lambda k: z[f"{prefix}/{k}"]
    n = len(g("kf_mp_state"))
    fx, fy, cx, cy, max_x = (float(v) for v in g("K"))
    kp0 = np.zeros((n, 2), np.float32)
    begin0, feat0 = synth.build_grid(kp0)
    kf = synth.Sim3KF(n, kp0, np.zeros(n, np.int32), np.zeros((n, 32), np.uint8), begin0, feat0,
                      np.eye(3, dtype=np.float32), np.zeros(3, np.float32), g("kf_mp_state"), g("kf_mp_pos"),
                      g("kf_mp_dmax"), g("kf_mp_dmin"), g("kf_mp_desc"), np.arange(n, dtype=np.int64),
                      fx=fx, fy=fy, cx=cx, cy=cy)
    kf.angle = g("kf_angle")
    frame = synth.make_proj_frame(g("fr_kp"), g("fr_octave"), g("fr_angle"), g("fr_desc"), fx=fx, fy=fy, cx=cx,
                                  cy=cy, max_x=max_x)
    th, od, chk = g("call")
    return types.SimpleNamespace(kf=kf, frame=frame, Tcw=g("Tcw"), already=g("already"), frame_mp=g("frame_mp"),
                                 th=float(th), orb_dist=int(od), check_orientation=bool(chk))


def random_problem(seed: int, n_kf: int, n_frame: int, th: float, orb_dist: int, **kw):
    """A random crowded problem (rsc.synth.make_reloc_projection_problem) as a problem namespace."""
    p = synth.make_reloc_projection_problem(np.random.default_rng(seed), n_kf, n_frame, **kw)
    return types.SimpleNamespace(kf=p.kf, frame=p.frame, Tcw=p.Tcw, already=p.already, frame_mp=p.frame_mp,
                                 th=float(th), orb_dist=int(orb_dist), check_orientation=True)
