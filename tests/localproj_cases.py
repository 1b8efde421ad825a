"""Hand-built problems with known answers for Tracking::SearchLocalPoints (TEST-ONLY), one per rule of
Frame::isInFrustum (src/Frame.cpp:336-392) and ORBmatcher::SearchByProjection(Frame&, vector<MapPoint>&, th)
(src/ORBmatcher.cpp:16-100), shared by the CPU tests, the GPU tests, the facade test and the golden fixture.

Geometry that can be checked by hand: identity Tcw, fx = fy = 100, cx = 300, cy = 200, mbf = 40, so a point
(x, y, z) projects to u = 100 x / z + 300, v = 100 y / z + 200, xr = u - 40 / z, and Ow = 0, PO = the point
itself; image [0, 700] x [0, 480], both ends inside.  A point at distance d with mfMaxDistance = d * 1.2^(L -
0.5) predicts level L (level 0: mfMaxDistance = d).  The default normal is the point itself, so viewCos = d
(above 0.998 for every d >= 1): radius 2.5 * th * 1.2^L.  A normal (0, 0, c) on a point (0, 0, 1) gives
viewCos = c exactly.  Descriptors: a point's is all zeros, a feature's has its first `bits` bits set, so the
descriptor distance is `bits`.  Features are monocular (u_right = -1) unless stated.  The grid cells are
11.75 px wide and PosInGrid rounds, so x = 298 and 299 are in column 25 and x = 301 in column 26: the
visiting order is 298, 299 (cell order = index order), then 301.
"""
from __future__ import annotations

import types

import numpy as np

import kfproj_ref as kr
import localproj_ref as lr
from rsc import synth

f32 = np.float32
FX = FY = 100.0
CX, CY = 300.0, 200.0
MAX_X = 700.0
MBF = 40.0
COS_LIMIT = 0.5
NN_RATIO = 0.8


def up(x, n=1):
    x = f32(x)
    for _ in range(n):
        x = np.nextafter(x, f32(np.inf))
    return x


def down(x, n=1):
    x = f32(x)
    for _ in range(n):
        x = np.nextafter(x, f32(-np.inf))
    return x


def desc_bits(bits: int, lo: int = 0) -> np.ndarray:
    d = np.zeros(32, np.uint8)
    for b in range(lo, lo + bits):
        d[b // 8] |= 1 << (b % 8)
    return d


def pt(x, y, z=1.0, level=0, state=1, skip=0, has_obs=1, normal=None, dmax=None, dmin=0.01, desc=None):
    return dict(pos=(x, y, z), level=level, state=state, skip=skip, has_obs=has_obs, normal=normal, dmax=dmax,
                dmin=dmin, desc=desc)


def ft(u, v, bits, octave=0, occ=0, ur=-1.0, desc=None):
    return dict(pt=(u, v), bits=bits, octave=octave, occ=occ, ur=ur, desc=desc)


def make_frame(kp, octave, desc, u_right, mbf=MBF, **kw):
    """A Frame namespace: rsc.synth.ProjFrame plus u_right (mvuRight) and mbf."""
    kp = np.ascontiguousarray(kp, f32).reshape(-1, 2)
    fr = synth.make_proj_frame(kp, octave, np.zeros(len(kp), f32), desc, **kw)
    fr.u_right = np.ascontiguousarray(u_right, f32).reshape(-1)
    fr.mbf = float(mbf)
    return fr


def build(pts, fts, th=1.0, Tcw=None):
    """A problem namespace: frame, pts, Tcw, skip, has_obs, frame_occ, cos_limit, th, nn_ratio."""
    n = len(pts)
    pos = np.array([p["pos"] for p in pts], f32).reshape(n, 3)
    dist = np.sqrt((pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]) + pos[:, 2] * pos[:, 2]).astype(f32)
    dmax = np.array([p["dmax"] if p["dmax"] is not None else
                     (d if p["level"] == 0 else f32(d * 1.2 ** (p["level"] - 0.5))) for d, p in zip(dist, pts)], f32)
    P = kr.points_of(state=[p["state"] for p in pts], pos=pos,
                     normal=[p["pos"] if p["normal"] is None else p["normal"] for p in pts], dmax=dmax,
                     dmin=[p["dmin"] for p in pts],
                     desc=[np.zeros(32, np.uint8) if p["desc"] is None else p["desc"] for p in pts])
    fr = make_frame([k["pt"] for k in fts], [k["octave"] for k in fts],
                    [desc_bits(k["bits"]) if k["desc"] is None else k["desc"] for k in fts],
                    [k["ur"] for k in fts], fx=FX, fy=FY, cx=CX, cy=CY, max_x=MAX_X)
    return types.SimpleNamespace(frame=fr, pts=P, Tcw=np.eye(4, dtype=f32) if Tcw is None else np.asarray(Tcw, f32),
                                 skip=np.array([p["skip"] for p in pts], np.uint8),
                                 has_obs=np.array([p["has_obs"] for p in pts], np.uint8),
                                 frame_occ=np.array([k["occ"] for k in fts], np.uint8),
                                 cos_limit=COS_LIMIT, th=float(th), nn_ratio=NN_RATIO)


def E(out, in_view, nmatches=None):
    """expected: out {feature: point}, in_view per point, nmatches (default: len(out))."""
    return dict(out=out, in_view=in_view, nmatches=len(out) if nmatches is None else nmatches)


def cases():
    """name -> (problem, expected).  Expected values are worked out in the comments, not computed."""
    c = {}
    # ---- frustum and skip gates ----
    # z < 0 (:350): (0, 0, -1) would project to u = 300 where feature 0 waits; (1, 0, 1) -> u = 400
    c["z_negative"] = (build([pt(0.0, 0.0, -1.0), pt(1.0, 0.0)], [ft(300, 200, 3), ft(400, 200, 3)]),
                       E({1: 1}, [0, 1]))
    # z == 0 with x != 0: invz = inf, u = +inf > mnMaxX, rejected by the bounds with no special case
    c["z_zero_inf"] = (build([pt(1.0, 0.0, 0.0), pt(1.0, 0.0)], [ft(300, 200, 3), ft(400, 200, 3)]),
                       E({1: 1}, [0, 1]))
    # inclusive bounds (:358): x = -3 -> u = 0 = mnMinX and x = 4 -> u = 700 = mnMaxX are both inside
    c["bound_on"] = (build([pt(-3.0, 0.0), pt(4.0, 0.0)], [ft(1, 200, 3), ft(699, 200, 3)]),
                     E({0: 0, 1: 1}, [1, 1]))
    # one float outside: x = -3 - ulp -> 100 x = -300.00003, u = -0.00003 < 0; x = 4 + ulp -> 100 x = 400.00006,
    # u = 700.00006 > 700
    c["bound_outside"] = (build([pt(down(-3.0), 0.0), pt(up(4.0), 0.0)], [ft(1, 200, 3), ft(699, 200, 3)]),
                          E({}, [0, 0]))
    # dist in [0.8 dmin, 1.2 dmax], both ends inside.  (0, 0, 2): 0.8f * 2.5 rounds to 2.0 = dist, accepted; with
    # the next float above 2.5 the bound is 2.0000002 > dist
    c["dist_min_on"] = (build([pt(0.0, 0.0, 2.0, dmin=2.5)], [ft(300, 200, 3)]), E({0: 0}, [1]))
    c["dist_min_beyond"] = (build([pt(0.0, 0.0, 2.0, dmin=up(2.5))], [ft(300, 200, 3)]), E({}, [0]))
    # (0, 0, 3): 1.2f * 2.5 = 3 + 2^-23, a tie that rounds to even = 3.0 = dist, accepted (ratio < 1: level 0);
    # with the next float below 2.5 the bound is 2.9999998 < dist
    c["dist_max_on"] = (build([pt(0.0, 0.0, 3.0, dmax=2.5)], [ft(300, 200, 3)]), E({0: 0}, [1]))
    c["dist_max_beyond"] = (build([pt(0.0, 0.0, 3.0, dmax=down(2.5))], [ft(300, 200, 3)]), E({}, [0]))
    # viewCos (:375-377): (0, 0, 2) with normal (0, 0, 0.5): dot = 1.0, viewCos = 0.5, not below the limit
    # (radius 4: the feature 3 px away is inside); one ulp less: 0.99999994 / 2 = 0.49999997 < 0.5
    c["viewcos_on"] = (build([pt(0.0, 0.0, 2.0, normal=(0.0, 0.0, 0.5))], [ft(303, 200, 3)]), E({0: 0}, [1]))
    c["viewcos_below"] = (build([pt(0.0, 0.0, 2.0, normal=(0.0, 0.0, down(0.5)))], [ft(303, 200, 3)]), E({}, [0]))
    # level clamps (MapPoint.cpp:384-398): ratio = 1 / 1.15 < 1 -> ceil of a negative quotient above -1 = 0;
    # the better descriptor sits on octave 1 = L + 1 and is not taken.  ratio = 1.2^9 -> 9 -> n_levels - 1 = 7:
    # radius 2.5 * 1.2^7 = 8.96, octaves 6 and 7 are searched, 5 is not
    c["level_low"] = (build([pt(0.0, 0.0, 1.0, dmax=f32(1.0 / 1.15))], [ft(301, 200, 1, octave=1), ft(302, 200, 20)]),
                      E({1: 0}, [1]))
    c["level_high"] = (build([pt(0.0, 0.0, 1.0, dmax=f32(1.2 ** 9))],
                             [ft(301, 200, 1, octave=5), ft(302, 200, 20, octave=6), ft(308, 200, 9, octave=7)]),
                       E({2: 0}, [1]))
    # Tracking.cpp:1006-1009: a point seen in this frame already and a bad point are skipped; the third matches
    c["skipped_points"] = (build([pt(0.0, 0.0, skip=1), pt(1.0, 0.0, state=2), pt(2.0, 0.0)],
                                 [ft(300, 200, 3), ft(400, 200, 3), ft(500, 200, 3)]), E({2: 2}, [0, 0, 1]))
    # ---- radius (:102-108) ----
    # viewCos == (float)0.998 = 0.99800003 > the double 0.998: radius 2.5, the feature 3 px away is outside and
    # the worse one 2 px away is taken; the next float below: radius 4.0, the feature 3 px away wins (3 vs 50
    # bits at one level: 3 <= 0.8 * 50, no veto)
    c["radius_double_compare"] = (build([pt(0.0, 0.0, 1.0, normal=(0.0, 0.0, f32(0.998)))],
                                        [ft(303, 200, 3), ft(302, 200, 50)]), E({1: 0}, [1]))
    c["radius_below"] = (build([pt(0.0, 0.0, 1.0, normal=(0.0, 0.0, down(f32(0.998))))],
                               [ft(303, 200, 3), ft(302, 200, 50)]), E({0: 0}, [1]))
    # ---- window and stereo gate ----
    # th = 1: radius 2.5, the feature 10 px away is outside; th = 5: 12.5, inside
    c["th_one"] = (build([pt(0.0, 0.0)], [ft(310, 200, 3)], th=1.0), E({}, [1]))
    c["th_five"] = (build([pt(0.0, 0.0)], [ft(310, 200, 3)], th=5.0), E({0: 0}, [1]))
    # |dx| == r is outside (strict <, Frame.cpp:440): 302.5 is excluded, 302.25 taken
    c["window_strict"] = (build([pt(0.0, 0.0)], [ft(302.5, 200, 3), ft(302.25, 200, 30)]), E({1: 0}, [1]))
    # levels [L-1, L]: L = 3 (radius 2.5 * 1.728 = 4.32) takes octaves 2 and 3; octave 4 is not searched.  Best
    # 9 bits at octave 3, runner-up 20 bits at octave 2: different levels, no ratio test
    c["levels"] = (build([pt(0.0, 0.0, level=3)],
                         [ft(301, 200, 1, octave=4), ft(302, 200, 9, octave=3), ft(303, 200, 20, octave=2)]),
                   E({1: 0}, [1]))
    # stereo gate (:62-67): xr = 300 - 40 = 260, radius 2.5.  u_right = 262.5: er = 2.5, not above, taken;
    # one float beyond: skipped, and the worse monocular feature (u_right < 0, ungated) is taken
    c["stereo_on"] = (build([pt(0.0, 0.0)], [ft(301, 200, 3, ur=262.5), ft(302, 200, 30)]), E({0: 0}, [1]))
    c["stereo_beyond"] = (build([pt(0.0, 0.0)], [ft(301, 200, 3, ur=up(262.5)), ft(302, 200, 30)]), E({1: 0}, [1]))
    # ---- cutoff and veto ----
    # bestDist <= TH_HIGH: 100 bits kept, 101 dropped; each is a single candidate (bestLevel2 = -1: no veto)
    c["cutoff"] = (build([pt(0.0, 0.0), pt(2.0, 0.0)], [ft(300, 200, 100), ft(500, 200, 101)]), E({0: 0}, [1, 1]))
    # veto at one level: 10 > 0.8f * 12 = 9.6; none across levels (point level 1, radius 3)
    c["veto_same_level"] = (build([pt(0.0, 0.0)], [ft(301, 200, 10), ft(302, 200, 12)]), E({}, [1]))
    c["no_veto_levels"] = (build([pt(0.0, 0.0, level=1)], [ft(301, 200, 10, octave=1), ft(302, 200, 12, octave=0)]),
                           E({0: 0}, [1]))
    # equal distances at two levels: the visiting order 298, 299, 301 decides which of the equals is the
    # runner-up.  Octaves (1, 1, 0): best = 298, runner-up = 299 at the same level, 10 > 8: vetoed.  Octaves
    # (1, 0, 1): runner-up = 299 at level 0: accepted on 298
    c["tie_levels_veto"] = (build([pt(0.0, 0.0, level=1)], [ft(298, 200, 10, octave=1), ft(299, 200, 10, octave=1),
                                                           ft(301, 200, 10, octave=0)]), E({}, [1]))
    c["tie_levels_pass"] = (build([pt(0.0, 0.0, level=1)], [ft(298, 200, 10, octave=1), ft(299, 200, 10, octave=0),
                                                           ft(301, 200, 10, octave=1)]), E({0: 0}, [1]))
    # visiting order is cell order, not index order: feature 0 at 301 is visited last, so best = feature 1 and
    # runner-up = feature 2, both at level 1: vetoed (in index order the runner-up would be at another level)
    c["tie_levels_order"] = (build([pt(0.0, 0.0, level=1)], [ft(301, 200, 10, octave=0), ft(299, 200, 10, octave=1),
                                                            ft(298, 200, 10, octave=1)]), E({}, [1]))
    # ---- occupancy (:58-60) ----
    # an entry occupant with observations blocks: the runner-up is taken alone
    c["entry_blocks"] = (build([pt(0.0, 0.0)], [ft(301, 200, 2, occ=2), ft(302, 200, 30)]), E({1: 0}, [1]))
    # an entry occupant without observations is overwritten
    c["entry_overwritten"] = (build([pt(0.0, 0.0)], [ft(301, 200, 2, occ=1), ft(302, 200, 30)]), E({0: 0}, [1]))
    # an earlier point with observations blocks: point 0 takes the 2-bit feature, point 1 the other
    c["earlier_blocks"] = (build([pt(0.0, 0.0), pt(0.0, 0.0)], [ft(301, 200, 2), ft(302, 200, 30)]),
                           E({0: 0, 1: 1}, [1, 1]))
    # an earlier point without observations is overwritten: both take feature 0, both count, the last stays
    c["earlier_overwritten"] = (build([pt(0.0, 0.0, has_obs=0), pt(0.0, 0.0)], [ft(301, 200, 2), ft(302, 200, 30)]),
                                E({0: 1}, [1, 1], nmatches=2))
    # the earlier point takes the best: the runner-up is promoted and its own runner-up (40 bits: 20 <= 32)
    # does not veto it
    c["promoted"] = (build([pt(0.0, 0.0), pt(0.0, 0.0)], [ft(301, 200, 2), ft(302, 200, 20), ft(301.5, 200, 40)]),
                     E({0: 0, 1: 1}, [1, 1]))
    # the earlier point takes the RUNNER-UP: point 1 alone is vetoed (10 > 0.8f * 11 = 8.8); point 0 at u = 304
    # sees only the feature at 302 (|301 - 304| = 3 > 2.5) and takes it, so point 1 has a single candidate
    c["veto_lifted"] = (build([pt(0.04, 0.0), pt(0.0, 0.0)], [ft(301, 200, 10), ft(302, 200, 11)]),
                        E({1: 0, 0: 1}, [1, 1]))
    c["veto_not_lifted"] = (build([pt(0.04, 0.0, state=2), pt(0.0, 0.0)], [ft(301, 200, 10), ft(302, 200, 11)]),
                            E({}, [0, 1]))
    return c


def domino(k: int = 40):
    """k points in a row 9 px apart with feature j 3 px right of point j's projection, th = 4 (radius 10): point
    i sees features i - 1 (6 px left) and i (3 px right) and no other.  Feature j has bits [0, 3 j) set and point
    i bits [0, 3 i - 2), so point i is at distance 1 from feature i - 1 (its best, which point i - 1 owns) and 2
    from feature i (1 <= 0.8 * 2: no veto).  Sequentially point i ends on feature i; in round 1 every point
    i >= 1 chooses feature i - 1, and the correction moves one point per round: k + 1 rounds."""
    pts = [pt((20 + 9 * i - 300) / 100.0, 0.0, desc=desc_bits(max(3 * i - 2, 0))) for i in range(k)]
    fts = [ft(23 + 9 * j, 200, 0, desc=desc_bits(3 * j)) for j in range(k)]
    return build(pts, fts, th=4.0), E({j: j for j in range(k)}, [1] * k)


def expected_out(problem, exp) -> np.ndarray:
    out = np.full(problem.frame.n, -1, np.int32)
    for f, s in exp["out"].items():
        out[f] = s
    return out


def random_problem(seed: int, th: float, n_frame: int = 600, n_points: int = 1500, n_pairs: int = 30, **kw):
    """A random crowded problem: rsc.synth.make_loop_projection_problem's KeyFrame as the Frame (clusters of
    features with near-identical descriptors that more points than features project onto), with about 30 % of
    the points without observations, about 30 % monocular features, the others with a u_right a few pixels
    around its true value, entry occupants of both kinds, and n_pairs planted lifted vetoes."""
    par = dict(n_clusters=24, cluster_kps=8, cluster_pts=14, occupied_frac=0.0, already_frac=0.05)
    par.update(kw)
    rng = np.random.default_rng(seed)
    p = synth.make_loop_projection_problem(rng, n_frame, n_points, **par)
    kf = p.kf
    T = p.Scw.astype(np.float64)
    # the depth behind each feature: that of the nearest projected point, else 5 m
    Pc = p.pts.pos.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    z = np.where(Pc[:, 2] > 0.1, Pc[:, 2], 5.0)
    uv = np.stack([kf.fx * Pc[:, 0] / z + kf.cx, kf.fy * Pc[:, 1] / z + kf.cy], 1)
    depth = np.full(kf.n, 5.0)
    for f in range(kf.n):
        d2 = ((uv - kf.kp[f]) ** 2).sum(1)
        j = int(np.argmin(d2))
        if d2[j] < 100.0:
            depth[f] = z[j]
    mbf = float(synth.EUROC_BF)
    u_right = kf.kp[:, 0] - mbf / depth + rng.normal(0, 6.0, kf.n)
    u_right = np.where(rng.random(kf.n) < 0.3, -1.0, np.maximum(u_right, 0.5)).astype(f32)
    occ = np.where(rng.random(kf.n) < 0.1, rng.integers(1, 3, kf.n), 0).astype(np.uint8)
    has_obs = (rng.random(p.pts.n) >= 0.3).astype(np.uint8)
    skip = p.already.copy()
    kp, octave, desc = kf.kp.copy(), kf.octave.copy(), kf.desc.copy()
    pts = types.SimpleNamespace(n=p.pts.n, **{k: np.array(getattr(p.pts, k)) for k in _PT})
    # lifted vetoes are rare by chance, so n_pairs of them are planted over features and points drawn at
    # random: features A, B 3 px apart at one octave whose descriptors differ in 21 bits; the earlier point
    # carries B's descriptor and takes B; the later one is at 10 bits from A and 11 from B, vetoed on entry
    # (10 > 0.8f * 11) and accepted on A once B is held by a point with observations
    sf = synth.scale_factors()
    fs = rng.choice(kf.n, 2 * n_pairs, replace=False).reshape(n_pairs, 2)
    ps = np.sort(rng.choice(p.pts.n, 2 * n_pairs, replace=False).reshape(n_pairs, 2), axis=1)
    Ow = -T[:3, :3].T @ T[:3, 3]
    for (fa, fb), (q0, q1) in zip(fs, ps):
        c = np.array([rng.uniform(40, synth.WIDTH - 40), rng.uniform(40, synth.HEIGHT - 40)])
        o = int(rng.integers(1, synth.N_LEVELS - 1))
        bits = rng.choice(256, 21, replace=False)
        dA = rng.integers(0, 256, 32, dtype=np.uint8)
        dB, dQ = dA.copy(), dA.copy()
        for b in bits:
            dB[b // 8] ^= 1 << (b % 8)
        for b in bits[:10]:
            dQ[b // 8] ^= 1 << (b % 8)
        kp[fa], kp[fb] = c + [-1.5, 0.0], c + [1.5, 0.0]
        octave[[fa, fb]] = o
        desc[fa], desc[fb] = dA, dB
        u_right[[fa, fb]] = -1.0
        occ[[fa, fb]] = 0
        zc = rng.uniform(3, 9)
        Xw = T[:3, :3].T @ (np.array([(c[0] - kf.cx) / kf.fx * zc, (c[1] - kf.cy) / kf.fy * zc, zc]) - T[:3, 3])
        d = np.linalg.norm(Xw - Ow)
        for q, dq in ((q0, dB), (q1, dQ)):
            pts.pos[q], pts.normal[q], pts.desc[q] = Xw, (Xw - Ow) / d, dq
            pts.dmax[q] = d * 1.2 ** (o - 0.5)
            pts.dmin[q] = pts.dmax[q] / sf[-1]
            pts.state[q], skip[q], has_obs[q] = 1, 0, 1
    fr = make_frame(kp, octave, desc, u_right, mbf=mbf)
    return types.SimpleNamespace(frame=fr, pts=pts, Tcw=p.Scw, skip=skip, has_obs=has_obs, frame_occ=occ,
                                 cos_limit=COS_LIMIT, th=float(th), nn_ratio=NN_RATIO)


# name -> (seed, th): chosen so that make_localproj_golden.py's conditions hold
RANDOM = {"random_a": (21, 5.0), "random_b": (22, 1.0)}


def reference(p, trace=None):
    """The restatement's answer for a problem: dict(out, track, nmatches, n_to_match, rounds, round1)."""
    r = lr.search_local_points(p.frame, p.pts, p.Tcw, p.skip, p.has_obs, p.frame_occ, p.cos_limit, p.th, p.nn_ratio,
                               trace)
    claim, rounds, first = lr.fixed_point_rounds(p.frame, p.pts, r["track"], p.skip, p.has_obs, p.frame_occ, p.th,
                                                 p.nn_ratio)
    assert np.array_equal(lr.out_of_claims(p.frame.n, claim), r["out"]), "the rounds' fixed point is not sequential"
    r["rounds"] = rounds
    r["round1"] = lr.out_of_claims(p.frame.n, first)
    return r


# ---- fixture packing (tests/golden/localproj_traces.npz) -----------------------------------------------
_PT = ("state", "pos", "normal", "dmax", "dmin", "desc")
_FR = ("kp", "octave", "desc", "u_right")


def to_arrays(p, prefix: str) -> dict:
    d = {f"{prefix}/pt_{k}": np.asarray(getattr(p.pts, k)) for k in _PT}
    d.update({f"{prefix}/fr_{k}": np.asarray(getattr(p.frame, k)) for k in _FR})
    d[f"{prefix}/K"] = np.array([p.frame.fx, p.frame.fy, p.frame.cx, p.frame.cy, p.frame.max_x, p.frame.mbf],
                                np.float64)
    d[f"{prefix}/Tcw"] = np.asarray(p.Tcw, f32)
    d[f"{prefix}/skip"] = np.asarray(p.skip, np.uint8)
    d[f"{prefix}/has_obs"] = np.asarray(p.has_obs, np.uint8)
    d[f"{prefix}/frame_occ"] = np.asarray(p.frame_occ, np.uint8)
    d[f"{prefix}/par"] = np.array([p.cos_limit, p.th, p.nn_ratio], f32)
    return d


def from_arrays(z, prefix: str):
    g = lambda k: z[f"{prefix}/{k}"]
    fx, fy, cx, cy, max_x, mbf = (float(v) for v in g("K"))
    fr = make_frame(g("fr_kp"), g("fr_octave"), g("fr_desc"), g("fr_u_right"), mbf=mbf, fx=fx, fy=fy, cx=cx, cy=cy,
                    max_x=max_x)
    pts = kr.points_of(**{k: g(f"pt_{k}") for k in _PT})
    cos_limit, th, nn = (float(v) for v in g("par"))
    return types.SimpleNamespace(frame=fr, pts=pts, Tcw=g("Tcw"), skip=g("skip"), has_obs=g("has_obs"),
                                 frame_occ=g("frame_occ"), cos_limit=cos_limit, th=th, nn_ratio=float(f32(nn)))
