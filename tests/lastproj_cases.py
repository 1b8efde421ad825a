"""Hand-built problems with known answers for ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th)
(src/ORBmatcher.cpp:1173-1315), one per rule (TEST-ONLY), shared by the CPU tests, the GPU tests, the facade
test and the golden fixture.

Geometry that can be checked by hand: identity current pose, fx = fy = 100, cx = 300, cy = 200, mbf = 40, so a
point (x, y, z) projects to u = 100 x / z + 300, v = 100 y / z + 200, ur = u - 40 / z; image [0, 700] x [0, 480],
both ends inside.  The radius is th * 1.2^o for a LastFrame keypoint at octave o (default th = 2.5, o = 0).
With the identity current pose twc = 0 and tlc.z is the last pose's z translation: 0 by default, so with mb = 0.4
the mode is "window" (octaves [o-1, o+1]); tz = 1 is forward, tz = -1 backward.  Descriptors: a slot's MapPoint
has all zeros, a feature has its first `bits` bits set, so the descriptor distance is `bits`.  Features are
monocular (u_right = -1) and all angles 0 (rotation bin 0) unless stated.  The grid cells are 11.75 px wide and
10 px high and PosInGrid rounds, so x = 298 and 299 are in column 25 and x = 301 in column 26: the visiting
order is 298, 299 (cell order = index order), then 301.
"""
from __future__ import annotations

import types

import numpy as np

import lastproj_ref as ref
from localproj_cases import desc_bits, down, make_frame, up
from rsc import synth

f32 = np.float32
FX = FY = 100.0
CX, CY = 300.0, 200.0
MAX_X = 700.0
MBF = 40.0
MB = 0.4
TH = 2.5


def sl(x, y, z=1.0, octave=0, state=1, has_obs=1, angle=0.0, desc=None):
    """A LastFrame slot: its MapPoint's position, mvKeys octave, mvKeysUn angle."""
    return dict(pos=(x, y, z), octave=octave, state=state, has_obs=has_obs, angle=angle, desc=desc)


def ft(u, v, bits, octave=0, occ=0, ur=-1.0, angle=0.0, desc=None):
    return dict(pt=(u, v), bits=bits, octave=octave, occ=occ, ur=ur, angle=angle, desc=desc)


def last_of(octave, angle, mp_state, mp_pos, mp_desc, mp_has_obs):
    n = len(octave)
    return types.SimpleNamespace(n=n, octave=np.ascontiguousarray(octave, np.int32),
                                 angle=np.ascontiguousarray(angle, f32),
                                 mp_state=np.ascontiguousarray(mp_state, np.uint8),
                                 mp_pos=np.ascontiguousarray(mp_pos, f32).reshape(n, 3),
                                 mp_desc=np.ascontiguousarray(mp_desc, np.uint8).reshape(n, 32),
                                 mp_has_obs=np.ascontiguousarray(mp_has_obs, np.uint8))


def pose(tz=0.0):
    T = np.eye(4, dtype=f32)
    T[2, 3] = tz
    return T


def build(slots, fts, th=TH, tz_last=0.0, mb=MB, check_ori=1, swap_cell=None):
    """A problem namespace: frame, last, Tcw_cur, Tcw_last, mb, frame_occ, th, check_ori.  swap_cell = (f, g):
    the two features, which share a cell, change places in mGrid's list of that cell."""
    fr = make_frame([k["pt"] for k in fts], [k["octave"] for k in fts],
                    [desc_bits(k["bits"]) if k["desc"] is None else k["desc"] for k in fts],
                    [k["ur"] for k in fts], fx=FX, fy=FY, cx=CX, cy=CY, max_x=MAX_X)
    fr.angle = np.array([k["angle"] for k in fts], f32)
    if swap_cell is not None:
        a, b = (int(np.nonzero(fr.cell_feat == f)[0][0]) for f in swap_cell)
        fr.cell_feat[a], fr.cell_feat[b] = fr.cell_feat[b], fr.cell_feat[a]
    last = last_of([s["octave"] for s in slots], [s["angle"] for s in slots], [s["state"] for s in slots],
                   [s["pos"] for s in slots],
                   [np.zeros(32, np.uint8) if s["desc"] is None else s["desc"] for s in slots],
                   [s["has_obs"] for s in slots])
    return types.SimpleNamespace(frame=fr, last=last, Tcw_cur=pose(), Tcw_last=pose(tz_last), mb=float(mb),
                                 frame_occ=np.array([k["occ"] for k in fts], np.uint8), th=float(th),
                                 check_ori=int(check_ori))


def E(out, nmatches=None, mode=0):
    """expected: out {feature: slot, or -2 for nullptr}, nmatches (default: the slots left set), mode."""
    return dict(out=out, nmatches=sum(1 for s in out.values() if s >= 0) if nmatches is None else nmatches,
                mode=mode)


def _levels(o, octs, tz, n_slots):
    """n_slots identical slots with observations at the image centre, LastFrame octave o, and one feature per
    octave of `octs` at 298 + k with k + 1 bits: the slots take the allowed features in order of distance, so the
    features matched are the set GetFeaturesInArea returns."""
    return build([sl(0.0, 0.0, octave=o) for _ in range(n_slots)],
                 [ft(298.0 + k, 200, k + 1, octave=oc) for k, oc in enumerate(octs)], tz_last=tz)


def _pairs(bins, extra_slots=(), extra_fts=(), **kw):
    """Independent (slot, feature) pairs 20 px apart along v = 100: pair k at u = 50 + 20 k, the slot's angle 30 *
    bins[k] (rotation bin bins[k] against the feature's angle 0).  extra_*: appended after the pairs."""
    slots = [sl((50 + 20 * k - 300) / 100.0, -1.0, angle=30.0 * b) for k, b in enumerate(bins)]
    fts = [ft(50 + 20 * k, 100, 3) for k in range(len(bins))]
    return build(slots + list(extra_slots), fts + list(extra_fts), **kw)


def cases():
    """name -> (problem, expected).  Expected values are worked out in the comments, not computed."""
    c = {}
    # ---- projection ----
    # inclusive bounds (:1218-1221), th = 8: x = -3 -> u = 0 = mnMinX, x = 4 -> u = 700 = mnMaxX, y = -2 -> v = 0,
    # y = 2.8f -> 100 y = 279.999995 which rounds to 280.0 in float -> v = 480 = mnMaxY: all four inside
    b_fts = [ft(1, 200, 3), ft(699, 200, 3), ft(300, 1, 3), ft(300, 474, 3)]
    c["bound_on"] = (build([sl(-3.0, 0.0), sl(4.0, 0.0), sl(0.0, -2.0), sl(0.0, 2.8)], b_fts, th=8.0),
                     E({0: 0, 1: 1, 2: 2, 3: 3}))
    # one float outside each: u = -0.00003, u = 700.00006, v = -0.00002, v = 480.00003
    c["bound_outside"] = (build([sl(down(-3.0), 0.0), sl(up(4.0), 0.0), sl(0.0, down(-2.0)), sl(0.0, up(2.8))],
                                b_fts, th=8.0), E({}))
    # invzc < 0 (:1212): (0, 0, -1) would project to u = 300 where feature 0 waits; (1, 0, 1) -> u = 400
    c["depth_negative"] = (build([sl(0.0, 0.0, -1.0), sl(1.0, 0.0)], [ft(300, 200, 3), ft(400, 200, 3)]), E({1: 1}))
    # z == +0 with x != 0: invzc = +inf passes :1212, u = +inf > mnMaxX, rejected by the bounds; a -0 coordinate
    # becomes +0 in the row sum and goes the same way.  (0, 0, 0) gives u = v = NaN, which passes both tests and
    # would reach floor: outside the reference's defined behaviour, skipped
    c["depth_zero"] = (build([sl(1.0, 0.0, 0.0), sl(1.0, 0.0, -0.0), sl(0.0, 0.0, 0.0), sl(1.0, 0.0)],
                             [ft(300, 200, 3), ft(400, 200, 3)]), E({1: 3}))
    # bestDist <= TH_HIGH (:1271): 100 bits kept, 101 dropped
    c["cutoff"] = (build([sl(0.0, 0.0), sl(2.0, 0.0)], [ft(300, 200, 100), ft(500, 200, 101)]), E({0: 0}))
    # an outlier slot and an empty slot are skipped (:1200-1202); the third matches
    c["skipped_slots"] = (build([sl(0.0, 0.0, state=2), sl(1.0, 0.0, state=0), sl(2.0, 0.0)],
                                [ft(300, 200, 3), ft(400, 200, 3), ft(500, 200, 3)]), E({2: 2}))
    # ---- window and stereo gate ----
    # |dx| == r is outside (strict <, Frame.cpp:440): 302.5 is excluded, 302.25 taken
    c["window_strict"] = (build([sl(0.0, 0.0)], [ft(302.5, 200, 3), ft(302.25, 200, 30)]), E({1: 0}))
    # (300 + 2.5) / 11.75 = 25.74: floor 25, ceil 26.  x = 301 is in column 26 (25.62 rounds up), which only
    # nMaxCellX = ceil(...) reaches (Frame.cpp:403)
    c["ceil_cell"] = (build([sl(0.0, 0.0)], [ft(301, 200, 3)]), E({0: 0}))
    # the radius grows with the LastFrame octave (:1226): o = 2 gives 2.5 * 1.44 = 3.6, so 303 is inside
    c["radius_octave"] = (build([sl(0.0, 0.0, octave=2), sl(1.0, 0.0, octave=0)],
                                [ft(303, 200, 3, octave=2), ft(403, 200, 3)]), E({0: 0}))
    # stereo gate (:1252-1258): ur = 300 - 40 = 260, radius 2.5.  mvuRight = 262.5: er = 2.5, not above, taken;
    # one float beyond: skipped, and the worse monocular feature is taken; mvuRight == 0 is not gated (> 0)
    c["stereo_on"] = (build([sl(0.0, 0.0)], [ft(301, 200, 3, ur=262.5), ft(302, 200, 30)]), E({0: 0}))
    c["stereo_beyond"] = (build([sl(0.0, 0.0)], [ft(301, 200, 3, ur=up(262.5)), ft(302, 200, 30)]), E({1: 0}))
    c["stereo_zero_ungated"] = (build([sl(0.0, 0.0)], [ft(301, 200, 3, ur=0.0), ft(302, 200, 30)]), E({0: 0}))
    # ---- level modes (:1230-1235) ----
    # o = 3 (radius 4.32), features at octaves 1..5 = indices 0..4, five slots
    c["levels_window"] = (_levels(3, [1, 2, 3, 4, 5], 0.0, 5), E({1: 0, 2: 1, 3: 2}, mode=0))      # [2, 4]
    c["levels_forward"] = (_levels(3, [1, 2, 3, 4, 5], 1.0, 5), E({2: 0, 3: 1, 4: 2}, mode=1))     # >= 3
    c["levels_backward"] = (_levels(3, [1, 2, 3, 4, 5], -1.0, 5), E({0: 0, 1: 1, 2: 2}, mode=2))   # [0, 3]
    # o = 0 (radius 2.5), features at octaves 0, 1, 2: window [-1, 1]; forward switches the check off (all);
    # backward [0, 0]
    c["levels_window_o0"] = (_levels(0, [0, 1, 2], 0.0, 3), E({0: 0, 1: 1}, mode=0))
    c["levels_forward_o0"] = (_levels(0, [0, 1, 2], 1.0, 3), E({0: 0, 1: 1, 2: 2}, mode=1))
    c["levels_backward_o0"] = (_levels(0, [0, 1, 2], -1.0, 3), E({0: 0}, mode=2))
    # o = n_levels - 1 = 7 (radius 8.96), features at octaves 5, 6, 7: window [6, 8]; forward >= 7; backward all
    c["levels_window_top"] = (_levels(7, [5, 6, 7], 0.0, 3), E({1: 0, 2: 1}, mode=0))
    c["levels_forward_top"] = (_levels(7, [5, 6, 7], 1.0, 3), E({2: 0}, mode=1))
    c["levels_backward_top"] = (_levels(7, [5, 6, 7], -1.0, 3), E({0: 0, 1: 1, 2: 2}, mode=2))
    # tlc.z == mb is neither forward nor backward (strict >, :1193-1194); the next float is
    lv = lambda tz: build([sl(0.0, 0.0, octave=3) for _ in range(5)],
                          [ft(298.0 + k, 200, k + 1, octave=1 + k) for k in range(5)], tz_last=tz, mb=0.5)
    c["mode_at_mb"] = (lv(0.5), E({1: 0, 2: 1, 3: 2}, mode=0))
    c["mode_above_mb"] = (lv(up(0.5)), E({2: 0, 3: 1, 4: 2}, mode=1))
    c["mode_below_mb"] = (lv(down(0.5)), E({1: 0, 2: 1, 3: 2}, mode=0))
    c["mode_at_minus_mb"] = (lv(-0.5), E({1: 0, 2: 1, 3: 2}, mode=0))
    c["mode_beyond_minus_mb"] = (lv(down(-0.5)), E({0: 0, 1: 1, 2: 2}, mode=2))
    # ---- order and ties (:1264, strict <: the first minimum in visiting order wins) ----
    # across columns: 299 (column 25) is visited before 301 (column 26), whatever the indices
    c["tie_columns"] = (build([sl(0.0, 0.0)], [ft(301, 200, 10), ft(299, 200, 10)]), E({1: 0}))
    # across rows of one column, th = 8: v = 199 is in row 20, v = 206 in row 21 (20.6 rounds up)
    c["tie_rows"] = (build([sl(0.0, 0.0)], [ft(300, 206, 10), ft(300, 199, 10)], th=8.0), E({1: 0}))
    # inside one cell the list order decides, not the index: feature 1 stands first in the permuted list
    c["tie_cell"] = (build([sl(0.0, 0.0)], [ft(300, 200, 10), ft(300.5, 200, 10)], swap_cell=(0, 1)), E({1: 0}))
    c["tie_cell_index_order"] = (build([sl(0.0, 0.0)], [ft(300, 200, 10), ft(300.5, 200, 10)]), E({0: 0}))
    # greedy order: slot 0 (with observations) takes the 2-bit feature, slot 1's runner-up is promoted
    c["greedy_promoted"] = (build([sl(0.0, 0.0), sl(0.0, 0.0)], [ft(301, 200, 2), ft(302, 200, 20)]),
                            E({0: 0, 1: 1}))
    # ---- occupancy depends on the occupant (:1248-1250) ----
    # a slot without observations is overwritten: both take feature 0, both count, the last stays
    c["nonblocking_overwritten"] = (build([sl(0.0, 0.0, has_obs=0), sl(0.0, 0.0)],
                                          [ft(301, 200, 2), ft(302, 200, 20)]), E({0: 1}, nmatches=2))
    # an entry occupant with observations blocks; one without is overwritten
    c["entry_with_obs"] = (build([sl(0.0, 0.0)], [ft(301, 200, 2, occ=2), ft(302, 200, 30)]), E({1: 0}))
    c["entry_without_obs"] = (build([sl(0.0, 0.0)], [ft(301, 200, 2, occ=1), ft(302, 200, 30)]), E({0: 0}))
    # ---- rotation check (:1292-1312) ----
    # bins 0: 10, 1: 5, 2: 1, 3: 1.  max3 = 1 against 0.1f * 10 = 1.0 in float: 1 < 1.0 is false, bin 2 stays
    # the third maximum (the smallest the 10 % rule keeps); bin 3 (not above max3) is removed: pair 16 nulled
    c["third_max_kept"] = (_pairs([0] * 10 + [1] * 5 + [2, 3]), E({**{k: k for k in range(16)}, 16: -2}))
    # bins 0: 11, 1: 5, 2: 1.  1 < 0.1f * 11 = 1.1: ind3 = -1 (the largest third maximum dropped), pair 16 nulled
    c["third_max_dropped"] = (_pairs([0] * 11 + [1] * 5 + [2]), E({**{k: k for k in range(16)}, 16: -2}))
    # 12 pairs in bin 0, then feature 12 at (100, 300) with two claimers: slot 12 without observations, slot 13
    # with.  The histogram has 14 entries; a bin with one entry (1 < 1.2) is removed.
    two = lambda a12, a13, **kw: _pairs([0] * 12, [sl(-2.0, 1.0, has_obs=0, angle=a12), sl(-2.0, 1.0, angle=a13)],
                                        [ft(100, 300, 3)], **kw)
    kept12 = {k: k for k in range(12)}
    # the FIRST claimer's bin (3) is removed: the entry nulls feature 12 although slot 13's bin is kept; nmatches
    # = 14 - 1, while 12 slots are left set
    c["first_claimer_removed"] = (two(90.0, 0.0), E({**kept12, 12: -2}, nmatches=13))
    # the LAST claimer's bin is removed: the same state
    c["last_claimer_removed"] = (two(0.0, 90.0), E({**kept12, 12: -2}, nmatches=13))
    # both kept: the last claimer stays and both count
    c["two_claimers_kept"] = (two(0.0, 0.0), E({**kept12, 12: 13}, nmatches=14))
    # mbCheckOrientation false: no removal
    c["no_orientation"] = (two(90.0, 0.0, check_ori=0), E({**kept12, 12: 13}, nmatches=14))
    # an entry occupant without observations, overwritten by a claim that is then removed: nullptr, not restored
    c["entry_without_obs_nulled"] = (_pairs([0] * 12, [sl(-2.0, 1.0, angle=90.0)], [ft(100, 300, 3, occ=1)]),
                                     E({**kept12, 12: -2}, nmatches=12))
    # rot < 0 wraps (:1279) and the order of the difference matters through ComputeThreeMaxima's strict > in bin
    # order: bins 0: 12, 1: 2, 5: 2 and two pairs with last 10, current 40 -> rot = -30 + 360 = 330 -> bin 11.
    # max2 = bin 1, max3 = bin 5 (2 > 0), bin 11 (2 is not above max3) is removed.  With the difference the other
    # way round the groups would sit in bins 11, 7 and 1 and the pairs 12, 13 would be the ones removed
    c["rot_wrap"] = (_pairs([0] * 12 + [1, 1, 5, 5], [sl(-2.0, 1.0, angle=10.0), sl(-1.0, 1.0, angle=10.0)],
                            [ft(100, 300, 3, angle=40.0), ft(200, 300, 3, angle=40.0)]),
                     E({**{k: k for k in range(16)}, 16: -2, 17: -2}, nmatches=16))
    return c


def domino(k: int = 40):
    """k slots in a row 9 px apart with feature j 3 px right of slot j's projection, th = 10 (radius 10): slot i
    sees features i - 1 (6 px left) and i (3 px right) and no other.  Feature j has bits [0, 3 j) set and slot i
    bits [0, 3 i - 2), so slot i is at distance 1 from feature i - 1 (its best, which slot i - 1 owns) and 2 from
    feature i.  Sequentially slot i ends on feature i; in round 1 every slot i >= 1 chooses feature i - 1, and the
    correction moves one slot per round: k + 1 rounds."""
    slots = [sl((20 + 9 * i - 300) / 100.0, 0.0, desc=desc_bits(max(3 * i - 2, 0))) for i in range(k)]
    fts = [ft(23 + 9 * j, 200, 0, desc=desc_bits(3 * j)) for j in range(k)]
    return build(slots, fts, th=10.0), E({j: j for j in range(k)})


def expected_out(problem, exp) -> np.ndarray:
    out = np.full(problem.frame.n, -1, np.int32)
    for f, s in exp["out"].items():
        out[f] = s
    return out


def _flip(rng, d, k):
    d = d.copy()
    for b in rng.choice(256, k, replace=False):
        d[b // 8] ^= 1 << (b % 8)
    return d


def random_problem(seed: int, th: float, mode: int = 0, n_frame: int = 600, n_last: int = 1500, n_clusters: int = 40,
                   cluster_kps: int = 8, cluster_slots: int = 20):
    """A crowded problem: clusters of current features a few pixels apart with near-identical descriptors onto
    which more LastFrame slots project than there are features, the rest scattered; about 30 % of the slots
    without observations, about 10 % outliers or empty, about 30 % monocular features, the others with a u_right
    a few pixels around its true value, entry occupants of both kinds; most slots agree with their cluster's
    angle, a sixth carry a random one.  A general current pose; the last pose is the current one moved along the
    optical axis so that the call's level mode is `mode`."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = (float(v) for v in (synth.FX, synth.FY, synth.CX, synth.CY))
    W, H, mbf = float(synth.WIDTH), float(synth.HEIGHT), float(synth.EUROC_BF)
    kp = np.zeros((n_frame, 2)); octave = np.zeros(n_frame, np.int32); angle = np.zeros(n_frame)
    desc = np.zeros((n_frame, 32), np.uint8)
    suv = np.zeros((n_last, 2)); soct = np.zeros(n_last, np.int32); sang = np.zeros(n_last)
    sdesc = np.zeros((n_last, 32), np.uint8)
    k = i = 0
    for _ in range(n_clusters):
        c = np.array([rng.uniform(40, W - 40), rng.uniform(40, H - 40)])
        o, a = int(rng.integers(1, 7)), rng.uniform(0, 360)
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        for _ in range(cluster_kps):
            kp[k], octave[k], angle[k] = c + rng.uniform(-4, 4, 2), o - 1 + int(rng.integers(0, 3)), \
                (a + rng.uniform(-10, 10)) % 360.0
            desc[k] = _flip(rng, base, 5)
            k += 1
        for _ in range(cluster_slots):
            suv[i], soct[i] = c + rng.uniform(-2, 2, 2), o
            sang[i] = rng.uniform(0, 360) if rng.random() < 1 / 6 else a
            sdesc[i] = _flip(rng, base, 3)
            i += 1
    while k < n_frame:
        kp[k], octave[k], angle[k] = (rng.uniform(2, W - 8), rng.uniform(2, H - 8)), int(rng.integers(0, 8)), \
            rng.uniform(0, 360)
        desc[k] = rng.integers(0, 256, 32, dtype=np.uint8)
        k += 1
    while i < n_last:
        src = int(rng.integers(0, n_frame))
        suv[i], soct[i], sang[i] = kp[src] + rng.uniform(-1, 1, 2), octave[src], angle[src]
        sdesc[i] = _flip(rng, desc[src], 8)
        i += 1
    z = rng.uniform(3, 9, n_last)
    z = np.where(rng.random(n_last) < 0.03, -z, z)           # behind the camera
    Pc = np.stack([(suv[:, 0] - cx) / fx * z, (suv[:, 1] - cy) / fy * z, z], 1)
    R = synth.random_rotation(rng, 0.2)
    t = rng.uniform(-0.5, 0.5, 3)
    Tc = np.eye(4); Tc[:3, :3], Tc[:3, 3] = R, t
    pos = (Pc - t) @ R                                        # Rcw^T (Pc - tcw)
    Tl = Tc.copy()
    Tl[2, 3] += {0: 0.0, 1: 0.5, 2: -0.5}[mode]               # tlc.z = the shift (Rlw = Rcw)
    state = np.where(rng.random(n_last) < 0.1, rng.integers(0, 2, n_last) * 2, 1).astype(np.uint8)
    has_obs = (rng.random(n_last) >= 0.3).astype(np.uint8)
    u_right = kp[:, 0] - mbf / 6.0 + rng.normal(0, 6.0, n_frame)
    u_right = np.where(rng.random(n_frame) < 0.3, -1.0, np.maximum(u_right, 0.5)).astype(f32)
    occ = np.where(rng.random(n_frame) < 0.1, rng.integers(1, 3, n_frame), 0).astype(np.uint8)
    fr = make_frame(kp, octave, desc, u_right, mbf=mbf)
    fr.angle = angle.astype(f32)
    last = last_of(soct, sang, state, pos, sdesc, has_obs)
    return types.SimpleNamespace(frame=fr, last=last, Tcw_cur=Tc.astype(f32), Tcw_last=Tl.astype(f32), mb=0.11,
                                 frame_occ=occ, th=float(th), check_ori=1)


def from_arrays_like(p, frame, last):
    """The call of `p` (poses, mb, th, check_ori) on another Frame pair, from an empty mvpMapPoints."""
    return types.SimpleNamespace(frame=frame, last=last, Tcw_cur=p.Tcw_cur, Tcw_last=p.Tcw_last, mb=p.mb,
                                 frame_occ=np.zeros(frame.n, np.uint8), th=p.th, check_ori=p.check_ori)


# name -> (seed, th, mode): chosen so that the census of tests/test_cpu_lastproj.py holds
RANDOM = {"random_a": (31, 7.0, 0), "random_b": (32, 15.0, 0), "random_forward": (33, 7.0, 1),
          "random_backward": (34, 7.0, 2)}


def reference(p, trace=None):
    """The restatement's answer for a problem: dict(out, nmatches, mode, rounds, round1)."""
    nmatches, out, mode = ref.search_by_projection_last(p, trace)
    claim, rounds, first = ref.fixed_point_rounds(p)
    n2, out2, _ = ref.finish(p, claim)
    assert n2 == nmatches and np.array_equal(out2, out), "the rounds' fixed point is not sequential"
    return dict(out=out, nmatches=nmatches, mode=mode, rounds=rounds, round1=ref.finish(p, first)[1])


# ---- fixture packing (tests/golden/lastproj_traces.npz) ------------------------------------------------
_LAST = ("octave", "angle", "mp_state", "mp_pos", "mp_desc", "mp_has_obs")
_FR = ("kp", "octave", "angle", "desc", "u_right", "cell_feat")


def to_arrays(p, prefix: str) -> dict:
    d = {f"{prefix}/last_{k}": np.asarray(getattr(p.last, k)) for k in _LAST}
    d.update({f"{prefix}/fr_{k}": np.asarray(getattr(p.frame, k)) for k in _FR})
    d[f"{prefix}/K"] = np.array([p.frame.fx, p.frame.fy, p.frame.cx, p.frame.cy, p.frame.max_x, p.frame.mbf],
                                np.float64)
    d[f"{prefix}/Tcw_cur"] = np.asarray(p.Tcw_cur, f32)
    d[f"{prefix}/Tcw_last"] = np.asarray(p.Tcw_last, f32)
    d[f"{prefix}/frame_occ"] = np.asarray(p.frame_occ, np.uint8)
    d[f"{prefix}/par"] = np.array([p.mb, p.th, p.check_ori], f32)
    return d


def from_arrays(z, prefix: str):
    g = lambda k: z[f"{prefix}/{k}"]
    fx, fy, cx, cy, max_x, mbf = (float(v) for v in g("K"))
    fr = make_frame(g("fr_kp"), g("fr_octave"), g("fr_desc"), g("fr_u_right"), mbf=mbf, fx=fx, fy=fy, cx=cx, cy=cy,
                    max_x=max_x)
    fr.angle = np.ascontiguousarray(g("fr_angle"), f32)
    fr.cell_feat = np.ascontiguousarray(g("fr_cell_feat"), np.int32)   # a permuted cell keeps its order
    last = last_of(*(g(f"last_{k}") for k in _LAST))
    mb, th, ori = (float(v) for v in g("par"))
    return types.SimpleNamespace(frame=fr, last=last, Tcw_cur=g("Tcw_cur"), Tcw_last=g("Tcw_last"), mb=mb,
                                 frame_occ=g("frame_occ"), th=th, check_ori=int(ori))
