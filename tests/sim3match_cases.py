"""Hand-built problems with known answers for ORBmatcher::SearchBySim3 (src/ORBmatcher.cpp:948-1170),
TEST-ONLY, shared by the CPU tests, the GPU tests and the golden fixture (sim3match_cases.npz).

groups() returns name -> (th, [(case name, case)]); a GPU test runs one group as one batch.  A case carries
kf1, kf2, R12, t12, m12 and the expected vnMatch1 (m1), vnMatch2 (m2) and out12, which are written by hand
from the comments below, never computed; UNPINNED (-9) marks the few slots that sit within an ulp or two of a
rounding decision no hand can settle (they are still compared between restatement, oracle and device).

The hand camera: fx = fy = 128, cx = 320, cy = 240, image [0, 640) x [0, 480), 64 x 48 cells of 10 px (grid
inverses 0.1), 8 levels of 1.2, identity poses and R12 = I, t12 = 0.  A point (x, y, 1) projects to
u = 128 x + 320, v = 128 y + 240, exactly in float for the dyadic x, y used; P(u, v) is the point that
projects to (u, v).  A MapPoint with mfMaxDistance = its distance predicts level 0 (ratio 1, log 0) and the
search radius is th.  A MapPoint descriptor is all zeros and a keypoint's has `bits` bits set, so the
descriptor distance is `bits`.  In the one-directional cases KF1 carries only MapPoints and KF2 only
keypoints; mirror() swaps the KeyFrames so the same rule is met by the KF2 -> KF1 direction.

Every boundary value is derived in float32 and stepped with np.nextafter until the float expression itself
changes side (asserted here), never trusted to a decimal literal.
"""
from __future__ import annotations

import types

import numpy as np

from rsc import synth

f32 = np.float32
UNPINNED = -9
I3 = np.eye(3, dtype=f32)
Z3 = np.zeros(3, f32)


def table(factor, levels):
    """mvScaleFactors as ORBextractor builds it: sf[0] = 1, sf[i] = sf[i - 1] * factor in float."""
    sf = [f32(1.0)]
    for _ in range(1, levels):
        sf.append(f32(sf[-1] * f32(factor)))
    return np.array(sf, f32)


def camera(fx=128.0, fy=128.0, cx=320.0, cy=240.0, min_x=0.0, max_x=640.0, min_y=0.0, max_y=480.0, factor=1.2,
           levels=8, R=None, t=None):
    return types.SimpleNamespace(fx=fx, fy=fy, cx=cx, cy=cy, min_x=min_x, max_x=max_x, min_y=min_y, max_y=max_y,
                                 sf=table(factor, levels), log_sf=f32(np.log(f32(factor))),
                                 gw=f32(f32(64) / f32(max_x - min_x)), gh=f32(f32(48) / f32(max_y - min_y)),
                                 R=I3 if R is None else np.asarray(R, f32), t=Z3 if t is None else np.asarray(t, f32))


HAND = camera()
FAR = (600.0, 20.0)   # where the keypoint of a slot goes when only its MapPoint matters (no case projects there)


def desc_bits(bits: int, lo: int = 0) -> np.ndarray:
    """bits [lo, lo + bits) set."""
    d = np.zeros(32, np.uint8)
    for b in range(lo, lo + bits):
        d[b // 8] |= 1 << (b % 8)
    return d


def norm(pos):
    """dist3D as the matcher forms it: sqrt((x*x + y*y) + z*z) in float."""
    x, y, z = (f32(v) for v in pos)
    return f32(np.sqrt(f32(f32(f32(x * x) + f32(y * y)) + f32(z * z))))


def proj(pos, cam=HAND):
    """(u, v) of a camera-frame point as the matcher forms it."""
    x, y, z = (f32(v) for v in pos)
    invz = f32(1.0 / np.float64(z))
    return (f32(f32(f32(cam.fx) * f32(x * invz)) + f32(cam.cx)), f32(f32(f32(cam.fy) * f32(y * invz)) + f32(cam.cy)))


def P(u, v, z=1.0):
    """The point of the hand camera's frame at depth z that projects to (u, v); asserted exact."""
    pos = (f32((u - 320.0) / 128.0 * z), f32((v - 240.0) / 128.0 * z), f32(z))
    assert proj(pos) == (f32(u), f32(v)), (u, v, z)
    return pos


def step_until(x, toward, pred):
    """The first float32 from x towards `toward` (x excluded) for which pred holds."""
    x = f32(x)
    for _ in range(8):
        x = np.nextafter(x, f32(toward))
        if pred(x):
            return x
    raise AssertionError("no float within 8 ulps satisfies the predicate")


def mp(pos, dmax=None, dmin=0.01, state=1, kp=FAR, octave=0, bits=200, mp_desc=None, desc=None):
    """A slot whose MapPoint matters: position (in the KeyFrame's world), mfMaxDistance (default: its norm,
    level 0 under identity poses), mfMinDistance, state 1 good / 2 bad; its own keypoint defaults to FAR with
    200 bits (never a match)."""
    return dict(kp=kp, octave=octave, bits=bits, desc=desc, pos=pos, dmax=norm(pos) if dmax is None else dmax,
                dmin=dmin, state=state, mp_desc=mp_desc)


def kpt(u, v, bits, octave=0, lo=0, desc=None):
    """A slot that is only a keypoint (NULL MapPoint)."""
    return dict(kp=(u, v), octave=octave, bits=bits, lo=lo, desc=desc, pos=None, dmax=0.0, dmin=0.0, state=0,
                mp_desc=None)


def make_kf(slots, cam=HAND, cell_order=None) -> synth.Sim3KF:
    n = len(slots)
    kp = np.array([s["kp"] for s in slots], f32).reshape(n, 2)
    begin, feat = synth.build_grid(kp, cam.min_x, cam.min_y, cam.gw, cam.gh)
    if cell_order is not None:   # the cell that holds these keypoints lists them in this order
        at = [int(np.nonzero(feat == j)[0][0]) for j in cell_order]
        assert sorted(at) == list(range(min(at), min(at) + len(at)))
        feat[min(at):min(at) + len(at)] = cell_order
    desc = np.array([desc_bits(s["bits"], s.get("lo", 0)) if s["desc"] is None else s["desc"] for s in slots],
                    np.uint8).reshape(n, 32)
    mdesc = np.array([np.zeros(32, np.uint8) if s["mp_desc"] is None else s["mp_desc"] for s in slots],
                     np.uint8).reshape(n, 32)
    pos = np.array([(0, 0, 0) if s["pos"] is None else s["pos"] for s in slots], f32).reshape(n, 3)
    return synth.Sim3KF(n, kp, np.array([s["octave"] for s in slots], np.int32), desc, begin, feat,
                        cam.R.copy(), cam.t.copy(), np.array([s["state"] for s in slots], np.uint8), pos,
                        np.array([s["dmax"] for s in slots], f32), np.array([s["dmin"] for s in slots], f32), mdesc,
                        np.full(n, -1, np.int64), fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, min_x=cam.min_x,
                        max_x=cam.max_x, min_y=cam.min_y, max_y=cam.max_y, scale_factors=cam.sf,
                        log_scale_factor=float(cam.log_sf), grid_w_inv=float(cam.gw), grid_h_inv=float(cam.gh))


def vec(n, d):
    a = np.full(n, -1, np.int32)
    for k, v in d.items():
        a[k] = v
    return a


def case(kf1, kf2, m1, m2=None, out=None, R12=I3, t12=Z3, m12=None):
    return types.SimpleNamespace(kf1=kf1, kf2=kf2, R12=np.asarray(R12, f32), t12=np.asarray(t12, f32),
                                 m12=np.full(kf1.n, -1, np.int32) if m12 is None else np.asarray(m12, np.int32),
                                 m1=vec(kf1.n, m1), m2=vec(kf2.n, m2 or {}), out=vec(kf1.n, out or {}))


def probe(points, kps, m1, cam2=HAND, cell_order=None):
    """KF1 = the MapPoints, KF2 = the keypoints: only KF1 -> KF2 finds anything, nothing is mutual."""
    return case(make_kf(points), make_kf(kps, cam2, cell_order), m1)


def mirror(c):
    """The same problem with the KeyFrames swapped (identity transform, equal intrinsics, nothing matched on
    entry): what KF1 -> KF2 found, KF2 -> KF1 now finds."""
    assert np.array_equal(c.R12, I3) and not c.t12.any() and (c.m12 == -1).all()
    inv = np.full(c.kf2.n, -1, np.int32)
    for i, j in enumerate(c.out):
        if j >= 0:
            inv[j] = i
    return types.SimpleNamespace(kf1=c.kf2, kf2=c.kf1, R12=c.R12, t12=c.t12, m12=np.full(c.kf2.n, -1, np.int32),
                                 m1=c.m2.copy(), m2=c.m1.copy(), out=inv)


def with_mirrors(cases):
    return cases + [(name + "/mirrored", mirror(c)) for name, c in cases]


# ---- edges (th = 8: radius 8 at level 0) ---------------------------------------------------------------------
def edges():
    out = []
    # depth and non-finite positions.  Slot 0 (0, 0, -1) is behind the camera: x / z = -0, it would project
    # to (320, 240) where keypoint 0 waits, at distance 1 = mfMaxDistance: only the depth test (:1008) stops
    # it.  Slot 1 = P(448, 240) is the control and takes keypoint 1.  z == 0: invz = inf, (1, 0, 0) -> u = inf;
    # (0, 0, 0) -> 0 * inf = NaN; z = -0.0 is not < 0, invz = -inf, 0 * -inf = NaN.  NaN / inf coordinates turn
    # the whole product NaN (0 * inf in the rotation rows).  IsInImage is false for every one of them.
    pts = [mp((0.0, 0.0, -1.0), dmax=1.0), mp(P(448, 240)), mp((1.0, 0.0, 0.0), dmax=1.0),
           mp((0.0, 0.0, 0.0), dmax=1.0), mp((0.0, 0.0, -0.0), dmax=1.0), mp((np.nan, 0.0, 1.0), dmax=1.0),
           mp((np.inf, 0.0, 1.0), dmax=1.0), mp((0.0, 0.0, np.inf), dmax=1.0), mp((0.0, -np.inf, 1.0), dmax=1.0)]
    out.append(("depth_nonfinite", probe(pts, [kpt(320, 240, 3), kpt(448, 240, 3)], {1: 1})))

    # IsInImage, min inclusive and max exclusive.  x = 2.5 -> u = 640 = mnMaxX: outside; the next float
    # below 2.5 whose u is below 640: inside, takes keypoint 0 at (634, 240) (cell 63; a keypoint at 638
    # would round to column 64 and not be in the grid at all).  x = -2.5 -> u = 0 = mnMinX: inside, keypoint 1
    # at (2, 240); one step further out: outside.  The same on y with v = 480 (y = 1.875) and v = 0.
    # All four search areas are cut by the grid's border: columns floor(-0.8) -> 0 and ceil(64.8) -> 63, rows
    # floor(-0.8) -> 0 and ceil(48.8) -> 47.
    u_of = lambda x: proj((x, 0.0, 1.0))[0]
    v_of = lambda y: proj((0.0, y, 1.0))[1]
    assert u_of(2.5) == 640 and u_of(-2.5) == 0 and v_of(1.875) == 480 and v_of(-1.875) == 0
    x_in = step_until(2.5, 0, lambda x: u_of(x) < 640)
    x_out = step_until(-2.5, -3, lambda x: u_of(x) < 0)
    y_in = step_until(1.875, 0, lambda y: v_of(y) < 480)
    y_out = step_until(-1.875, -3, lambda y: v_of(y) < 0)
    pts = [mp((2.5, 0.0, 1.0)), mp((x_in, 0.0, 1.0)), mp((-2.5, 0.0, 1.0)), mp((x_out, 0.0, 1.0)),
           mp((0.0, 1.875, 1.0)), mp((0.0, y_in, 1.0)), mp((0.0, -1.875, 1.0)), mp((0.0, y_out, 1.0))]
    kps = [kpt(634, 240, 3), kpt(2, 240, 3), kpt(320, 474, 3), kpt(320, 2, 3)]
    out.append(("image_bounds", probe(pts, kps, {1: 0, 2: 1, 5: 2, 6: 3})))

    # dist3D in [0.8 mfMinDistance, 1.2 mfMaxDistance], both ends inside; all on the axis -> (320, 240),
    # keypoint 0.  (0, 0, 3): 1.2f * 2.5 = 3 + 2^-23 ties to 3.0 = dist3D: not above, kept (ratio 0.83 -> level
    # 0); with the first mfMaxDistance below 2.5 whose bound is below 3: rejected.  (0, 0, 2): 0.8f * 2.5 rounds
    # to 2.0 = dist3D: not below, kept; with the first mfMinDistance above 2.5 whose bound exceeds 2: rejected.
    assert f32(f32(1.2) * f32(2.5)) == 3 and f32(f32(0.8) * f32(2.5)) == 2
    dmax_out = step_until(2.5, 0, lambda d: f32(f32(1.2) * d) < 3)
    dmin_out = step_until(2.5, 3, lambda d: f32(f32(0.8) * d) > 2)
    pts = [mp((0.0, 0.0, 3.0), dmax=2.5), mp((0.0, 0.0, 3.0), dmax=dmax_out),
           mp((0.0, 0.0, 2.0), dmax=2.0, dmin=2.5), mp((0.0, 0.0, 2.0), dmax=2.0, dmin=dmin_out)]
    out.append(("distance_bounds", probe(pts, [kpt(320, 240, 3)], {0: 0, 2: 0})))

    # |dx| < r and |dy| < r are strict (KeyFrame.cpp:590).  Slot 0 -> (320, 240): keypoint 0 at (328, 240)
    # has |dx| = 8 = r: not a candidate, nothing else is near.  Slot 1 -> (320, 112): keypoint 1 one float
    # below 328: taken.  Slots 2, 3: the same on y at (192, 240) / (192, 112).  Slot 4 -> (448, 240): columns
    # floor(44.0) = 44 .. ceil(45.6) = 46; keypoint 4 at (455.5, 240) has |dx| = 7.5 and lies in column
    # round(45.55) = 46, which only ceil reaches.
    pts = [mp(P(320, 240)), mp(P(320, 112)), mp(P(192, 240)), mp(P(192, 112)), mp(P(448, 240))]
    kps = [kpt(328, 240, 3), kpt(np.nextafter(f32(328), f32(0)), 112, 3), kpt(192, 248, 3),
           kpt(192, np.nextafter(f32(120), f32(0)), 3), kpt(455.5, 240, 3)]
    out.append(("radius_and_ceil_cell", probe(pts, kps, {1: 1, 3: 3, 4: 4})))

    # bestDist <= TH_HIGH = 100 (:1064): 100 bits is a match, 101 is not
    out.append(("th_high", probe([mp(P(192, 240)), mp(P(448, 240))], [kpt(192, 240, 100), kpt(448, 240, 101)],
                                 {0: 0})))
    return with_mirrors(out)


# ---- levels (th = 8) -----------------------------------------------------------------------------------------
def ulps(a, b):
    return int(f32(a).view(np.int32)) - int(f32(b).view(np.int32))


def levels():
    """PredictScale = ceil(log(mfMaxDistance / dist) / log 1.2), clamped to [0, 7], at every power of 1.2.
    Sites 64 px apart (the largest radius is 8 * 1.2^7 = 28.7).  Per level k five MapPoints whose ratio sits
    64 ulps below sf[k], 3 ulps below, at it, 3 above and 64 above (each within 2 ulps of that, asserted).  The
    three nearest are unpinned, except k = 0 on the optical axis where the ratio is exactly 1.  62 ulps of the ratio move log(ratio) / log 1.2 by >= 2e-5, while the float
    table entry sf[k] is off 1.2^k by < 2.5e-6 in that quotient and the float evaluation (log, log 1.2, the
    division) by ~1e-6 at level 7, so below -> level k and above -> level k + 1 can be written by hand; the
    decision within a few ulps is left to the unpinned points and the comparison with the oracle.
    Each site has keypoint `lo` (octave max(k - 1, 0), 5 bits) and, for k < 7, `hi` (octave k + 1, 3 bits)
    2 px to the right: level k admits octaves [k - 1, k], so only lo; level k + 1 admits [k, k + 1], so hi
    (for k = 0 both, hi is better).  The index taken therefore shows the level."""
    sf = HAND.sf
    sites = [(64 * (1 + c), 48 + 64 * r) for r in range(6) for c in range(9)]
    sites.remove((320, 240))
    pts, kps, m1 = [], [], {}

    def site_for(k, side):
        return (320, 240) if (k, side) == (0, 0) else sites.pop(0)

    for k in range(8):
        for side in (-64, -3, 0, 3, 64):
            u, v = site_for(k, side)
            pos = P(u, v)
            d = norm(pos)
            want = (sf[k].view(np.int32) + np.int32(side)).view(f32)   # sf[k] moved by `side` ulps
            dmax = f32(want * d)
            off = ulps(f32(dmax / d), sf[k])
            assert abs(off - side) <= 2, (k, side, off)
            lo = len(kps)
            kps.append(kpt(u, v, 5, octave=max(k - 1, 0)))
            if k < 7:
                kps.append(kpt(u + 2, v, 3, octave=k + 1))
            if (k, side) == (0, 0):
                assert f32(dmax / d) == 1
            if abs(side) <= 3 and (k, side) != (0, 0):
                m1[len(pts)] = UNPINNED
            elif side < 0 or k == 7 or (k, side) == (0, 0):
                m1[len(pts)] = lo          # level k (k = 7 above: 8 clamped to 7)
            else:
                m1[len(pts)] = lo + 1      # level k + 1
            pts.append(mp(pos, dmax=dmax))
    # a ratio far above 1.2^7: ceil(log 100 / log 1.2) = 26 -> clamped to 7: octave 6 is admitted
    u, v = sites.pop(0)
    m1[len(pts)] = len(kps)
    pts.append(mp(P(u, v), dmax=f32(100.0 * norm(P(u, v)))))
    kps.append(kpt(u, v, 3, octave=6))
    # octaves L - 2 .. L + 1 around L = 3 (ratio 1.2^2 * 1.1): octave 1 (1 bit) and 4 (2 bits) carry the best
    # descriptors but are outside [2, 3]; of octave 2 (9 bits) and 3 (5 bits) the latter wins
    u, v = sites.pop(0)
    m1[len(pts)] = len(kps) + 2
    pts.append(mp(P(u, v), dmax=f32(sf[2] * f32(1.1) * norm(P(u, v)))))
    kps += [kpt(u - 2, v, 1, octave=1), kpt(u - 1, v, 9, octave=2), kpt(u + 1, v, 5, octave=3),
            kpt(u + 2, v, 2, octave=4)]
    out = [("powers", probe(pts, kps, m1))]
    # the lower clamp needs log(ratio) / log sf <= -1 while dist3D <= 1.2 mfMaxDistance, i.e. a scale factor
    # below 1.2: destination with 1.1.  (0, 0, 2.3) with mfMaxDistance 2: ratio 0.87, log / log 1.1 = -1.47,
    # ceil = -1 -> clamped to 0, radius 8, keypoint 0 (octave 0) at (320, 240)
    fine = camera(factor=1.1)
    c = case(make_kf([mp((0.0, 0.0, 2.3), dmax=2.0)], fine), make_kf([kpt(320, 240, 3)], fine), {0: 0})
    out.append(("clamp_low", c))
    return with_mirrors(out)


# ---- ties (th = 8) -------------------------------------------------------------------------------------------
def ties():
    """Equal minimum distances: the first in GetFeaturesInArea's visiting order (ix, then iy, then the cell's
    own order) wins (`dist < bestDist`, :1054).  One MapPoint P(320, 240): columns 31..33, rows 23..25."""
    A, B, C = 0, 8, 16   # different descriptors of equal weight: bits [lo, lo + 4)
    pt = [mp(P(320, 240))]
    out = [
        # column 31 is visited before column 33: keypoint 1 wins although its index is higher
        ("columns_high_index", probe(pt, [kpt(326, 240, 4, lo=A), kpt(314, 240, 4, lo=B)], {0: 1})),
        # the same with the indices the other way: keypoint 0 (the last minimum would be 1)
        ("columns_low_index", probe(pt, [kpt(314, 240, 4, lo=A), kpt(326, 240, 4, lo=B)], {0: 0})),
        # one column, row 23 before row 25: keypoint 1
        ("rows", probe(pt, [kpt(320, 246, 4, lo=A), kpt(320, 234, 4, lo=B)], {0: 1})),
        # one cell (32, 24), listed [0, 1]: keypoint 0; listed [1, 0] (the ABI takes the order as given): 1
        ("cell_ascending", probe(pt, [kpt(321, 241, 4, lo=A), kpt(322, 242, 4, lo=B)], {0: 0})),
        ("cell_permuted", probe(pt, [kpt(321, 241, 4, lo=A), kpt(322, 242, 4, lo=B)], {0: 1}, cell_order=[1, 0])),
        # three-way: cells (32, 24), (32, 23), (31, 25): column 31 first: keypoint 2
        ("three_way", probe(pt, [kpt(322, 242, 4, lo=A), kpt(320, 234, 4, lo=B), kpt(314, 246, 4, lo=C)], {0: 2})),
        # a tie at exactly TH_HIGH: bits [0, 100) and [100, 200), column 31 first: keypoint 1, still a match
        ("tie_at_100", probe(pt, [kpt(326, 240, 100, lo=0), kpt(314, 240, 100, lo=100)], {0: 1})),
    ]
    return with_mirrors(out)


# ---- agree (th = 8) ------------------------------------------------------------------------------------------
def agree():
    S = [(64 * (1 + k), 48) for k in range(7)]   # sites 64 px apart, level 0, radius 8
    here = lambda k, dx=0, **kw: mp(P(*S[k]), kp=(S[k][0] + dx, S[k][1]), **kw)
    kf1 = make_kf([
        here(0, bits=3),              # 0  A: mutual with KF2 slot 0
        here(1, bits=3),              # 1  B: -> KF2 slot 1, but that one prefers slot 2
        kpt(S[1][0] + 2, S[1][1], 1),  # 2  B: a keypoint with the better descriptor, no MapPoint
        here(2, bits=3),              # 3  C: -> KF2 slot 2, which answers 3 (3 bits against 5)
        here(2, dx=2, bits=5),        # 4  C: -> KF2 slot 2 as well
        here(3, dx=3, bits=7),        # 5  D: matched12 = 3: not searched, KF2 slot 3 is vbAlreadyMatched2
        here(3, bits=3),              # 6  D: -> KF2 slot 3 all the same (forward ignores vbAlreadyMatched2)
        here(4, bits=3),              # 7  E: matched12 = -2 (a MapPoint not in KF2): not searched
        here(3, dx=5, bits=9),        # 8  D: matched12 = 3 again (two entries naming one idx2)
        here(5, bits=3, state=2),     # 9  F: bad MapPoint
        kpt(S[6][0], S[6][1], 3),     # 10 G: NULL
    ])
    kf2 = make_kf([here(0, bits=3), here(1, bits=3), here(2, bits=3), here(3, bits=3), here(4, bits=3),
                   kpt(S[5][0], S[5][1], 3), here(6, bits=3, state=2)])
    m12 = [-1, -1, -1, -1, -1, 3, -1, -2, 3, -1, -1]
    # forward: 0 -> 0, 1 -> 1, 3 -> 2, 4 -> 2, 6 -> 3; 2 and 10 NULL, 5, 7, 8 already matched, 9 bad.
    # backward: 0 -> 0; 1 -> KF1's 2 (1 bit beats 3); 2 -> 3 (3 bits beat 5); 3 already matched; 4 -> 7 (the
    # keypoint of an already matched slot is still a candidate); 5 NULL; 6 bad.
    # agreement: 0 (0 <-> 0) and 3 (3 -> 2 -> 3); 1 fails (1 -> 2), 4 fails (2 -> 3), 6 fails (3 not searched).
    out = [("rules", case(kf1, kf2, {0: 0, 1: 1, 3: 2, 4: 2, 6: 3}, {0: 0, 1: 2, 2: 3, 4: 7}, {0: 0, 3: 2}, m12=m12))]
    # a KeyFrame paired with itself under the identity: every good slot matches itself (its descriptor is its
    # own keypoint's); slot 2 is NULL and slot 4 bad
    own = [desc_bits(6, lo=10 * k) for k in range(6)]
    kfs = make_kf([here(k, desc=own[k], mp_desc=own[k], state=(0 if k == 2 else 2 if k == 4 else 1))
                   for k in range(6)])
    same = {0: 0, 1: 1, 3: 3, 5: 5}
    out.append(("self", case(kfs, kfs, same, same, same)))
    return out


# ---- frames (th = 7.5) ---------------------------------------------------------------------------------------
def frames():
    """KF1 and KF2 differ in intrinsics, image bounds (negative minima), level count (8 / 5), scale factor
    (1.2 / 1.3) and grid inverses (0.1 / 0.08), and both poses are non-trivial:
      KF1: fx = fy = 128, cx = 320, cy = 240, image [-13, 627) x [-12, 468), Rcw = Rz(90 deg), tcw = (0.5, -0.25, 1)
      KF2: fx = 96, fy = 160, cx = 256, cy = 192, image [-16, 784) x [-8, 592), Rcw = I, tcw = (-0.5, 0.25, 0.5)
      R12 = R1 R2^T = Rz(90 deg), t12 = t1 - R12 t2 = (0.75, 0.25, 0.5); everything dyadic, so exact in float.
    Projections use pKF1's intrinsics in BOTH directions: a point (X, Y, 2) of either destination camera
    lands at u = 64 X + 320, v = 64 Y + 240.  Forward MapPoints are given by their KF2 camera coordinates p2
    (world = p2 - t2), backward ones by their KF1 camera coordinates p1 (world = R1^T (p1 - t1)).
    KF1 slots 0-5 are the forward MapPoints, 6-14 keypoints j0-j8; KF2 slots 0-7 are keypoints k0-k7, 8-13
    the backward MapPoints.  Radius 7.5 * sf[level] of the destination."""
    R1 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f32)
    t1, t2 = np.array([0.5, -0.25, 1.0], f32), np.array([-0.5, 0.25, 0.5], f32)
    c1 = camera(128, 128, 320, 240, -13, 627, -12, 468, 1.2, 8, R1, t1)
    c2 = camera(96, 160, 256, 192, -16, 784, -8, 592, 1.3, 5, I3, t2)
    assert c1.gw == f32(0.1) and c2.gw == f32(0.08) and c2.gh == f32(0.08)
    fwd = lambda p2: tuple(np.asarray(p2, f32) - t2)
    bwd = lambda p1: tuple(R1.T @ (np.asarray(p1, f32) - t1))
    far1, far2 = (620.0, 460.0), (700.0, 560.0)
    s17 = norm((2.0, -3.0, 2.0))
    kf1 = make_kf([
        # 0 (a): p2 = (2, 1, 2), dist 3 -> (448, 304) = k0; with KF2's intrinsics (352, 272) = decoy k1
        mp(fwd((2, 1, 2)), dmax=3.0, kp=far1, octave=7),
        # 1 (f): p2 = (2, -1, 2) -> (448, 176); k2 at (454, 176) lies in column round(470 * .08) = 38, reached by
        #   floor(456.5 * .08) = 36 .. ceil(471.5 * .08) = 38 but not by 35 .. 37 without the + 16
        mp(fwd((2, -1, 2)), dmax=3.0, kp=far1, octave=7),
        # 2 (e): p2 = (6, 0, 2) -> (704, 240) = k3: inside KF2's image, outside KF1's (mnMaxX 627)
        mp(fwd((6, 0, 2)), dmax=norm((6.0, 0.0, 2.0)), kp=far1, octave=7),
        # 3 (i, log factor): p2 = (-2, 1, 2) -> (192, 304), ratio 3.75 / 3 = 1.25: log 1.25 / log 1.3 = 0.85 ->
        #   level 1 -> octaves [0, 1] -> k4 (octave 0); with log 1.2: 1.22 -> level 2 -> k5 (octave 2, better)
        mp(fwd((-2, 1, 2)), dmax=3.75, kp=far1, octave=7),
        # 4 (i, level count): p2 = (-2, -1, 2) -> (192, 176), ratio 12.75 / 3 = 4.25: log / log 1.3 = 5.5 -> 6,
        #   clamped to 4 of KF2's 5 levels -> octaves [3, 4] -> k6 (octave 3); with 8 levels: level 6, nothing
        mp(fwd((-2, -1, 2)), dmax=12.75, kp=far1, octave=7),
        # 5 (j): p2 = (2, -3, 2) -> (448, 48), ratio 1.25 -> level 1, radius 7.5 * 1.3 = 9.75: k7 at |dx| = 9.5
        #   is inside; with KF1's table the radius is 9.0 and it is not
        mp(fwd((2, -3, 2)), dmax=f32(f32(1.25) * s17), kp=far1, octave=7),
        kpt(384, 304, 5),             # 6  j0: backward slot 8 lands here
        kpt(304, 272, 3),             # 7  j1: where KF2's intrinsics would put it
        kpt(327, 176, 3),             # 8  j2
        kpt(-9, 240, 3),              # 9  j3
        kpt(192, 304, 5, octave=0),   # 10 j4
        kpt(194, 304, 3, octave=2),   # 11 j5
        kpt(192, 176, 3, octave=6),   # 12 j6
        kpt(448, 48, 9, octave=2),    # 13 j7
        kpt(460, 48, 3, octave=2),    # 14 j8
    ], c1)
    s6, s5 = norm((1.0, 1.0, 2.0)), norm((0.0, -1.0, 2.0))
    xe = -5.2265625   # 64 * xe + 320 = -14.5
    kf2 = make_kf([
        kpt(448, 304, 5), kpt(352, 272, 3), kpt(454, 176, 3), kpt(704, 240, 3),   # k0 - k3
        kpt(192, 304, 5, octave=0), kpt(194, 304, 3, octave=2), kpt(192, 176, 3, octave=3),   # k4 - k6
        kpt(457.5, 48, 3, octave=1),                                               # k7
        # 8 (a): p1 = (1, 1, 2) -> (384, 304) = j0; with KF2's (the source's) intrinsics (304, 272) = decoy j1
        mp(bwd((1, 1, 2)), dmax=s6, kp=far2, octave=4),
        # 9 (f): p1 = (0, -1, 2) -> (320, 176); j2 at (327, 176) lies in column round(340 * .1) = 34, reached by
        #   floor(325.5 * .1) = 32 .. ceil(340.5 * .1) = 35 but not by 31 .. 33 without the + 13
        mp(bwd((0, -1, 2)), dmax=s5, kp=far2, octave=4),
        # 10 (e): p1 = (xe, 0, 2) -> (-14.5, 240): outside KF1's image (mnMinX -13), inside KF2's (-16): not
        #   searched; with the source's bounds it would take j3 at (-9, 240)
        mp(bwd((xe, 0, 2)), dmax=norm((xe, 0.0, 2.0)), kp=far2, octave=4),
        # 11 (i, log factor): p1 = (-2, 1, 2) -> (192, 304), ratio 1.25: log / log 1.2 = 1.22 -> level 2 ->
        #   octaves [1, 2] -> j5; with log 1.3: level 1 -> [0, 1] -> j4
        mp(bwd((-2, 1, 2)), dmax=3.75, kp=far2, octave=4),
        # 12 (i, level count): p1 = (-2, -1, 2) -> (192, 176), ratio 9.9 / 3 = 3.3: log / log 1.2 = 6.55 -> 7 ->
        #   octaves [6, 7] -> j6; with KF2's 5 levels: clamped to 4, nothing
        mp(bwd((-2, -1, 2)), dmax=9.9, kp=far2, octave=4),
        # 13 (j): p1 = (2, -3, 2) -> (448, 48), ratio 1.25 -> level 2, radius 7.5 * 1.44 = 10.8: j7 (9 bits) at
        #   the projection; j8 (3 bits) at |dx| = 12 is outside, but inside KF2's 7.5 * 1.69 = 12.7
        mp(bwd((2, -3, 2)), dmax=f32(f32(1.25) * s17), kp=far2, octave=4),
    ], c2)
    t12 = t1 - R1 @ t2
    assert np.array_equal(t12, np.array([0.75, 0.25, 0.5], f32))
    # nothing is mutual: the forward matches end on NULL slots of KF2 and the backward ones on NULL slots of KF1
    c = case(kf1, kf2, {0: 0, 1: 2, 2: 3, 3: 4, 4: 6, 5: 7}, {8: 6, 9: 8, 11: 11, 12: 12, 13: 13}, {}, R12=R1, t12=t12)
    return [("two_cameras", c)]


# ---- shapes (th = 7.5) ---------------------------------------------------------------------------------------
SHAPE_PAIRS = [(0, 64), (64, 0), (1, 1), (63, 65), (65, 63), (64, 64), (255, 256), (256, 257), (257, 255),
               (513, 513), (513, 1), (64, 513), (1, 257)]


def lattice_kf(n, rev, _cache={}):
    """n slots on a 20 px lattice (sites (10 + 20 a, 10 + 20 b), 32 per row; neighbours are outside the
    radius 7.5): slot i sits on site i, or on site n - 1 - i when rev; keypoint, MapPoint (level 0) and both
    descriptors (the site number) belong to the site, so a slot can only match the other KeyFrame's slot on
    the same site."""
    if (n, rev) not in _cache:
        slots = []
        for i in range(n):
            s = n - 1 - i if rev else i
            u, v = 10 + 20 * (s % 32), 10 + 20 * (s // 32)
            d = np.zeros(32, np.uint8)
            d[0], d[1] = s & 255, s >> 8
            slots.append(mp(P(u, v), kp=(u, v), desc=d, mp_desc=d))
        _cache[(n, rev)] = make_kf(slots)
    return _cache[(n, rev)]


def shapes():
    """Sizes around the 64-lane, 256-thread and multi-block limits in one heterogeneous batch (the launch grid
    follows the largest).  KF1 in site order, KF2 reversed: KF1 slot i and KF2 slot n2 - 1 - i share site i, so
    m1[i] = n2 - 1 - i for i < n2, m2[j] = n2 - 1 - j where that is below n1, and every pair of slots on a common
    site is mutual: nFound = min(n1, n2), 513 for the largest pair.  KeyFrame objects are shared between pairs."""
    out = []
    for n1, n2 in SHAPE_PAIRS:
        m1 = {i: n2 - 1 - i for i in range(min(n1, n2))}
        m2 = {j: n2 - 1 - j for j in range(n2) if n2 - 1 - j < n1}
        out.append((f"{n1}x{n2}", case(lattice_kf(n1, False), lattice_kf(n2, True), m1, m2, dict(m1))))
    return out


def groups():
    """name -> (th, [(case name, case)])."""
    return {"frames": (7.5, frames()), "edges": (8.0, edges()), "levels": (8.0, levels()), "ties": (8.0, ties()),
            "agree": (8.0, agree()), "shapes": (7.5, shapes())}
