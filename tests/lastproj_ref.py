"""Sequential restatement of ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th)
(src/ORBmatcher.cpp:1173-1315) and of Tracking::TrackWithMotionModel (src/Tracking.cpp:724-774), the reference
the device kernels are compared with bit for bit (TEST-ONLY), written from the reference text and independent of
csrc/rsc_lastproj.h:

* ``level_mode``: bForward / bBackward (:1183-1194);
* ``search_by_projection_last``: the matcher, slot by slot on an explicit ``mvpMapPoints`` list, with a trace;
* ``fixed_point_rounds``: the rounds of the device mapping restated on the same functions (round count);
* ``run_track_motion_model``: the driver's replay with oracle_lib.pose_optimization;
* ``PERTURBATIONS``: single rules switched off, to show that the cases pin each of them.

Every operation rounds to its type, fixed-size sums run left to right.  A problem is a namespace with frame
(rsc.synth.ProjFrame plus u_right, mbf), last (n, octave, angle, mp_state, mp_pos, mp_desc, mp_has_obs),
Tcw_cur, Tcw_last, mb, frame_occ, th, check_ori.
"""
from __future__ import annotations

import types

import numpy as np

import localproj_ref as lr
from rsc import synth

f32 = np.float32
TH_HIGH = 100
HISTO_LENGTH = 30
MODE_WINDOW, MODE_FORWARD, MODE_BACKWARD = 0, 1, 2
_POP = lr._POP

# trace reason codes, one per LastFrame slot
NO_POINT, OUTLIER, DEPTH, BOUNDS, NAN_PIXEL, EMPTY_WINDOW, NO_FREE, ABOVE_TH, MATCHED = range(9)

# name -> what the switched-off rule becomes
PERTURBATIONS = {
    "bounds_exclusive": "u <= mnMinX || u >= mnMaxX",
    "invz_le_zero": "invzc <= 0 rejects",
    "invz_float_division": "invzc = 1.0f / z",
    "radius_inclusive": "fabs(dx) <= r",
    "forward_window_levels": "forward mode searches [o-1, o+1]",
    "levels_o_minus_1_to_o": "window mode searches [o-1, o]",
    "stereo_gate_dropped": "no stereo gate",
    "stereo_gate_ge_zero": "the gate applies when mvuRight >= 0",
    "occupancy_ignores_obs": "any occupant blocks",
    "last_minimum_ties": "dist <= bestDist",
    "th_high_strict": "bestDist < TH_HIGH",
    "histogram_surviving_only": "one histogram entry per feature, from its last claimer",
    "removal_last_writer_only": "a removed entry nulls its feature only when it is the last claimer",
    "no_ten_percent_rule": "ComputeThreeMaxima keeps the three largest bins",
    "angle_order_swapped": "rot = current angle - last angle",
}


# Two of them cannot change any output on inputs inside the reference's defined behaviour, and
# tests/test_cpu_lastproj.py proves that instead of looking for a case:
# * invzc == 0 needs an infinite z (1 / FLT_MAX is a non-zero subnormal), and an infinite coordinate makes
#   xc = 0 * inf or u = (fx * inf) * 0 a NaN, which is outside the defined behaviour;
# * 1.0f / z and (float)(1.0 / (double)z) are the same float for every significand of z (all 2^23 are
#   enumerated; both scale exactly with the exponent).
UNOBSERVABLE = ("invz_le_zero", "invz_float_division")


def _dot3(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def level_mode(Tcw_cur, Tcw_last, mb) -> int:
    """:1183-1194: 1 forward, 2 backward, 0 neither."""
    Tc, Tl = np.asarray(Tcw_cur, f32).reshape(4, 4), np.asarray(Tcw_last, f32).reshape(4, 4)
    with np.errstate(all="ignore"):
        twc = [f32(-_dot3(Tc[:3, r], Tc[:3, 3])) for r in range(3)]                       # :1186
        tlcz = f32(_dot3(Tl[2, :3], twc) + Tl[2, 3])                                      # :1191
        if tlcz > f32(mb):                                                                # :1193
            return MODE_FORWARD
        if f32(-tlcz) > f32(mb):                                                          # :1194
            return MODE_BACKWARD
    return MODE_WINDOW


def three_maxima(sizes, off=()):
    """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cpp:1446-1487) on the bin sizes."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        s = int(s)
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if "no_ten_percent_rule" not in off:
        if f32(max2) < f32(f32(0.1) * f32(max1)):
            ind2 = ind3 = -1
        elif f32(max3) < f32(f32(0.1) * f32(max1)):
            ind3 = -1
    return ind1, ind2, ind3


def rot_bin(angle_last, angle_cur, off=()) -> int:
    """:1278-1283."""
    a, b = (angle_cur, angle_last) if "angle_order_swapped" in off else (angle_last, angle_cur)
    rot = f32(f32(a) - f32(b))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b_ = int(np.floor(float(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH)))) + 0.5))  # round(): rot >= 0 here
    return 0 if b_ == HISTO_LENGTH else b_


def project(p, i, off=()):
    """:1205-1226 for slot i: (reason, None) or (None, (u, v, ur, radius, octave))."""
    fr, T = p.frame, np.asarray(p.Tcw_cur, f32).reshape(4, 4)
    with np.errstate(all="ignore"):
        X = np.asarray(p.last.mp_pos[i], f32)
        xc, yc, zc = (f32(f32(f32(f32(T[r, 0] * X[0]) + f32(T[r, 1] * X[1])) + f32(T[r, 2] * X[2])) + T[r, 3])
                      for r in range(3))                                                  # :1206
        if "invz_float_division" in off:
            invzc = f32(f32(1.0) / zc)
        else:
            invzc = f32(1.0 / np.float64(zc))                                             # :1210
        if invzc < 0 or ("invz_le_zero" in off and invzc <= 0):                           # :1212
            return DEPTH, None
        u = f32(f32(f32(f32(fr.fx) * xc) * invzc) + f32(fr.cx))                           # :1215
        v = f32(f32(f32(f32(fr.fy) * yc) * invzc) + f32(fr.cy))
        if "bounds_exclusive" in off:
            if u <= f32(fr.min_x) or u >= f32(fr.max_x) or v <= f32(fr.min_y) or v >= f32(fr.max_y):
                return BOUNDS, None
        if u < f32(fr.min_x) or u > f32(fr.max_x):                                        # :1218
            return BOUNDS, None
        if v < f32(fr.min_y) or v > f32(fr.max_y):                                        # :1220
            return BOUNDS, None
        if np.isnan(u) or np.isnan(v):   # passes both tests and reaches floor: outside the reference's defined
            return NAN_PIXEL, None       # behaviour, skipped
        o = int(p.last.octave[i])                                                         # :1223
        radius = f32(f32(p.th) * synth.scale_factors()[o])                                # :1226
        ur = f32(u - f32(f32(fr.mbf) * invzc))                                            # :1254
    return None, (u, v, ur, radius, o)


def _area(fr, x, y, r, lo, hi, off=()):
    """GetFeaturesInArea (Frame.cpp:394-447), optionally with an inclusive radius."""
    if "radius_inclusive" not in off:
        return lr.features_in_area(fr, x, y, r, lo, hi)
    wide = lr.features_in_area(fr, x, y, np.nextafter(r, f32(np.inf)), lo, hi)
    return [f for f in wide if abs(f32(fr.kp[f, 0] - x)) <= r and abs(f32(fr.kp[f, 1] - y)) <= r]


def window(p, mode, u, v, radius, o, off=()):
    """:1230-1235."""
    fr = p.frame
    if mode == MODE_FORWARD and "forward_window_levels" not in off:
        return _area(fr, u, v, radius, o, -1, off)
    if mode == MODE_BACKWARD:
        return _area(fr, u, v, radius, 0, o, off)
    if mode == MODE_WINDOW and "levels_o_minus_1_to_o" in off:
        return _area(fr, u, v, radius, o - 1, o, off)
    return _area(fr, u, v, radius, o - 1, o + 1, off)


def best_free(p, i, idx, ur, radius, blocked, off=()):
    """:1242-1269: (bestDist, bestIdx2) over the window `idx`; blocked[f]: mvpMapPoints[f] is set and has
    Observations() > 0."""
    fr = p.frame
    best_dist, best_idx = 256, -1
    for f in idx:
        if blocked[f]:                                                                    # :1248-1250
            continue
        gated = fr.u_right[f] >= 0 if "stereo_gate_ge_zero" in off else fr.u_right[f] > 0  # :1252
        if gated and "stereo_gate_dropped" not in off:
            er = f32(abs(f32(ur - fr.u_right[f])))                                        # :1255
            if er > radius:                                                               # :1256
                continue
        d = int(_POP[np.bitwise_xor(fr.desc[f], p.last.mp_desc[i])].sum())                # :1262
        if d < best_dist or ("last_minimum_ties" in off and d <= best_dist):              # :1264
            best_dist, best_idx = d, f
    return best_dist, best_idx


def _accept(best_dist, off=()):
    return best_dist < TH_HIGH if "th_high_strict" in off else best_dist <= TH_HIGH       # :1271


def finish(p, claim, off=()):
    """:1292-1312 from the claims in slot order: (nmatches, out, bins).  out[f]: >= 0 the slot left in
    mvpMapPoints[f], -1 untouched, -2 set to nullptr."""
    fr, last = p.frame, p.last
    out = np.full(fr.n, -1, np.int32)
    bins = np.full(last.n, -1, np.int32)
    claimers = [i for i in range(last.n) if claim[i] >= 0]
    for i in claimers:
        out[claim[i]] = i                                                                 # :1273
    nmatches = len(claimers)                                                              # :1274
    if not p.check_ori:
        return nmatches, out, bins
    hist = [[] for _ in range(HISTO_LENGTH)]
    for i in claimers:
        bins[i] = rot_bin(last.angle[i], fr.angle[claim[i]], off)
        if "histogram_surviving_only" in off and out[claim[i]] != i:
            continue
        hist[bins[i]].append(i)                                                           # :1285
    keep = three_maxima([len(h) for h in hist], off)                                      # :1299
    final = out.copy()
    for b in range(HISTO_LENGTH):                                                         # :1301-1311
        if b in keep:
            continue
        for i in hist[b]:
            if "removal_last_writer_only" not in off or out[claim[i]] == i:
                final[claim[i]] = -2                                                      # :1307
            nmatches -= 1                                                                 # :1308
    return nmatches, final, bins


def search_by_projection_last(p, trace=None, off=()):
    """ORBmatcher.cpp:1173-1315.  Returns (nmatches, out int32[frame n], mode).  Inputs are not modified.
    With a dict in `trace`: reason[i], claim[i], bin[i], claimers (per feature) and walked (the slots whose
    four best entry-free candidates <= TH_HIGH were all blocked when their turn came and that had more)."""
    fr, last = p.frame, p.last
    mode = level_mode(p.Tcw_cur, p.Tcw_last, p.mb)
    occ = np.asarray(p.frame_occ)
    blocked = (occ != 0) if "occupancy_ignores_obs" in off else (occ == 2)
    entry_blocked = blocked.copy()
    claim = np.full(last.n, -1, np.int32)
    reason = np.full(last.n, NO_POINT, np.int32)
    walked = []
    for i in range(last.n):                                                               # :1196
        if last.mp_state[i] == 0:                                                         # :1200
            continue
        if last.mp_state[i] != 1:                                                         # :1202
            reason[i] = OUTLIER
            continue
        why, pr = project(p, i, off)
        if why is not None:
            reason[i] = why
            continue
        u, v, ur, radius, o = pr
        idx = window(p, mode, u, v, radius, o, off)
        if not idx:                                                                       # :1237
            reason[i] = EMPTY_WINDOW
            continue
        best_dist, best_idx = best_free(p, i, idx, ur, radius, blocked, off)
        if trace is not None:
            ds = sorted((int(_POP[np.bitwise_xor(fr.desc[f], last.mp_desc[i])].sum()), k, f)
                        for k, f in enumerate(idx) if not entry_blocked[f]
                        and best_free(p, i, [f], ur, radius, entry_blocked, off)[1] == f)
            ds = [t for t in ds if t[0] <= TH_HIGH]
            if len(ds) > 4 and all(blocked[f] for _, _, f in ds[:4]):
                walked.append(i)
        if best_idx < 0:
            reason[i] = NO_FREE
            continue
        if not _accept(best_dist, off):
            reason[i] = ABOVE_TH
            continue
        reason[i] = MATCHED
        claim[i] = best_idx
        blocked[best_idx] = True if "occupancy_ignores_obs" in off else bool(last.mp_has_obs[i])
    nmatches, out, bins = finish(p, claim, off)
    if trace is not None:
        trace.update(reason=reason, claim=claim, bin=bins, walked=walked,
                     claimers=np.bincount(claim[claim >= 0], minlength=fr.n))
    return nmatches, out, mode


def fixed_point_rounds(p):
    """The rounds of the device mapping restated on the functions above: every round rebuilds blocked[f] for
    slot i = (an entry occupant with observations, or a slot j < i with observations claims f) from the claims
    of the round before and lets every slot decide again, until a round changes no claim.  Returns (claim
    int32[last n], rounds, claim after round 1)."""
    fr, last = p.frame, p.last
    mode = level_mode(p.Tcw_cur, p.Tcw_last, p.mb)
    entry_blocked = np.asarray(p.frame_occ) == 2
    gw, gh = f32(synth.GRID_W_INV), f32(synth.GRID_H_INV)
    win = {}
    for i in range(last.n):
        if last.mp_state[i] != 1:
            continue
        why, pr = project(p, i)
        if why is not None:
            continue
        u, v, ur, radius, o = pr
        # the kernel's bound counts the slots whose cell range is not empty, not those with a feature in it
        x0 = max(0, int(np.floor(f32(f32(f32(u - f32(fr.min_x)) - radius) * gw))))
        x1 = min(lr.GRID_COLS - 1, int(np.ceil(f32(f32(f32(u - f32(fr.min_x)) + radius) * gw))))
        y0 = max(0, int(np.floor(f32(f32(f32(v - f32(fr.min_y)) - radius) * gh))))
        y1 = min(lr.GRID_ROWS - 1, int(np.ceil(f32(f32(f32(v - f32(fr.min_y)) + radius) * gh))))
        if x0 >= lr.GRID_COLS or x1 < 0 or y0 >= lr.GRID_ROWS or y1 < 0:
            continue
        win[i] = (window(p, mode, u, v, radius, o), ur, radius)
    claim = np.full(last.n, -1, np.int32)
    first = None
    rounds = 0
    big = np.iinfo(np.int32).max
    for _ in range(len(win) + 1):
        owner = np.where(entry_blocked, -1, big).astype(np.int64)
        for i in np.nonzero(claim >= 0)[0]:
            if last.mp_has_obs[i]:
                owner[claim[i]] = min(owner[claim[i]], i)
        nxt = np.full(last.n, -1, np.int32)
        for i, (idx, ur, radius) in win.items():
            if idx:
                d, b = best_free(p, i, idx, ur, radius, owner < i)
                if b >= 0 and _accept(d):
                    nxt[i] = b
        rounds += 1
        if first is None:
            first = nxt.copy()
        changed = not np.array_equal(nxt, claim)
        claim = nxt
        if not changed:
            break
    return claim, rounds, first


# ---- Tracking::TrackWithMotionModel (Tracking.cpp:724-774) ----------------------------------------------
def run_track_motion_model(p, only_tracking: bool):
    """The driver's replay for one frame: p.th is the first threshold (15 or 7).  Returns the record of
    rsc_track_motion_result plus out and discarded (int32 [frame n])."""
    import oracle_lib as ol
    fr, last = p.frame, p.last
    q = types.SimpleNamespace(**vars(p))
    q.frame_occ = np.zeros(fr.n, np.uint8)                                                # :724
    q.check_ori = True                                                                    # :716
    T0 = np.asarray(p.Tcw_cur, f32).reshape(4, 4)
    rec = dict(ok=0, searches=1, nmatches_search=[-1, -1], mode=0, nmatches=0, nmatches_map=0, vo=0, n_good=0,
               Tcw=T0.ravel().copy())
    nmatches, out, mode = search_by_projection_last(q)                                    # :732
    rec["nmatches_search"][0], rec["mode"] = nmatches, mode
    if nmatches < 20:                                                                     # :735
        q.th = float(f32(f32(2.0) * f32(p.th)))                                           # :738
        nmatches, out, _ = search_by_projection_last(q)
        rec["searches"], rec["nmatches_search"][1] = 2, nmatches
    out = np.where(out >= 0, out, -1).astype(np.int32)
    disc = np.full(fr.n, -1, np.int32)
    rec["nmatches"] = nmatches
    if nmatches < 20:                                                                     # :741
        return dict(rec, out=out, discarded=disc)
    inv = (f32(1.0) / (synth.scale_factors() * synth.scale_factors())).astype(f32)
    has = out >= 0
    Xw = np.zeros((fr.n, 3), f32)
    Xw[has] = np.asarray(last.mp_pos, f32).reshape(-1, 3)[out[has]]
    frame = types.SimpleNamespace(n=fr.n, has_mp=has.astype(np.uint8), uv=fr.kp, Xw=Xw, inv_sigma2=inv[fr.octave],
                                  fx=fr.fx, fy=fr.fy, cx=fr.cx, cy=fr.cy, Tcw=T0, u_right=fr.u_right, bf=fr.mbf)
    n_good, T, outl, _ = ol.pose_optimization(frame)                                      # :745
    n_map = 0
    for f in range(fr.n):                                                                 # :749-766
        if out[f] < 0:
            continue
        if outl[f] == 1:
            disc[f] = out[f]
            out[f] = -1
            nmatches -= 1
        elif last.mp_has_obs[out[f]]:
            n_map += 1
    rec.update(nmatches=nmatches, nmatches_map=n_map, n_good=int(n_good), Tcw=np.asarray(T, f32).ravel())
    if only_tracking:                                                                     # :768-772
        rec["vo"] = int(n_map < 10)
        rec["ok"] = int(nmatches > 20)
    else:
        rec["ok"] = int(n_map >= 10)                                                      # :774
    return dict(rec, out=out, discarded=disc)
