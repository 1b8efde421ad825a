"""Sequential numpy-float32 restatement of the relocalization matcher, the reference the device
kernel is compared with bit for bit (TEST-ONLY):

* ``search_by_projection``: ORBmatcher::SearchByProjection(Frame&, KeyFrame, sAlreadyFound, th, ORBdist)
  (src/ORBmatcher.cpp:1317-1444) with Frame::GetFeaturesInArea (src/Frame.cpp:394-447), MapPoint by
  MapPoint in slot order; MapPoint::PredictScale and ORBmatcher::ComputeThreeMaxima are the oracle's.
* ``reloc_refine_ref``: the refinement chain of Tracking::Relocalization (src/Tracking.cpp:1294-1323)
  over the oracle's PoseOptimization.

Float conventions are those of oracle/sim3match_oracle.h: every operation rounds to float32, matrix
rows are summed left to right, `1.0/z` is a double division rounded to float.
"""
from __future__ import annotations

import math
import types

import numpy as np

import oracle_lib as ol
from rsc import synth

f32 = np.float32
GRID_COLS, GRID_ROWS = 64, 48
HISTO_LENGTH = 30
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _round(x) -> int:
    """C round(): halves away from zero."""
    x = float(x)
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def features_in_area(F, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea (Frame.cpp:394-447): indices in (ix, iy, cell order) order."""
    gw, gh = f32(synth.GRID_W_INV), f32(synth.GRID_H_INV)
    mnx, mny = f32(F.min_x), f32(F.min_y)
    x0 = max(0, int(np.floor((x - mnx - r) * gw)))                 # :399
    if x0 >= GRID_COLS:
        return np.zeros(0, np.int64)
    x1 = min(GRID_COLS - 1, int(np.ceil((x - mnx + r) * gw)))      # :403
    if x1 < 0:
        return np.zeros(0, np.int64)
    y0 = max(0, int(np.floor((y - mny - r) * gh)))                 # :407
    if y0 >= GRID_ROWS:
        return np.zeros(0, np.int64)
    y1 = min(GRID_ROWS - 1, int(np.ceil((y - mny + r) * gh)))      # :411
    if y1 < 0:
        return np.zeros(0, np.int64)
    cells = []
    for ix in range(x0, x1 + 1):                                   # :417-421
        for iy in range(y0, y1 + 1):
            c = ix * GRID_ROWS + iy
            cells.append(F.cell_feat[F.cell_begin[c]:F.cell_begin[c + 1]])
    idx = np.concatenate(cells).astype(np.int64) if cells else np.zeros(0, np.int64)
    if idx.size == 0:
        return idx
    octv = F.octave[idx]
    ok = (octv >= min_level) & (octv <= max_level)                 # :428-435 (bCheckLevels, maxLevel >= 0)
    dx = F.kp[idx, 0] - x                                          # :437-441, float32
    dy = F.kp[idx, 1] - y
    ok &= (np.abs(dx) < r) & (np.abs(dy) < r)
    return idx[ok]


def project(F, kf, Tcw, i, th):
    """:1341-1371 for MapPoint slot i: (u, v, radius, level) or None when the point is skipped."""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    Xw = np.asarray(kf.mp_pos[i], f32)
    xc = [f32(f32(f32(f32(R[r, 0] * Xw[0]) + f32(R[r, 1] * Xw[1])) + f32(R[r, 2] * Xw[2])) + t[r])
          for r in range(3)]                                       # :1343
    Ow = [f32(-f32(f32(f32(R[0, r] * t[0]) + f32(R[1, r] * t[1])) + f32(R[2, r] * t[2])))
          for r in range(3)]                                       # :1323
    invzc = f32(1.0 / float(xc[2]))                                # :1347
    u = f32(f32(f32(f32(F.fx) * xc[0]) * invzc) + f32(F.cx))       # :1349
    v = f32(f32(f32(f32(F.fy) * xc[1]) * invzc) + f32(F.cy))       # :1350
    if u < f32(F.min_x) or u > f32(F.max_x):                       # :1352
        return None
    if v < f32(F.min_y) or v > f32(F.max_y):                       # :1354
        return None
    po = [f32(Xw[k] - Ow[k]) for k in range(3)]                    # :1358
    dist3D = f32(np.sqrt(f32(f32(f32(po[0] * po[0]) + f32(po[1] * po[1])) + f32(po[2] * po[2]))))
    max_d = f32(f32(1.2) * f32(kf.mp_dmax[i]))                     # :1361 GetMaxDistanceInvariance
    min_d = f32(f32(0.8) * f32(kf.mp_dmin[i]))
    if dist3D < min_d or dist3D > max_d:                           # :1365
        return None
    sf = synth.scale_factors()
    level = ol.lib().ora_predict_scale(float(kf.mp_dmax[i]), float(dist3D), float(synth.LOG_SCALE_FACTOR),
                                       len(sf))                    # :1368
    return u, v, f32(f32(th) * sf[level]), level                   # :1371


def search_by_projection(F, kf, Tcw, already, frame_mp, th, orb_dist, check_orientation=True, trace=None):
    """Returns (nmatches, out int32[F.n]): out[f] = KeyFrame slot of the new match on Frame feature f
    that survives the rotation check, else -1.  frame_mp / already are not modified.  With a dict in
    `trace`, trace['claim'][i] = feature taken by slot i before the rotation check and
    trace['free_best'][i] = the feature it would take if no MapPoint of this call claimed anything."""
    occupied = np.asarray(frame_mp) >= 0                           # CurrentFrame.mvpMapPoints[i2] set
    taken = occupied.copy()
    out = np.full(F.n, -1, np.int32)
    claim = np.full(kf.n, -1, np.int32)
    free_best = np.full(kf.n, -1, np.int32)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]                   # :1326
    nmatches = 0
    for i in range(kf.n):                                          # :1333
        if kf.mp_state[i] != 1 or already[i]:                      # :1337-1339
            continue
        pr = project(F, kf, Tcw, i, th)
        if pr is None:
            continue
        u, v, radius, level = pr
        idx = features_in_area(F, u, v, radius, level - 1, level + 1)  # :1373
        if idx.size == 0:                                          # :1375
            continue
        d = _POP[np.bitwise_xor(F.desc[idx], kf.mp_desc[i][None, :])].sum(1)
        for which, blocked in ((0, occupied), (1, taken)):
            dd = d[~blocked[idx]]                                  # :1386-1387
            ii = idx[~blocked[idx]]
            best = -1
            if dd.size and dd.min() < 256:                         # :1380, :1393 strict <: first minimum
                k = int(np.argmin(dd))
                if dd[k] <= orb_dist:                              # :1400
                    best = int(ii[k])
            if which == 0:
                free_best[i] = best
        if best < 0:
            continue
        taken[best] = True                                         # :1402
        out[best] = i
        claim[i] = best
        nmatches += 1
        if check_orientation:                                      # :1405-1415
            rot = f32(f32(kf.angle[i]) - f32(F.angle[best]))
            if rot < 0.0:
                rot = f32(rot + f32(360.0))
            b = _round(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH))))
            if b == HISTO_LENGTH:
                b = 0
            assert 0 <= b < HISTO_LENGTH
            rot_hist[b].append(best)
    if check_orientation:                                          # :1422-1441
        keep = ol.compute_three_maxima([len(h) for h in rot_hist])
        for b in range(HISTO_LENGTH):
            if b not in keep:
                for f in rot_hist[b]:
                    out[f] = -1
                    nmatches -= 1
    if trace is not None:
        trace["claim"], trace["free_best"] = claim, free_best
    return nmatches, out


def n_eligible(kf, already) -> int:
    return int(((np.asarray(kf.mp_state) == 1) & (np.asarray(already) == 0)).sum())


# ---- Tracking::Relocalization's refinement chain (Tracking.cpp:1294-1323) ----------------------------
def _poseopt(F, kf, fr, frame_mp, Tcw):
    """Optimizer::PoseOptimization(&mCurrentFrame) on the slots that hold a MapPoint."""
    inv = (f32(1.0) / (synth.scale_factors() * synth.scale_factors())).astype(f32)
    has = frame_mp >= 0
    Xw = np.zeros((F.n, 3), f32)
    Xw[has] = kf.mp_pos[frame_mp[has]]
    frame = types.SimpleNamespace(n=F.n, has_mp=has.astype(np.uint8), uv=F.kp, Xw=Xw, inv_sigma2=inv[F.octave],
                                  fx=F.fx, fy=F.fy, cx=F.cx, cy=F.cy, Tcw=np.asarray(Tcw, f32).reshape(4, 4),
                                  u_right=fr.get("u_right"), bf=fr.get("bf", 0.0))
    n_good, T, outl, _ = ol.pose_optimization(frame)
    return n_good, T, (outl == 1) & has


def reloc_refine_ref(F, kf, fr, frame_mp, found, n_good_in, Tcw_in):
    """Tracking.cpp:1294-1323 for one candidate.  frame_mp: KeyFrame slot per Frame slot after
    :1289-1291; found: sFound over the KeyFrame slots (:1278).  Returns a dict: n_good,
    n_additional[2] (-1: stage not run), pose_opts, Tcw, frame_mp (final)."""
    mp = np.array(frame_mp, np.int32)
    found = np.array(found, np.uint8)
    n_good = int(n_good_in)
    T = np.asarray(Tcw_in, f32).reshape(4, 4).copy()
    n_add = [-1, -1]
    pose_opts = 0
    if n_good < 50:                                                # :1294
        nadd, out = search_by_projection(F, kf, T, found, mp, 10, 100)  # :1296
        mp[out >= 0] = out[out >= 0]
        n_add[0] = nadd
        if nadd + n_good >= 50:                                    # :1298
            n_good, T, _ = _poseopt(F, kf, fr, mp, T)              # :1300 (outliers stay in mvpMapPoints)
            pose_opts = 1
            if 30 < n_good < 50:                                   # :1304
                found = np.zeros(kf.n, np.uint8)                   # :1306-1309
                found[mp[mp >= 0]] = 1
                nadd, out = search_by_projection(F, kf, T, found, mp, 3, 64)  # :1310
                mp[out >= 0] = out[out >= 0]
                n_add[1] = nadd
                if n_good + nadd >= 50:                            # :1313
                    n_good, T, outl = _poseopt(F, kf, fr, mp, T)   # :1315
                    pose_opts = 2
                    mp[outl] = -1                                  # :1317-1319
    return dict(n_good=n_good, n_additional=n_add, pose_opts=pose_opts, Tcw=T, frame_mp=mp)


# ---- Tracking::Relocalization from the candidate solvers to bMatch (Tracking.cpp:1239-1335) ----------
def run_reloc_refined(F, cands, seeds, u_right, bf, params=None):
    """The round-robin of events_oracle.run_reloc_gated with the refinement chain inside: cands =
    [(kf, matches int32 [F.n] = vvpMapPointMatches as KeyFrame slots, PnPScene)].  Returns the record of
    rsc_reloc_refined_result plus frame_mp (final mvpMapPoints as KeyFrame slots of the winner) and
    `trace`, one entry per success: (round, candidate, first nGood, chain record or None)."""
    import events_oracle as eo
    from rsc import events as rev
    params = rev.RELOC_PARAMS if params is None else params
    solvers = [ol.OraclePnP(sc, int(s)) for (_, _, sc), s in zip(cands, seeds)]
    for o in solvers:
        o.set_ransac_parameters(*params)
    rec = dict(status=eo.GATE_NONE, winner=-1, round=-1, hypothesis=-1, n_inliers=0, n_good=0, rejected=0, gates=0,
               n_good_first=0, n_additional=[-1, -1], chains=0, Tcw=np.zeros(16, f32), frame_mp=None, trace=[])
    fr = dict(u_right=u_right, bf=bf)
    active = list(range(len(solvers)))
    rnd = 0
    while active:                                                  # :1239
        nxt = []
        for i in active:                                           # :1241
            kf, matches, sc = cands[i]
            r = solvers[i].iterate(5)                              # :1255
            if not r["no_more"]:                                   # :1258-1262
                nxt.append(i)
            if not r["ok"]:
                continue
            inl = np.asarray(r["inliers"], bool)
            f = eo._frame_for(sc, inl, r["T"], u_right, bf)
            n_good, T, outl, _ = ol.pose_optimization(f)           # :1284
            rec["gates"] += 1
            if n_good < 10:                                        # :1286
                rec["rejected"] += 1
                rec["trace"].append((rnd, i, n_good, None))
                continue
            mp = np.where(inl & (np.where(f.has_mp == 1, outl, 0) != 1), matches, -1).astype(np.int32)  # :1289-1291
            found = np.zeros(kf.n, np.uint8)                       # :1278
            found[matches[inl]] = 1
            first, chain, add = n_good, None, [-1, -1]
            if n_good < 50:                                        # :1294
                chain = reloc_refine_ref(F, kf, fr, mp, found, n_good, T)
                rec["chains"] += 1
                n_good, T, mp, add = chain["n_good"], chain["Tcw"], chain["frame_mp"], chain["n_additional"]
            rec["trace"].append((rnd, i, first, chain))
            if n_good < 50:                                        # :1327
                rec["rejected"] += 1
                continue
            rec.update(status=eo.GATE_MATCH, winner=i, round=rnd, hypothesis=r["iterations"] - 1,
                       n_inliers=r["n_inliers"], n_good=n_good, n_good_first=first, n_additional=list(add),
                       Tcw=np.asarray(T, f32).ravel(), frame_mp=mp)
            return rec
        active = nxt
        rnd += 1
    return rec
