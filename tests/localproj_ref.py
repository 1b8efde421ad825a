"""Sequential restatement of Tracking::SearchLocalPoints (src/Tracking.cpp:1003-1028), the reference the
device kernels are compared with bit for bit (TEST-ONLY), written from the reference text and independent of
csrc/rsc_localproj.h:

* ``is_in_frustum``: Frame::isInFrustum (src/Frame.cpp:336-392), numpy float32 step by step;
* ``features_in_area``: Frame::GetFeaturesInArea (src/Frame.cpp:394-447) with minLevel / maxLevel;
* ``radius_by_viewing_cos``: ORBmatcher::RadiusByViewingCos (src/ORBmatcher.cpp:102-108);
* ``search_by_projection``: ORBmatcher::SearchByProjection(Frame&, vector<MapPoint>&, th) (:16-100), point by
  point in list order on an explicit ``F.mvpMapPoints``;
* ``search_local_points``: the two together (Tracking.cpp:1003-1028);
* ``fixed_point_rounds``: the rounds of the device mapping restated on the same functions (round count).

Every operation rounds to its type, fixed-size sums run left to right; MapPoint::PredictScale is the oracle's.
"""
from __future__ import annotations

import numpy as np

import oracle_lib as ol
from rsc import synth

f32 = np.float32
GRID_COLS, GRID_ROWS = 64, 48
TH_HIGH = 100
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)

# what isInFrustum leaves in the MapPoint (rsc_track_record, include/rsc.h)
TRACK = np.dtype([("in_view", np.int32), ("proj_x", f32), ("proj_y", f32), ("proj_xr", f32), ("level", np.int32),
                  ("view_cos", f32)])


def is_in_frustum(fr, pts, Tcw, i, cos_limit):
    """Frame.cpp:336-392 for point i: None (mbTrackInView = false) or (u, v, xr, level, viewCos)."""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    with np.errstate(all="ignore"):
        P = np.asarray(pts.pos[i], f32)                                                   # :341
        Pc = [f32(f32(f32(f32(T[r, 0] * P[0]) + f32(T[r, 1] * P[1])) + f32(T[r, 2] * P[2])) + T[r, 3])
              for r in range(3)]                                                          # :344
        Ow = [f32(-f32(f32(f32(T[0, r] * T[0, 3]) + f32(T[1, r] * T[1, 3])) + f32(T[2, r] * T[2, 3])))
              for r in range(3)]                                                          # mOw = -Rcw^T tcw
        if Pc[2] < f32(0.0):                                                              # :350
            return None
        invz = f32(f32(1.0) / Pc[2])                                                      # :354 float division
        u = f32(f32(f32(f32(fr.fx) * Pc[0]) * invz) + f32(fr.cx))                         # :355
        v = f32(f32(f32(f32(fr.fy) * Pc[1]) * invz) + f32(fr.cy))
        if np.isnan(u) or np.isnan(v):   # outside the reference's defined behaviour (NaN reaches floor): skipped
            return None
        if u < f32(fr.min_x) or u > f32(fr.max_x):                                        # :358
            return None
        if v < f32(fr.min_y) or v > f32(fr.max_y):                                        # :360
            return None
        max_d = f32(f32(1.2) * f32(pts.dmax[i]))                                          # :364
        min_d = f32(f32(0.8) * f32(pts.dmin[i]))                                          # :365
        PO = [f32(P[k] - Ow[k]) for k in range(3)]                                        # :366
        dist = f32(np.sqrt(f32(f32(f32(PO[0] * PO[0]) + f32(PO[1] * PO[1])) + f32(PO[2] * PO[2]))))  # :367
        if dist < min_d or dist > max_d:                                                  # :369
            return None
        Pn = np.asarray(pts.normal[i], f32)                                               # :373
        dot = f32(f32(f32(PO[0] * Pn[0]) + f32(PO[1] * Pn[1])) + f32(PO[2] * Pn[2]))
        view_cos = f32(dot / dist)                                                        # :375
        if view_cos < f32(cos_limit):                                                     # :377
            return None
        level = ol.lib().ora_predict_scale(float(pts.dmax[i]), float(dist), float(synth.LOG_SCALE_FACTOR),
                                           len(synth.scale_factors()))                    # :381
        xr = f32(u - f32(f32(fr.mbf) * invz))                                             # :386
        return u, v, xr, int(level), view_cos


def radius_by_viewing_cos(view_cos) -> float:
    """ORBmatcher.cpp:102-108: the float is compared with the double literal 0.998."""
    return 2.5 if float(f32(view_cos)) > 0.998 else 4.0


def features_in_area(fr, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea (Frame.cpp:394-447): indices in (ix, iy, cell order) order."""
    assert np.isfinite(x) and np.isfinite(y), "NaN / inf reached the cell arithmetic"
    gw, gh = f32(synth.GRID_W_INV), f32(synth.GRID_H_INV)
    mnx, mny = f32(fr.min_x), f32(fr.min_y)
    x0 = max(0, int(np.floor(f32(f32(f32(x - mnx) - r) * gw))))                           # :399
    if x0 >= GRID_COLS:
        return []
    x1 = min(GRID_COLS - 1, int(np.ceil(f32(f32(f32(x - mnx) + r) * gw))))                # :403
    if x1 < 0:
        return []
    y0 = max(0, int(np.floor(f32(f32(f32(y - mny) - r) * gh))))                           # :407
    if y0 >= GRID_ROWS:
        return []
    y1 = min(GRID_ROWS - 1, int(np.ceil(f32(f32(f32(y - mny) + r) * gh))))                # :411
    if y1 < 0:
        return []
    check = min_level > 0 or max_level >= 0                                               # :415
    out = []
    for ix in range(x0, x1 + 1):                                                          # :417
        for iy in range(y0, y1 + 1):
            c = ix * GRID_ROWS + iy
            for f in fr.cell_feat[fr.cell_begin[c]:fr.cell_begin[c + 1]]:
                f = int(f)
                if check:                                                                 # :428-435
                    o = int(fr.octave[f])
                    if o < min_level:
                        continue
                    if max_level >= 0 and o > max_level:
                        continue
                dx = f32(fr.kp[f, 0] - x)                                                 # :437
                dy = f32(fr.kp[f, 1] - y)
                if abs(dx) < r and abs(dy) < r:                                           # :440
                    out.append(f)
    return out


def _window(fr, tr, i, th):
    """ORBmatcher.cpp:31-40 for point i: (indices, radius)."""
    level = int(tr["level"][i])
    r = f32(radius_by_viewing_cos(tr["view_cos"][i]))                                     # :34
    if float(f32(th)) != 1.0:                                                             # :20, :36
        r = f32(r * f32(th))
    rad = f32(r * synth.scale_factors()[level])                                           # :40
    return features_in_area(fr, tr["proj_x"][i], tr["proj_y"][i], rad, level - 1, level), rad


def _decide(fr, pts, tr, i, idx, rad, blocked, nn_ratio, stat=None):
    """:47-92 for point i over the window `idx`: (bestIdx or -1, dict of what happened).  blocked[f]: the
    occupant of F.mvpMapPoints[f] has Observations() > 0."""
    best_dist, best_level, best_dist2, best_level2, best_idx = 256, -1, 256, -1, -1
    stereo = 0
    for f in idx:
        if blocked[f]:                                                                    # :58-60
            continue
        if fr.u_right[f] > 0:                                                             # :62
            er = f32(abs(f32(tr["proj_xr"][i] - fr.u_right[f])))                          # :64
            if er > rad:                                                                  # :65
                stereo += 1
                continue
        d = int(_POP[np.bitwise_xor(fr.desc[f], pts.desc[i])].sum())                      # :71
        if d < best_dist:                                                                 # :73
            best_dist2, best_dist = best_dist, d
            best_level2, best_level = best_level, int(fr.octave[f])
            best_idx = f
        elif d < best_dist2:                                                              # :81
            best_level2, best_dist2 = int(fr.octave[f]), d
    info = dict(best=best_idx, best_dist=best_dist, veto=False, stereo=stereo)
    if best_dist <= TH_HIGH:                                                              # :89
        if best_level == best_level2 and f32(best_dist) > f32(f32(nn_ratio) * f32(best_dist2)):  # :91
            info["veto"] = True
            return -1, info
        return best_idx, info
    return -1, info


def _searched(pts, skip, tr, i) -> bool:
    """:25-29 (and the caller's skip list, whose points have mbTrackInView false)."""
    return bool(tr["in_view"][i]) and pts.state[i] == 1 and not skip[i]


def search_by_projection(fr, pts, track, skip, has_obs, frame_occ, th, nn_ratio, trace=None):
    """ORBmatcher.cpp:16-100.  track: TRACK records (the MapPoints' mbTrackInView ... members).  Returns
    (nmatches, out int32[fr.n]): out[f] = index into pts of the MapPoint the call leaves in F.mvpMapPoints[f],
    else -1.  Inputs are not modified.  With a dict in `trace`, counters of the branches taken:
    matches; vetoes (:91 fired); stereo (candidates skipped at :65); overwrites (a match written over an
    earlier point of this call, which had no observations); promoted (an accepted point whose best candidate
    on entry was held by an earlier point of the call); lifted (a point the ratio test would have vetoed on
    entry, accepted on the same feature because an earlier point took the runner-up); claim[i]."""
    tr = np.asarray(track, TRACK)
    entry_blocked = np.asarray(frame_occ) == 2
    blocked = entry_blocked.copy()
    holder = np.full(fr.n, -1, np.int32)       # the point of this call in F.mvpMapPoints[f]
    claim = np.full(pts.n, -1, np.int32)
    cnt = dict(matches=0, vetoes=0, stereo=0, overwrites=0, promoted=0, lifted=0, searched=0)
    nmatches = 0
    for i in range(pts.n):                                                                # :22
        if not _searched(pts, skip, tr, i):                                               # :25-29
            continue
        cnt["searched"] += 1
        idx, rad = _window(fr, tr, i, th)
        if not idx:                                                                       # :42
            continue
        b, info = _decide(fr, pts, tr, i, idx, rad, blocked, nn_ratio)
        cnt["stereo"] += info["stereo"]
        cnt["vetoes"] += info["veto"]
        if b < 0:
            continue
        if trace is not None:
            b0, info0 = _decide(fr, pts, tr, i, idx, rad, entry_blocked, nn_ratio)
            if info0["best"] >= 0 and blocked[info0["best"]] and not entry_blocked[info0["best"]]:
                cnt["promoted"] += 1
            if info0["veto"] and info0["best"] == b:
                cnt["lifted"] += 1
        if holder[b] >= 0:
            cnt["overwrites"] += 1
        holder[b] = i                                                                     # :94
        blocked[b] = bool(has_obs[i])           # the new occupant's Observations() > 0
        claim[i] = b
        nmatches += 1                                                                     # :95
    cnt["matches"] = nmatches
    if trace is not None:
        trace.update(cnt)
        trace["claim"] = claim
    return nmatches, holder


def frustum_all(fr, pts, Tcw, skip, cos_limit):
    """Tracking.cpp:1003-1016: (track records, nToMatch).  A point that is skipped, bad or outside has
    in_view = 0 and zeros."""
    tr = np.zeros(pts.n, TRACK)
    n_to_match = 0
    for i in range(pts.n):
        if skip[i] or pts.state[i] != 1:                                                  # :1006-1009
            continue
        r = is_in_frustum(fr, pts, Tcw, i, cos_limit)                                     # :1011
        if r is None:
            continue
        tr[i] = (1, r[0], r[1], r[2], r[3], r[4])
        n_to_match += 1                                                                   # :1014
    return tr, n_to_match


def search_local_points(fr, pts, Tcw, skip, has_obs, frame_occ, cos_limit, th, nn_ratio, trace=None):
    """Tracking.cpp:1003-1028.  Returns dict(out, track, nmatches, n_to_match)."""
    tr, n_to_match = frustum_all(fr, pts, Tcw, skip, cos_limit)
    n, out = (0, np.full(fr.n, -1, np.int32))
    if n_to_match > 0:                                                                    # :1018
        n, out = search_by_projection(fr, pts, tr, skip, has_obs, frame_occ, th, nn_ratio, trace)
    return dict(out=out, track=tr, nmatches=n, n_to_match=n_to_match)


def fixed_point_rounds(fr, pts, track, skip, has_obs, frame_occ, th, nn_ratio):
    """The rounds of the device mapping restated on the functions above: every round rebuilds
    blocked[f] for point i = (an entry occupant with observations, or a point j < i with observations claims f)
    from the claims of the round before and lets every point decide again, until a round changes no claim.
    Returns (claim int32[pts.n], rounds, claim after round 1)."""
    tr = np.asarray(track, TRACK)
    entry_blocked = np.asarray(frame_occ) == 2
    win = {}
    for i in range(pts.n):
        if not _searched(pts, skip, tr, i) or np.isnan(tr["proj_x"][i]) or np.isnan(tr["proj_y"][i]):
            continue
        idx, rad = _window(fr, tr, i, th)
        x, y = tr["proj_x"][i], tr["proj_y"][i]
        # the kernel's bound counts the points whose cell range is not empty, not those with a feature in it
        gw, gh = f32(synth.GRID_W_INV), f32(synth.GRID_H_INV)
        x0 = max(0, int(np.floor(f32(f32(f32(x - f32(fr.min_x)) - rad) * gw))))
        x1 = min(GRID_COLS - 1, int(np.ceil(f32(f32(f32(x - f32(fr.min_x)) + rad) * gw))))
        y0 = max(0, int(np.floor(f32(f32(f32(y - f32(fr.min_y)) - rad) * gh))))
        y1 = min(GRID_ROWS - 1, int(np.ceil(f32(f32(f32(y - f32(fr.min_y)) + rad) * gh))))
        if x0 >= GRID_COLS or x1 < 0 or y0 >= GRID_ROWS or y1 < 0:
            continue
        win[i] = (idx, rad)
    claim = np.full(pts.n, -1, np.int32)
    first = None
    rounds = 0
    big = np.iinfo(np.int32).max
    for _ in range(len(win) + 1):
        owner = np.where(entry_blocked, -1, big).astype(np.int64)
        for i in np.nonzero(claim >= 0)[0]:
            if has_obs[i]:
                owner[claim[i]] = min(owner[claim[i]], i)
        nxt = np.full(pts.n, -1, np.int32)
        for i, (idx, rad) in win.items():
            if idx:
                nxt[i] = _decide(fr, pts, tr, i, idx, rad, owner < i, nn_ratio)[0]
        rounds += 1
        if first is None:
            first = nxt.copy()
        changed = not np.array_equal(nxt, claim)
        claim = nxt
        if not changed:
            break
    return claim, rounds, first


def out_of_claims(n_features, claim):
    out = np.full(n_features, -1, np.int32)
    for i in np.nonzero(np.asarray(claim) >= 0)[0]:
        out[claim[i]] = i
    return out
