"""Sequential restatements of the loop-closing projection stage, the references the device kernels and the
host composition are compared with bit for bit (TEST-ONLY):

* ``search_by_projection_kf``: ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
  (src/ORBmatcher.cpp:241-352), numpy float32, point by point in list order;
* ``fuse``: ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cpp:823-946);
* ``features_in_area``: KeyFrame::GetFeaturesInArea (src/KeyFrame.cpp:560-599), ``is_in_image``: :601-604;
* ``compose``: gSmw, mg2oScw = gScm * gSmw, mScw = toIso(mg2oScw) (src/LoopClosing.cpp:318-320), numpy
  float64, with g2o::Sim3::operator* (Thirdparty/g2o/g2o/types/sim3.h:266-272), Eigen 3.3's
  Quaterniond(Matrix3d), generic quaternion product, _transformVector and toRotationMatrix;
* ``loop_verify``: LoopClosing.cpp:318-320 and :360-370 on the gate's result.

Float conventions are those of oracle/sim3match_oracle.h: every operation rounds to its type, fixed-size
sums run left to right; MapPoint::PredictScale is the oracle's.
"""
from __future__ import annotations

import types

import numpy as np

import oracle_lib as ol
from rsc import synth

f32 = np.float32
f64 = np.float64
GRID_COLS, GRID_ROWS = 64, 48
TH_LOW = 50
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def is_in_image(kf, u, v) -> bool:
    """KeyFrame::IsInImage (KeyFrame.cpp:601-604): the maximum is excluded; false for inf / NaN."""
    return bool(u >= f32(kf.min_x) and u < f32(kf.max_x) and v >= f32(kf.min_y) and v < f32(kf.max_y))


def features_in_area(kf, x, y, r):
    """KeyFrame::GetFeaturesInArea (KeyFrame.cpp:560-599): indices in (ix, iy, cell order) order."""
    assert np.isfinite(x) and np.isfinite(y), "NaN / inf reached the cell arithmetic"
    gw, gh = f32(synth.GRID_W_INV), f32(synth.GRID_H_INV)
    mnx, mny = f32(kf.min_x), f32(kf.min_y)
    x0 = max(0, int(np.floor((x - mnx - r) * gw)))                 # :565
    if x0 >= GRID_COLS:
        return np.zeros(0, np.int64)
    x1 = min(GRID_COLS - 1, int(np.ceil((x - mnx + r) * gw)))      # :569
    if x1 < 0:
        return np.zeros(0, np.int64)
    y0 = max(0, int(np.floor((y - mny - r) * gh)))                 # :573
    if y0 >= GRID_ROWS:
        return np.zeros(0, np.int64)
    y1 = min(GRID_ROWS - 1, int(np.ceil((y - mny + r) * gh)))      # :577
    if y1 < 0:
        return np.zeros(0, np.int64)
    cells = []
    for ix in range(x0, x1 + 1):                                   # :581-585
        for iy in range(y0, y1 + 1):
            c = ix * GRID_ROWS + iy
            cells.append(kf.cell_feat[kf.cell_begin[c]:kf.cell_begin[c + 1]])
    idx = np.concatenate(cells).astype(np.int64) if cells else np.zeros(0, np.int64)
    if idx.size == 0:
        return idx
    dx = kf.kp[idx, 0] - x                                         # :589-593, float32
    dy = kf.kp[idx, 1] - y
    return idx[(np.abs(dx) < r) & (np.abs(dy) < r)]


def decompose(Scw, fuse: bool):
    """:250-252 (Scw as it is) or :832-836 (divided by scw).  Returns (Rcw, tcw, Ow)."""
    T = np.asarray(Scw, f32).reshape(4, 4)
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    if fuse:
        scw = f32(np.sqrt(f32(f32(f32(R[0, 0] * R[0, 0]) + f32(R[0, 1] * R[0, 1])) + f32(R[0, 2] * R[0, 2]))))  # :833
        R = (R / scw).astype(f32)                                  # :834
        t = (t / scw).astype(f32)                                  # :835
    Ow = [f32(-f32(f32(f32(R[0, r] * t[0]) + f32(R[1, r] * t[1])) + f32(R[2, r] * t[2]))) for r in range(3)]
    return R, t, Ow


def project(kf, pts, R, t, Ow, i, th, fuse: bool, info=None):
    """:270-309 / :855-895 for point i: (u, v, radius, level) or None when the point is skipped.  With a dict
    in `info`, info['u'], info['v'] = the projection when it was computed."""
    with np.errstate(all="ignore"):
        Xw = np.asarray(pts.pos[i], f32)
        xc = [f32(f32(f32(f32(R[r, 0] * Xw[0]) + f32(R[r, 1] * Xw[1])) + f32(R[r, 2] * Xw[2])) + t[r])
              for r in range(3)]                                   # :273
        if xc[2] < 0.0:                                            # :276 / :861
            return None
        invz = f32(1.0 / float(xc[2])) if fuse else f32(f32(1.0) / xc[2])  # :865 double / :280 float division
        x = f32(xc[0] * invz)                                      # :281
        y = f32(xc[1] * invz)
        u = f32(f32(f32(kf.fx) * x) + f32(kf.cx))                  # :284
        v = f32(f32(f32(kf.fy) * y) + f32(kf.cy))
        if info is not None:
            info["u"], info["v"] = u, v
        if not is_in_image(kf, u, v):                              # :288
            return None
        po = [f32(Xw[k] - Ow[k]) for k in range(3)]                # :294
        dist = f32(np.sqrt(f32(f32(f32(po[0] * po[0]) + f32(po[1] * po[1])) + f32(po[2] * po[2]))))
        max_d = f32(f32(1.2) * f32(pts.dmax[i]))                   # :292 GetMaxDistanceInvariance
        min_d = f32(f32(0.8) * f32(pts.dmin[i]))
        if dist < min_d or dist > max_d:                           # :297
            return None
        Pn = np.asarray(pts.normal[i], f32)                        # :301
        dot = f32(f32(f32(po[0] * Pn[0]) + f32(po[1] * Pn[1])) + f32(po[2] * Pn[2]))
        if float(dot) < 0.5 * float(dist):                         # :303, compared in double
            return None
        sf = synth.scale_factors()
        level = ol.lib().ora_predict_scale(float(pts.dmax[i]), float(dist), float(synth.LOG_SCALE_FACTOR),
                                           len(sf))                # :306
        return u, v, f32(f32(th) * sf[level]), level               # :309


def _best(kf, pts, i, idx, level, blocked):
    """:319-343 / :906-928: first minimum over the keypoints of levels [L-1, L] that are not blocked."""
    best_dist, best_idx = 256, -1
    for f in idx:
        f = int(f)
        if blocked is not None and blocked[f]:                     # :324
            continue
        o = int(kf.octave[f])
        if o < level - 1 or o > level:                             # :329
            continue
        d = int(_POP[np.bitwise_xor(kf.desc[f], pts.desc[i])].sum())
        if d < best_dist:                                          # :336
            best_dist, best_idx = d, f
    return best_idx if best_dist <= TH_LOW else -1                 # :343


def search_by_projection_kf(kf, pts, Scw, already, occupied, th, trace=None):
    """Returns (nmatches, out int32[kf.n]): out[idx] = index into pts of the MapPoint written to
    vpMatched[idx], else -1.  Inputs are not modified.  With a dict in `trace`: trace['claim'][i] = the
    keypoint point i took, trace['free_best'][i] = the keypoint it would take if no point of this call
    claimed anything (its round-1 choice), trace['windows'] = points that reached the keypoint loop."""
    R, t, Ow = decompose(Scw, False)
    occupied = np.asarray(occupied).astype(bool)
    taken = occupied.copy()
    out = np.full(kf.n, -1, np.int32)
    claim = np.full(pts.n, -1, np.int32)
    free_best = np.full(pts.n, -1, np.int32)
    nmatches = windows = 0
    for i in range(pts.n):                                         # :261
        if pts.state[i] != 1 or already[i]:                        # :266
            continue
        pr = project(kf, pts, R, t, Ow, i, th, False)
        if pr is None:
            continue
        u, v, radius, level = pr
        idx = features_in_area(kf, u, v, radius)                   # :311
        if idx.size == 0:                                          # :313
            continue
        windows += 1
        free_best[i] = _best(kf, pts, i, idx, level, occupied)
        best = _best(kf, pts, i, idx, level, taken)
        if best < 0:
            continue
        taken[best] = True                                         # :345
        out[best] = i
        claim[i] = best
        nmatches += 1
    if trace is not None:
        trace["claim"], trace["free_best"], trace["windows"] = claim, free_best, windows
    return nmatches, out


def fixed_point_rounds(kf, pts, Scw, already, occupied, th):
    """The rounds of the device mapping (rsc_kfproj.h) restated on the reference's functions: every round
    rebuilds owner[f] = the lowest point claiming f from the claims of the round before and lets every
    point take its best keypoint among those with owner >= itself, until a round changes no claim.
    Returns (claim int32[pts.n], rounds, exhausted): exhausted = points that, in some round, found their
    four best free-on-entry candidates (distance <= 50, visiting order) all taken although more qualified,
    which is where the kernel walks the window again."""
    R, t, Ow = decompose(Scw, False)
    occupied = np.asarray(occupied).astype(bool)
    win = {}
    for i in range(pts.n):
        if pts.state[i] != 1 or already[i]:
            continue
        pr = project(kf, pts, R, t, Ow, i, th, False)
        if pr is None:
            continue
        idx = features_in_area(kf, pr[0], pr[1], pr[2])
        level = pr[3]
        cand = []                                                  # (distance, keypoint) in visiting order
        for f in idx:
            f = int(f)
            o = int(kf.octave[f])
            if occupied[f] or o < level - 1 or o > level:
                continue
            d = int(_POP[np.bitwise_xor(kf.desc[f], pts.desc[i])].sum())
            if d <= TH_LOW:
                cand.append((d, f))
        order = sorted(range(len(cand)), key=lambda k: (cand[k][0], k))  # stable: ties in visiting order
        win[i] = [cand[k] for k in order]
    claim = np.full(pts.n, -1, np.int32)
    exhausted = set()
    rounds = 0
    big = np.iinfo(np.int32).max
    for _ in range(len(win) + 1):
        owner = np.full(kf.n, big, np.int64)
        for i in np.nonzero(claim >= 0)[0]:
            owner[claim[i]] = min(owner[claim[i]], i)
        nxt = np.full(pts.n, -1, np.int32)
        for i, cand in win.items():
            free = [k for k, (d, f) in enumerate(cand) if owner[f] >= i]
            if free:
                nxt[i] = cand[free[0]][1]
            if len(cand) > 4 and (not free or free[0] >= 4):
                exhausted.add(i)
        rounds += 1
        changed = not np.array_equal(nxt, claim)
        claim = nxt
        if not changed:
            break
    return claim, rounds, len(exhausted)


def fuse(kf, pts, Scw, in_kf, th):
    """Returns a dict: nfused, best_idx int32[pts.n] (bestIdx when bestDist <= 50, else -1), and the host part
    of :930-940 from the KeyFrame's own slots: replace[i] = the slot whose good MapPoint goes to
    vpReplacePoint[i] (else -1), added[i] = the slot point i is added to (else -1).  AddMapPoint fills the
    slot at once, so a later point with the same bestIdx finds the earlier one there: holder[i] = that earlier
    point of the list (else -1: the slot's MapPoint is the KeyFrame's own)."""
    R, t, Ow = decompose(Scw, True)
    best_idx = np.full(pts.n, -1, np.int32)
    replace = np.full(pts.n, -1, np.int32)
    added = np.full(pts.n, -1, np.int32)
    holder = np.full(pts.n, -1, np.int32)
    held = {}
    nfused = 0
    for i in range(pts.n):                                         # :846
        if pts.state[i] != 1 or in_kf[i]:                          # :851
            continue
        pr = project(kf, pts, R, t, Ow, i, th, True)
        if pr is None:
            continue
        u, v, radius, level = pr
        idx = features_in_area(kf, u, v, radius)                   # :897
        if idx.size == 0:
            continue
        b = _best(kf, pts, i, idx, level, None)                    # :906-925 (INT_MAX start, same cutoff)
        if b < 0:                                                  # :928
            continue
        best_idx[i] = b
        if b in held:                                              # :930-934: a point this call added (good)
            replace[i] = b
            holder[i] = held[b]
        elif kf.mp_state[b] != 0:                                  # :931
            if kf.mp_state[b] == 1:                                # :933
                replace[i] = b
        else:
            added[i] = b                                           # :938-939: GetMapPoint(b) is set from here on
            held[b] = i
        nfused += 1
    return dict(nfused=nfused, best_idx=best_idx, replace=replace, added=added, holder=holder)


def n_eligible(pts, already) -> int:
    return int(((np.asarray(pts.state) == 1) & (np.asarray(already) == 0)).sum())


# ---- LoopClosing.cpp:318-320 in float64 ----------------------------------------------------------------
def quat_from_R(m):
    """Eigen 3.3 Quaterniond(Matrix3d) (Geometry/Quaternion.h quaternionbase_assign_op_impl): (x, y, z, w)."""
    m = np.asarray(m, f64)
    tr = f64(f64(m[0, 0] + m[1, 1]) + m[2, 2])
    q = [f64(0)] * 4
    if tr > 0.0:
        t = f64(np.sqrt(f64(tr + 1.0)))
        q[3] = f64(0.5 * t)
        t = f64(0.5 / t)
        q[0] = f64(f64(m[2, 1] - m[1, 2]) * t)
        q[1] = f64(f64(m[0, 2] - m[2, 0]) * t)
        q[2] = f64(f64(m[1, 0] - m[0, 1]) * t)
        return q
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = f64(np.sqrt(f64(f64(f64(m[i, i] - m[j, j]) - m[k, k]) + 1.0)))
    q[i] = f64(0.5 * t)
    t = f64(0.5 / t)
    q[3] = f64(f64(m[k, j] - m[j, k]) * t)
    q[j] = f64(f64(m[j, i] + m[i, j]) * t)
    q[k] = f64(f64(m[k, i] + m[i, k]) * t)
    return q


def quat_mul(a, b):
    """Eigen's generic quat_product (x, y, z, w)."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    w = f64(f64(f64(f64(aw * bw) - f64(ax * bx)) - f64(ay * by)) - f64(az * bz))
    x = f64(f64(f64(f64(aw * bx) + f64(ax * bw)) + f64(ay * bz)) - f64(az * by))
    y = f64(f64(f64(f64(aw * by) + f64(ay * bw)) + f64(az * bx)) - f64(ax * bz))
    z = f64(f64(f64(f64(aw * bz) + f64(az * bw)) + f64(ax * by)) - f64(ay * bx))
    return [x, y, z, w]


def quat_rotate(q, v):
    """QuaternionBase::_transformVector: uv = 2 (q.vec x v); v + w uv + q.vec x uv."""
    x, y, z, w = q
    uv = [f64(f64(y * v[2]) - f64(z * v[1])), f64(f64(z * v[0]) - f64(x * v[2])), f64(f64(x * v[1]) - f64(y * v[0]))]
    uv = [f64(c + c) for c in uv]
    c = [f64(f64(y * uv[2]) - f64(z * uv[1])), f64(f64(z * uv[0]) - f64(x * uv[2])),
         f64(f64(x * uv[1]) - f64(y * uv[0]))]
    return [f64(f64(v[k] + f64(w * uv[k])) + c[k]) for k in range(3)]


def quat_to_R(q):
    """QuaternionBase::toRotationMatrix."""
    x, y, z, w = q
    tx, ty, tz = f64(2.0 * x), f64(2.0 * y), f64(2.0 * z)
    twx, twy, twz = f64(tx * w), f64(ty * w), f64(tz * w)
    txx, txy, txz = f64(tx * x), f64(ty * x), f64(tz * x)
    tyy, tyz, tzz = f64(ty * y), f64(tz * y), f64(tz * z)
    return np.array([[f64(1.0 - f64(tyy + tzz)), f64(txy - twz), f64(txz + twy)],
                     [f64(txy + twz), f64(1.0 - f64(txx + tzz)), f64(tyz - twx)],
                     [f64(txz - twy), f64(tyz + twx), f64(1.0 - f64(txx + tyy))]], f64)


def compose(S_cm, R_mw, t_mw):
    """S_cm float64[8] = gScm as q (x, y, z, w), t, s; R_mw float32 [3,3], t_mw float32 [3] = the matched
    KeyFrame's pose.  Returns (mg2oScw float64[8], mScw float32[16])."""
    S_cm = np.asarray(S_cm, f64)
    q2 = quat_from_R(np.asarray(R_mw, f32).astype(f64))            # :318 Sim3(R.cast<double>(), t.cast<double>(), 1.0)
    t2 = [f64(c) for c in np.asarray(t_mw, f32)]
    q1, t1, s1 = list(S_cm[:4]), list(S_cm[4:7]), f64(S_cm[7])
    r = quat_mul(q1, q2)                                           # sim3.h:268
    rt = quat_rotate(q1, t2)
    t = [f64(f64(s1 * rt[k]) + t1[k]) for k in range(3)]           # sim3.h:269
    s = f64(s1 * f64(1.0))                                         # sim3.h:270
    T = np.zeros((4, 4), f32)                                      # Converter.cpp:31-37
    T[:3, :3] = quat_to_R(r).astype(f32)
    T[:3, 3] = np.array(t, f64).astype(f32)
    T[3, 3] = 1.0
    return np.array(r + t + [s], f64), T.reshape(16)


def loop_verify(kf_cur, kf_matched, pts, S, matches, already):
    """LoopClosing.cpp:318-320, :360-370.  Returns a dict: accepted, n_projected, n_total, Scw_sim3, Scw,
    projected int32[kf_cur.n]."""
    S_cw, T = compose(S, kf_matched.Rcw, kf_matched.tcw)
    occupied = (np.asarray(matches) != -1).astype(np.uint8)        # a non-null pointer (-2 included)
    n, out = search_by_projection_kf(kf_cur, pts, T.reshape(4, 4), already, occupied, 10)  # :360
    total = int(occupied.sum()) + n                                # :363-368
    return dict(accepted=int(total >= 40), n_projected=n, n_total=total, Scw_sim3=S_cw, Scw=T, projected=out)


def points_of(**kw):
    """A MapPoint list namespace: n, state, pos, normal, dmax, dmin, desc."""
    n = len(kw["state"])
    return types.SimpleNamespace(n=n, state=np.asarray(kw["state"], np.uint8),
                                 pos=np.asarray(kw["pos"], f32).reshape(n, 3),
                                 normal=np.asarray(kw["normal"], f32).reshape(n, 3),
                                 dmax=np.asarray(kw["dmax"], f32), dmin=np.asarray(kw["dmin"], f32),
                                 desc=np.asarray(kw["desc"], np.uint8).reshape(n, 32))
