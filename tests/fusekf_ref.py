"""Sequential restatement of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cpp:671-821), the matcher of
LocalMapping::SearchInNeighbors, the reference the device kernel, the host emulation and the facade are compared
with bit for bit (TEST-ONLY):

* ``fuse_kf``: the matcher part, :688-795, numpy float32, point by point in list order: bestIdx when bestDist <=
  TH_LOW, else -1, and which gate rejected what (for the non-vacuity asserts of the tests);
* ``MapPoint`` / ``KeyFrame`` / ``fuse_replay`` / ``search_in_neighbors``: a small map model with the bookkeeping
  of :690-695 and :797-817, ``Replace`` and ``ComputeDistinctiveDescriptors`` as in MapPoint.cpp:158-197,224-290,
  and the forward-plus-backward sequence of LocalMapping.cpp:458-490.  The model iterates a point's observations
  in KeyFrame-id order; the reference iterates in pointer order, which no test can pin.

Float conventions are those of tests/kfproj_ref.py: every operation rounds to its type, fixed-size sums run left
to right."""
from __future__ import annotations

import numpy as np

import kfproj_ref as kr
import oracle_lib as ol
from rsc import synth

f32 = np.float32
TH_LOW = 50
_POP = kr._POP


def inv_level_sigma2(sf) -> np.ndarray:
    """mvInvLevelSigma2 as ORBextractor.cpp:359,367 derives it: 1.0f / (sf[l] * sf[l]), each step rounded."""
    sf = np.asarray(sf, f32)
    return (f32(1.0) / (sf * sf).astype(f32)).astype(f32)


def project(kf, pts, i, th, info=None):
    """:698-736 for point i: (u, v, ur, radius, level) or None when the point is skipped.  With a dict in `info`,
    info['u'], info['v'] = the projection when it was computed."""
    sf, log_sf, _, _ = synth.kf_geometry(kf)
    with np.errstate(all="ignore"):
        R = np.asarray(kf.Rcw, f32).reshape(3, 3)
        t = np.asarray(kf.tcw, f32).reshape(3)
        Ow = np.asarray(kf.Ow, f32).reshape(3)                     # :682 GetCameraCenter(), the stored one
        Xw = np.asarray(pts.pos[i], f32)
        xc = [f32(f32(f32(f32(R[r, 0] * Xw[0]) + f32(R[r, 1] * Xw[1])) + f32(R[r, 2] * Xw[2])) + t[r])
              for r in range(3)]                                   # :699
        if xc[2] < f32(0.0):                                       # :702
            return None
        invz = f32(f32(1.0) / xc[2])                               # :705, float division
        x = f32(xc[0] * invz)
        y = f32(xc[1] * invz)
        u = f32(f32(f32(kf.fx) * x) + f32(kf.cx))                  # :709
        v = f32(f32(f32(kf.fy) * y) + f32(kf.cy))
        if info is not None:
            info["u"], info["v"] = u, v
        if not kr.is_in_image(kf, u, v):                           # :713
            return None
        ur = f32(u - f32(f32(kf.mbf) * invz))                      # :716
        po = [f32(Xw[k] - Ow[k]) for k in range(3)]                # :720
        dist = f32(np.sqrt(f32(f32(f32(po[0] * po[0]) + f32(po[1] * po[1])) + f32(po[2] * po[2]))))
        max_d = f32(f32(1.2) * f32(pts.dmax[i]))                   # :718
        min_d = f32(f32(0.8) * f32(pts.dmin[i]))
        if dist < min_d or dist > max_d:                           # :724
            return None
        Pn = np.asarray(pts.normal[i], f32)
        dot = f32(f32(f32(po[0] * Pn[0]) + f32(po[1] * Pn[1])) + f32(po[2] * Pn[2]))
        if float(dot) < 0.5 * float(dist):                         # :730, compared in double
            return None
        level = ol.lib().ora_predict_scale(float(pts.dmax[i]), float(dist), float(log_sf), len(sf))  # :733
        return u, v, ur, f32(f32(th) * sf[level]), level           # :736


def fuse_kf(kf, pts, skip, th, stats=None):
    """Returns best_idx int32[pts.n].  With a dict in `stats`: counts of keypoints rejected by the level gate, the
    stereo gate and the mono gate, of windows walked, and the largest window."""
    sf = synth.kf_geometry(kf)[0]
    inv_s2 = inv_level_sigma2(sf)
    best = np.full(pts.n, -1, np.int32)
    st = dict(level=0, stereo=0, mono=0, windows=0, largest=0)
    for i in range(pts.n):                                         # :688
        if pts.state[i] != 1 or skip[i]:                           # :695
            continue
        pr = project(kf, pts, i, th)
        if pr is None:
            continue
        u, v, ur, radius, level = pr
        idx = kr.features_in_area(kf, u, v, radius)                # :738
        if idx.size == 0:                                          # :740
            continue
        st["windows"] += 1
        st["largest"] = max(st["largest"], int(idx.size))
        best_dist, best_idx = 256, -1                              # :747
        for f in idx:
            f = int(f)
            o = int(kf.octave[f])
            if o < level - 1 or o > level:                         # :757
                st["level"] += 1
                continue
            ex = f32(u - kf.kp[f, 0])
            ey = f32(v - kf.kp[f, 1])
            if kf.u_right[f] >= 0:                                 # :760 (+0 and -0 are stereo)
                er = f32(ur - kf.u_right[f])
                e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))
                if float(f32(e2 * inv_s2[o])) > 7.8:               # :771
                    st["stereo"] += 1
                    continue
            else:
                e2 = f32(f32(ex * ex) + f32(ey * ey))
                if float(f32(e2 * inv_s2[o])) > 5.99:              # :782
                    st["mono"] += 1
                    continue
            d = int(_POP[np.bitwise_xor(kf.desc[f], pts.desc[i])].sum())
            if d < best_dist:                                      # :790
                best_dist, best_idx = d, f
        if best_dist <= TH_LOW:                                    # :798
            best[i] = best_idx
    if stats is not None:
        stats.update(st)
    return best


# ---- the map model ------------------------------------------------------------------------------------------
class KeyFrame:
    """Slots (MapPoint or None), the stereo flag and the descriptor of every keypoint; `view` is what fuse_kf reads."""

    def __init__(self, kid, view):
        self.id, self.view = kid, view
        self.slots = [None] * view.n
        self.stereo = np.asarray(view.u_right) >= 0
        self.desc = np.asarray(view.desc, np.uint8)


class MapPoint:
    def __init__(self, pid, pos, normal, dmax, dmin, desc):
        self.id, self.bad = pid, False
        self.pos, self.normal, self.dmax, self.dmin = pos, normal, dmax, dmin
        self.desc = np.array(desc, np.uint8)
        self.obs = {}   # KeyFrame id -> (KeyFrame, idx)
        self.nobs = 0
        self.replaced = None

    def is_in_keyframe(self, kf):
        return kf.id in self.obs

    def add_observation(self, kf, idx):                            # MapPoint.cpp:76-87
        if kf.id in self.obs:
            return
        self.obs[kf.id] = (kf, idx)
        self.nobs += 2 if kf.stereo[idx] else 1

    def compute_distinctive_descriptors(self):                     # MapPoint.cpp:224-290
        if self.bad or not self.obs:
            return
        ds = [kf.desc[idx] for _, (kf, idx) in sorted(self.obs.items())]
        n = len(ds)
        D = np.array([[int(_POP[np.bitwise_xor(a, b)].sum()) for b in ds] for a in ds])
        best_median, best = np.iinfo(np.int32).max, 0
        for i in range(n):
            median = sorted(D[i])[int(0.5 * (n - 1))]
            if median < best_median:
                best_median, best = median, i
        self.desc = ds[best].copy()

    def replace(self, other):                                      # MapPoint.cpp:158-197
        if other.id == self.id:
            return
        obs, self.obs, self.bad, self.replaced = self.obs, {}, True, other
        for _, (kf, idx) in sorted(obs.items()):
            if not other.is_in_keyframe(kf):
                kf.slots[idx] = other                              # ReplaceMapPointMatch
                other.add_observation(kf, idx)
            else:
                kf.slots[idx] = None                               # EraseMapPointMatch
        other.compute_distinctive_descriptors()


def points_view(mps):
    """The matcher's view of a MapPoint list without nulls (kfproj_ref.points_of)."""
    return kr.points_of(state=[2 if p.bad else 1 for p in mps], pos=[p.pos for p in mps],
                        normal=[p.normal for p in mps], dmax=[p.dmax for p in mps], dmin=[p.dmin for p in mps],
                        desc=[p.desc for p in mps] if mps else np.zeros((0, 32), np.uint8))


def fuse(kf: KeyFrame, mps, th=3.0, trace=None):
    """ORBmatcher::Fuse(pKF, vpMapPoints, th) on the model, sequentially: every point is matched from the map as
    it stands when the loop reaches it.  mps may hold None and repeated points.  Returns nFused.  With a list in
    `trace`: the bestIdx of every list position as the loop saw it (-1: none or skipped)."""
    n_fused = 0
    for pos, mp in enumerate(mps):
        b = -1
        if mp is not None and not mp.bad and not mp.is_in_keyframe(kf):  # :692-695
            b = int(fuse_kf(kf.view, points_view([mp]), np.zeros(1, np.uint8), th)[0])
        if trace is not None:
            trace.append(b)
        if b < 0:
            continue
        occ = kf.slots[b]                                          # :800
        if occ is not None:
            if not occ.bad:                                        # :803
                if occ.nobs > mp.nobs:                             # :805
                    mp.replace(occ)
                else:
                    occ.replace(mp)
        else:
            mp.add_observation(kf, b)                              # :813
            kf.slots[b] = mp                                       # :814
        n_fused += 1                                               # :816
    return n_fused


def search_in_neighbors(cur: KeyFrame, targets, th=3.0):
    """LocalMapping.cpp:458-490.  Returns (forward nFused per target, candidates of the backward call, its nFused)."""
    matches = list(cur.slots)                                      # :460
    forward = [fuse(k, matches, th) for k in targets]              # :461-466
    cand, seen = [], set()
    for k in targets:                                              # :472-488
        for mp in list(k.slots):
            if mp is None or mp.bad or mp.id in seen:
                continue
            seen.add(mp.id)
            cand.append(mp)
    return forward, cand, fuse(cur, cand, th)                      # :490


def snapshot(kfs, mps):
    """What the facade test compares: every KeyFrame's slots as point ids, every point's bad flag, observations and
    nObs."""
    return dict(slots=[[-1 if s is None else s.id for s in k.slots] for k in kfs],
                bad=[int(p.bad) for p in mps], nobs=[p.nobs for p in mps],
                obs=[sorted((kid, idx) for kid, (_, idx) in p.obs.items()) for p in mps],
                desc=[p.desc.tolist() for p in mps])
