"""Sequential restatement of Frame::ComputeStereoMatches() (src/Frame.cpp:538-673, the keypoint-only matcher) in
numpy and plain Python, in the reference's own order: sort the right keypoints by (y, index), two binary searches
with <=, an ordered scan with a strict <, a second sort of (dist, i), and the walk from the back.  It shares no
decomposition with the kernel (no key, no histogram, no threshold sweep): those equivalences are what the tests
check.  TEST-ONLY.

A frame is a types.SimpleNamespace with kp float32 [n,2] (mvKeysUn pt), octave int32 [n], desc uint8 [n,32], scale
float32 [n_levels], r_kp float32 [m,2] (mvKeysRight pt), r_octave int32 [m], r_desc uint8 [m,32], mbf, mb."""
from __future__ import annotations

import types

import numpy as np

F32 = np.float32
TH_HIGH, TH_LOW = 100, 50
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def frame(kp, octave, desc, scale, r_kp, r_octave, r_desc, mbf, mb):
    return types.SimpleNamespace(
        kp=np.asarray(kp, np.float32).reshape(-1, 2), octave=np.asarray(octave, np.int32).reshape(-1),
        desc=np.asarray(desc, np.uint8).reshape(-1, 32), scale=np.asarray(scale, np.float32).reshape(-1),
        r_kp=np.asarray(r_kp, np.float32).reshape(-1, 2), r_octave=np.asarray(r_octave, np.int32).reshape(-1),
        r_desc=np.asarray(r_desc, np.uint8).reshape(-1, 32), mbf=F32(mbf), mb=F32(mb))


def descriptor_distance(a, b) -> int:
    return int(POP[np.bitwise_xor(a, b)].sum())


def _upper(ordered_y, target):
    """The reference's search (:569-584): the first position whose y is not <= target, -1 when there is none."""
    high, low, found = len(ordered_y), 0, -1
    while low < high:
        mid = low + (high - low) // 2
        if ordered_y[mid] <= target:
            low = mid + 1
        else:
            found = mid
            high = mid
    return found


def compute(fr):
    """dict(u_right, depth float32 [n]; best_right, best_dist int32 [n] (before the cut, -1: not accepted);
    n_candidates, n_removed, median, th_dist)."""
    with np.errstate(all="ignore"):
        return _compute(fr)


def _compute(fr):
    N, M = len(fr.kp), len(fr.r_kp)
    u_right = np.full(N, -1.0, np.float32)
    depth = np.full(N, -1.0, np.float32)
    best_right = np.full(N, -1, np.int32)
    best_dist = np.full(N, -1, np.int32)
    th_orb = (TH_HIGH + TH_LOW) // 2
    # std::sort of pair<float, uint16_t>: by y, then by index; Python compares -0.0 == 0.0 as C++ does
    ordered = sorted((float(fr.r_kp[i, 1]), i) for i in range(M))
    ordered_y = [F32(y) for y, _ in ordered]
    max_d = F32(fr.mbf) / F32(fr.mb)
    dist_idx = []
    for i in range(N):
        uL, yL = F32(fr.kp[i, 0]), F32(fr.kp[i, 1])
        min_u = uL - max_d
        max_u = uL - F32(0)
        if max_u < 0:
            continue
        level = int(fr.octave[i])
        r = F32(2.0) * F32(fr.scale[level])
        idx_min = _upper(ordered_y, yL - r)
        if idx_min == -1:
            continue
        idx_max = _upper(ordered_y, yL + r)
        if idx_max == 0:
            continue
        if idx_max == -1:
            idx_max = M
        best, best_idx = TH_HIGH, -1
        for pos in range(idx_min, idx_max):
            j = ordered[pos][1]
            oct_r = int(fr.r_octave[j])
            if oct_r < level - 1 or oct_r > level + 1:
                continue
            uR = F32(fr.r_kp[j, 0])
            if uR >= min_u and uR <= max_u:
                d = descriptor_distance(fr.desc[i], fr.r_desc[j])
                if d < best:
                    best, best_idx = d, j
        if best < th_orb:
            best_uR = F32(fr.r_kp[best_idx, 0])
            disparity = uL - best_uR
            if disparity >= 0 and disparity < max_d:
                u_right[i] = best_uR
                if disparity <= 0:
                    disparity = F32(0.01)
                    u_right[i] = F32(np.float64(uL) - np.float64(0.01))
                depth[i] = F32(fr.mbf) / disparity
                dist_idx.append((best, i))
                best_right[i], best_dist[i] = best_idx, best
    dist_idx.sort()
    removed = 0
    if dist_idx:
        median = dist_idx[len(dist_idx) // 2][0]
        th_dist = F32(1.5) * F32(1.4) * F32(median)
        for k in range(len(dist_idx) - 1, -1, -1):
            if F32(dist_idx[k][0]) < th_dist:
                break
            u_right[dist_idx[k][1]] = -1.0
            depth[dist_idx[k][1]] = -1.0
            removed += 1
    else:  # the reference reads vDistIdx[0] of an empty vector; pinned by the C ABI
        median = -1
        th_dist = F32(1.5) * F32(1.4) * F32(-1)
    return dict(u_right=u_right, depth=depth, best_right=best_right, best_dist=best_dist,
                n_candidates=len(dist_idx), n_removed=removed, median=int(median), th_dist=F32(th_dist))


def same(a, b) -> list:
    """The fields in which two results differ (floats compared as bits)."""
    bad = []
    for k in ("u_right", "depth"):
        if not np.array_equal(np.asarray(a[k], np.float32).view(np.uint32), np.asarray(b[k], np.float32).view(np.uint32)):
            bad.append(k)
    for k in ("best_right", "best_dist"):
        if not np.array_equal(a[k], b[k]):
            bad.append(k)
    for k in ("n_candidates", "n_removed", "median"):
        if int(a[k]) != int(b[k]):
            bad.append(k)
    if np.float32(a["th_dist"]).view(np.uint32) != np.float32(b["th_dist"]).view(np.uint32):
        bad.append("th_dist")
    return bad
