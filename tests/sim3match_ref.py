"""Independent restatement of ORBmatcher::SearchBySim3 (src/ORBmatcher.cpp:948-1170) with a trace (TEST-ONLY).

Pure Python over numpy float32 scalars, one rounding per operation, sharing no code with the kernel
(sim3match.hip) or the C oracle (oracle/sim3match_oracle.cpp); only PredictScale's log is the oracle's
fdlibm restatement, pinned on its own in test_cpu_sim3match.py.  Every quantity of a KeyFrame (intrinsics,
image bounds, scale table, level count, log factor, grid inverses) is read from that KeyFrame object.

py_trace returns both directions (vnMatch1 / vnMatch2), a reason code per source slot, the mutual result
and the branch statistics census() adds up.  PERTURBATIONS lists single rules that can be switched off, each
with the directions it applies to (0 = KF1 -> KF2, 1 = KF2 -> KF1): the CPU tests prove that the hand-built
cases (sim3match_cases.py) notice every one of them.
"""
from __future__ import annotations

import collections
import math
import types

import numpy as np

import oracle_lib as ol
from rsc import synth

f32 = np.float32

# reason codes, in the order the reference tests (the oracle's Sim3Reason)
NOT_SEARCHED, DEPTH, IMAGE, DISTANCE, NO_CANDIDATE, ABOVE_TH_HIGH, MATCHED = range(7)
REASONS = ("not_searched", "depth", "image", "distance", "no_candidate", "above_th_high", "matched")
TH_HIGH = 100
COLS, ROWS = 64, 48

# name -> (directions it applies to, what a kernel with this mistake would do)
PERTURBATIONS = {
    "a_dst_intrinsics": ((0,), "the destination's intrinsics instead of pKF1's (:951-954)"),
    "a_src_intrinsics": ((1,), "the source's intrinsics instead of pKF1's"),
    "b_no_src_translation": ((0, 1), "the source KeyFrame's translation ignored (:1004, :1084)"),
    "c_no_depth": ((0, 1), "no depth test (:1008, :1088)"),
    "d_image_max_inclusive": ((0, 1), "IsInImage with an inclusive maximum"),
    "e_src_bounds": ((0, 1), "IsInImage on the source's bounds"),
    "f_no_min_in_cells": ((0, 1), "- mnMinX / - mnMinY dropped from the cell arithmetic"),
    "g_no_dist_factors": ((0, 1), "distance bounds without the 1.2 / 0.8 factors"),
    "h_dist_max_strict": ((0, 1), "dist3D >= maxDistance rejected"),
    "i_src_log_factor": ((0, 1), "PredictScale with the source's mfLogScaleFactor"),
    "i_src_levels": ((0, 1), "PredictScale with the source's mnScaleLevels"),
    "j_src_scale_table": ((0, 1), "radius from the source's mvScaleFactors"),
    "k_radius_inclusive": ((0, 1), "|dx| <= r"),
    "l_floor_max_cell": ((0, 1), "floor for the maximum cell"),
    "m_octave_plus_one": ((0, 1), "octave window [L-1, L+1]"),
    "n_last_minimum": ((0, 1), "the last minimum wins ties"),
    "o_lowest_index": ((0, 1), "ties to the lowest keypoint index instead of the visiting order"),
    "p_th_high_strict": ((0, 1), "bestDist < TH_HIGH"),
    "q_ignore_already2": ((1,), "vbAlreadyMatched2 ignored"),
    "r_minus2_unmatched": ((0,), "matched12 == -2 treated as unmatched"),
    "s_bad_searched": ((0, 1), "bad MapPoints searched"),
    "t_no_agreement": ((0,), "no agreement step: out12 = vnMatch1"),
}


def _rot(R, x, t=None):
    """Eigen Matrix3f * Vector3f (+ Vector3f), each row summed left to right."""
    R = np.asarray(R, f32).reshape(3, 3)
    o = []
    for r in range(3):
        s = f32(f32(f32(R[r, 0] * x[0]) + f32(R[r, 1] * x[1])) + f32(R[r, 2] * x[2]))
        o.append(s if t is None else f32(s + t[r]))
    return np.array(o, f32)


def _bits(row):
    """A 256-bit descriptor as one integer (the Hamming distance is the popcount of an xor)."""
    return int.from_bytes(np.asarray(row, np.uint8).tobytes(), "little")


def _log(x):
    return f32(ol.lib().ora_dm_log(float(x)))


def _direction(d, src, dst, kf1, Rsd, tsd, already, th, P):
    """One direction (:992-1070 with src = KF1, :1072-1150 with src = KF2): (match, reason, stats)."""
    s_sf, s_log, _, _ = synth.kf_geometry(src)
    d_sf, d_log, gx, gy = synth.kf_geometry(dst)
    cam = kf1
    if "a_dst_intrinsics" in P:
        cam = dst
    if "a_src_intrinsics" in P:
        cam = src
    box = src if "e_src_bounds" in P else dst
    lo_x, hi_x, lo_y, hi_y = f32(box.min_x), f32(box.max_x), f32(box.min_y), f32(box.max_y)
    org_x, org_y = (f32(0), f32(0)) if "f_no_min_in_cells" in P else (f32(dst.min_x), f32(dst.min_y))
    log_sf = s_log if "i_src_log_factor" in P else d_log
    n_levels = len(s_sf) if "i_src_levels" in P else len(d_sf)
    table = s_sf if "j_src_scale_table" in P else d_sf
    dst_desc = [_bits(row) for row in dst.desc]
    match = np.full(src.n, -1, np.int32)
    reason = np.full(src.n, NOT_SEARCHED, np.int32)
    st = collections.Counter()
    for i in range(src.n):
        state = int(src.mp_state[i])
        if state == 0 or already[i] or (state != 1 and "s_bad_searched" not in P):
            continue
        tcw = np.asarray(src.tcw, f32).reshape(3)
        pc = _rot(src.Rcw, src.mp_pos[i], None if "b_no_src_translation" in P else tcw)
        pd = _rot(Rsd, pc, tsd)
        if pd[2] < 0 and "c_no_depth" not in P:
            reason[i] = DEPTH
            continue
        invz = f32(1.0 / np.float64(pd[2]))
        x, y = f32(pd[0] * invz), f32(pd[1] * invz)
        u = f32(f32(f32(cam.fx) * x) + f32(cam.cx))
        v = f32(f32(f32(cam.fy) * y) + f32(cam.cy))
        if "d_image_max_inclusive" in P:
            inside = u >= lo_x and u <= hi_x and v >= lo_y and v <= hi_y
        else:
            inside = u >= lo_x and u < hi_x and v >= lo_y and v < hi_y
        if not inside:
            reason[i] = IMAGE
            continue
        dmax, dmin = f32(src.mp_dmax[i]), f32(src.mp_dmin[i])
        mx, mn = (dmax, dmin) if "g_no_dist_factors" in P else (f32(f32(1.2) * dmax), f32(f32(0.8) * dmin))
        d3 = f32(np.sqrt(f32(f32(f32(pd[0] * pd[0]) + f32(pd[1] * pd[1])) + f32(pd[2] * pd[2]))))
        if d3 < mn or d3 > mx or ("h_dist_max_strict" in P and d3 >= mx):
            reason[i] = DISTANCE
            continue
        # MapPoint::PredictScale (MapPoint.cpp:367-381)
        raw = math.ceil(f32(_log(f32(dmax / d3)) / log_sf))
        st["level_clamp_low"] += raw < 0
        st["level_clamp_high"] += raw >= n_levels
        lvl = min(max(raw, 0), n_levels - 1)
        lvl_r = min(lvl, len(table) - 1)  # only a perturbed table can be shorter than the level count
        r = f32(f32(th) * table[lvl_r])
        # KeyFrame::GetFeaturesInArea (KeyFrame.cpp:560-599)
        fx0 = math.floor(f32(f32(f32(u - org_x) - r) * gx))
        fx1 = f32(f32(f32(u - org_x) + r) * gx)
        fy0 = math.floor(f32(f32(f32(v - org_y) - r) * gy))
        fy1 = f32(f32(f32(v - org_y) + r) * gy)
        top = math.floor if "l_floor_max_cell" in P else math.ceil
        fx1, fy1 = top(fx1), top(fy1)
        x0, x1, y0, y1 = max(0, fx0), min(COLS - 1, fx1), max(0, fy0), min(ROWS - 1, fy1)
        reason[i] = NO_CANDIDATE
        if x0 >= COLS or x1 < 0 or y0 >= ROWS or y1 < 0:
            continue
        st["clamp_min_x"] += fx0 < 0
        st["clamp_max_x"] += fx1 > COLS - 1
        st["clamp_min_y"] += fy0 < 0
        st["clamp_max_y"] += fy1 > ROWS - 1
        hi_oct = lvl + 1 if "m_octave_plus_one" in P else lvl
        best, bi, ties = 1 << 31, -1, 0
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                c = ix * ROWS + iy
                for e in range(int(dst.cell_begin[c]), int(dst.cell_begin[c + 1])):
                    j = int(dst.cell_feat[e])
                    dx, dy = abs(f32(dst.kp[j, 0] - u)), abs(f32(dst.kp[j, 1] - v))
                    if "k_radius_inclusive" in P:
                        near = dx <= r and dy <= r
                    else:
                        near = dx < r and dy < r
                    if not near or dst.octave[j] < lvl - 1 or dst.octave[j] > hi_oct:
                        continue
                    dd = bin(_bits(src.mp_desc[i]) ^ dst_desc[j]).count("1")
                    if dd == best:
                        ties += 1
                        if "n_last_minimum" in P or ("o_lowest_index" in P and j < bi):
                            bi = j
                    elif dd < best:
                        best, bi, ties = dd, j, 0
        if bi < 0:
            continue
        st["tie"] += ties > 0
        st["best_100"] += best == 100
        st["best_101"] += best == 101
        if best < TH_HIGH or (best == TH_HIGH and "p_th_high_strict" not in P):
            match[i], reason[i] = bi, MATCHED
        else:
            reason[i] = ABOVE_TH_HIGH
    for k, v in enumerate(np.bincount(reason, minlength=len(REASONS))):
        st[REASONS[k]] = int(v)
    return match, reason, st


def py_trace(kf1, kf2, R12, t12, m12, th=7.5, perturb=None, dirs=None):
    """SearchBySim3 with its trace: a namespace of nfound, out, m1, m2, reason1, reason2 and stats (one
    Counter per direction).  perturb: a PERTURBATIONS key, applied in the directions `dirs` (default: all it
    applies to)."""
    P = [set(), set()]
    if perturb is not None:
        for d in (PERTURBATIONS[perturb][0] if dirs is None else dirs):
            assert d in PERTURBATIONS[perturb][0], (perturb, d)
            P[d].add(perturb)
    R12 = np.asarray(R12, f32).reshape(3, 3)
    t12 = np.asarray(t12, f32).reshape(3)
    R21 = R12.T.copy()   # R21 = R12^T, t21 = -R21 * t12 (:963-964)
    t21 = np.array([-v for v in _rot(R21, t12)], f32)
    m12 = np.asarray(m12, np.int32)
    a1 = [m >= 0 if "r_minus2_unmatched" in P[0] else m != -1 for m in m12]   # (:972-984)
    a2 = [False] * kf2.n
    if "q_ignore_already2" not in P[1]:
        for m in m12:
            if m >= 0:
                a2[m] = True
    with np.errstate(all="ignore"):
        m1, r1, s1 = _direction(0, kf1, kf2, kf1, R21, t21, a1, th, P[0])
        m2, r2, s2 = _direction(1, kf2, kf1, kf1, R12, t12, a2, th, P[1])
    out = np.full(kf1.n, -1, np.int32)   # check agreement (:1152-1167)
    for i in range(kf1.n):
        if m1[i] >= 0 and (m2[m1[i]] == i or "t_no_agreement" in P[0]):
            out[i] = m1[i]
    return types.SimpleNamespace(nfound=int((out >= 0).sum()), out=out, m1=m1, m2=m2, reason1=r1, reason2=r2,
                                 stats=(s1, s2))


def py_search(kf1, kf2, R12, t12, m12, th=7.5):
    """(nFound, out12), the interface of oracle_lib.search_by_sim3."""
    t = py_trace(kf1, kf2, R12, t12, m12, th)
    return t.nfound, t.out


def census(traces):
    """Branch statistics summed over py_trace results, per direction: a pair of dicts with the reason counts
    (REASONS), `tie` (slots whose minimum distance was reached by more than one eligible keypoint),
    `best_100` / `best_101`, `level_clamp_low` / `level_clamp_high` (PredictScale's two clamps taken) and
    `clamp_min_x` / `clamp_max_x` / `clamp_min_y` / `clamp_max_y` (cell ranges cut at the grid's four sides)."""
    keys = REASONS + ("tie", "best_100", "best_101", "level_clamp_low", "level_clamp_high", "clamp_min_x",
                      "clamp_max_x", "clamp_min_y", "clamp_max_y")
    tot = (collections.Counter(), collections.Counter())
    for t in traces:
        for d in (0, 1):
            tot[d].update(t.stats[d])
    return tuple({k: int(tot[d][k]) for k in keys} for d in (0, 1))
