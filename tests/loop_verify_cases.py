"""A synthetic LoopClosing::ComputeSim3() event for the closing stage (TEST-ONLY): one small loop event whose
gate (tests/events_oracle.run_loop_gated) accepts its candidate with fewer than 39 matched slots, and
mvpLoopMapPoints lists over it whose sequential restatement (tests/kfproj_ref.loop_verify) ends on exactly 39
(rejected), exactly 40 (accepted) and more matches.

The list is what LoopClosing.cpp:337-357 gathers: the matched KeyFrame's good MapPoints in slot order, then
points of covisible KeyFrames, here placed on keypoints of the current KeyFrame that nothing matched yet (so
they are found by the projection).  SearchByProjection is sequential, so a prefix of the list gives a prefix
of the matches: the 39 / 40 lists are prefixes of the full one, cut after the claim that reaches the count."""
from __future__ import annotations

import types

import numpy as np

import events_oracle as eo
import kfproj_ref as kr
from rsc import synth

SEED, N_POINTS, N_EXTRA, MATCH_FRAC = 4242, 46, 60, 0.75


def event():
    """(kf1, [(kf2, matches12, Sim3Pair)], seeds)"""
    rng = np.random.default_rng(SEED)
    kf1, cands = synth.make_loop_gate_event(rng, [0.95], n_points=N_POINTS, n_extra=N_EXTRA, match_frac=MATCH_FRAC)
    return kf1, cands, [int(x) for x in rng.integers(1, 1 << 30, len(cands))]


def loop_points(kf1, kf2, S, matches, n_covisible: int = 30):
    """(points namespace, already uint8) for the accepted candidate kf2 with gate result (S, matches)."""
    _, T = kr.compose(S, kf2.Rcw, kf2.tcw)
    T = T.reshape(4, 4).astype(np.float64)
    R, t = T[:3, :3], T[:3, 3]
    Ow = -R.T @ t
    sf = synth.scale_factors()
    slots = np.nonzero(kf2.mp_state == 1)[0]                       # LoopClosing.cpp:344-355
    pos = [kf2.mp_pos[s].astype(np.float64) for s in slots]
    desc = [kf2.mp_desc[s] for s in slots]
    dmax = [float(kf2.mp_dmax[s]) for s in slots]
    already = [int(s in set(int(m) for m in matches if m >= 0)) for s in slots]
    free = [f for f in range(kf1.n) if matches[f] == -1 and kf1.mp_id[f] < 0][:n_covisible]
    for f in free:                                                 # a covisible KeyFrame's point seen at keypoint f
        z = 5.0
        Xc = np.array([(kf1.kp[f, 0] - kf1.cx) / kf1.fx * z, (kf1.kp[f, 1] - kf1.cy) / kf1.fy * z, z])
        Xw = R.T @ (Xc - t)
        pos.append(Xw)
        desc.append(kf1.desc[f])
        dmax.append(float(np.linalg.norm(Xw - Ow) * 1.2 ** (int(kf1.octave[f]) - 0.5)))
        already.append(0)
    pos = np.array(pos)
    nrm = pos - Ow
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    dmax = np.array(dmax, np.float32)
    pts = kr.points_of(state=np.ones(len(pos), np.uint8), pos=pos, normal=nrm, dmax=dmax,
                       dmin=(dmax / sf[-1]).astype(np.float32), desc=np.array(desc, np.uint8))
    return pts, np.array(already, np.uint8)


def prefix(pts, already, n):
    return (kr.points_of(state=pts.state[:n], pos=pts.pos[:n], normal=pts.normal[:n], dmax=pts.dmax[:n],
                         dmin=pts.dmin[:n], desc=pts.desc[:n]), already[:n])


def build():
    """A namespace: kf1, cands, seeds, gate (the oracle's record), and `lists` = [(points, already, expected
    restatement dict)] with n_total 39, 40 and the full list's."""
    kf1, cands, seeds = event()
    gate = eo.run_loop_gated(kf1, cands, seeds)
    assert gate["status"] == eo.GATE_MATCH
    kf2 = cands[gate["winner"]][0]
    occupied = int((gate["matches"] != -1).sum())
    assert 20 <= occupied < 39, occupied
    pts, already = loop_points(kf1, kf2, gate["S"], gate["matches"])
    tr = {}
    kr.search_by_projection_kf(kf1, pts, kr.compose(gate["S"], kf2.Rcw, kf2.tcw)[1].reshape(4, 4), already,
                               (gate["matches"] != -1).astype(np.uint8), 10, tr)
    hits = np.nonzero(tr["claim"] >= 0)[0]
    assert occupied + len(hits) > 40, (occupied, len(hits))
    lists = []
    for total in (39, 40, None):
        n = pts.n if total is None else int(hits[total - occupied - 1]) + 1
        p, a = prefix(pts, already, n)
        exp = kr.loop_verify(kf1, kf2, p, gate["S"], gate["matches"], a)
        assert total is None or exp["n_total"] == total
        lists.append((p, a, exp))
    assert [x[2]["accepted"] for x in lists] == [0, 1, 1]
    return types.SimpleNamespace(kf1=kf1, cands=cands, seeds=seeds, gate=gate, kf2=kf2, lists=lists)
