"""ORBmatcher::SearchBySim3 oracle (oracle/sim3match_oracle.cpp) pinned on CPU:

* the fdlibm log restatement used for MapPoint::PredictScale (rsc_math.h) against numpy / glibc;
* PredictScale (MapPoint.cpp:367-381) on hand-made ratios, including both clamps;
* hand-built known answers (ORBmatcher.cpp:948-1170): the mutual-agreement rule, already-matched
  (with and without an index in KF2) and bad MapPoints, the octave window [level-1, level],
  TH_HIGH inclusive;
* an independent pure-Python restatement (sim3match_ref.py, numpy float32 scalars) against the C
  oracle on random pairs: these reach the depth, IsInImage and scale-invariance branches, but both
  KeyFrames of a random pair share intrinsics, bounds and pyramid and KF1 sits at the origin, so
  "pKF1's intrinsics in both directions", source/destination mix-ups, exact boundaries and tie order
  are NOT exercised here — test_cpu_sim3match_cases.py does that on hand-built cases and pins which
  mistakes the random pairs miss;
* the committed golden fixture tests/golden/sim3match_traces.npz.

The reference ships no tests for this path; the known answers follow its text.
"""
import math
import os

import numpy as np
import pytest

import oracle_lib as ol
from rsc import synth
from sim3match_ref import py_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_log_restatement_within_one_ulp():
    rng = np.random.default_rng(3)
    x = np.exp(rng.uniform(-40, 40, 20000))
    L = ol.lib()
    got = np.array([L.ora_dm_log(float(v)) for v in x])
    ref = np.log(x)
    ulp = np.abs(np.spacing(ref))
    assert (np.abs(got - ref) <= ulp).all()
    # logf as the float rounding: equal to float32(log) except within an ulp of a rounding boundary
    xf = x.astype(np.float32)
    lf = np.array([np.float32(L.ora_dm_log(float(v))) for v in xf])
    assert (lf == np.log(xf.astype(np.float64)).astype(np.float32)).mean() > 0.999


@pytest.mark.parametrize("dmax,dist,expect", [
    (1.0, 1.0, 0),             # log(1) = 0 -> ceil(0) = 0
    (1.0, 2.0, 0),             # negative -> clamped to 0
    (10.0, 1.0, 7),            # ceil(log(10)/log(1.2)) = 13 -> clamped to levels - 1
    (1.44, 1.0, 2),            # 1.2^2 in float: log ratio / log 1.2 rounds to just above or at 2
    (1.3, 1.0, 2),             # between 1.2 and 1.44 -> 2
    (1.1, 1.0, 1),
])
def test_predict_scale(dmax, dist, expect):
    got = ol.lib().ora_predict_scale(dmax, dist, float(synth.LOG_SCALE_FACTOR), 8)
    if dmax == 1.44:
        r = f32(f32(dmax) / f32(dist))
        q = f32(np.float32(ol.lib().ora_dm_log(float(r))) / synth.LOG_SCALE_FACTOR)
        expect = int(math.ceil(q))
    assert got == expect


def test_random_pairs_match_python_restatement():
    for seed in range(3):
        kf1, kf2, R12, t12, m12 = synth.make_sim3match_pair(np.random.default_rng(100 + seed), n_points=150,
                                                            n_extra=60)
        nf, out = ol.search_by_sim3(kf1, kf2, R12, t12, m12)
        pnf, pout = py_search(kf1, kf2, R12, t12, m12)
        assert nf == pnf and np.array_equal(out, pout), seed
        assert nf > 5


# ---- known answers --------------------------------------------------------------------------
def tiny_pair(n=1):
    """KF1 and KF2 with identity poses looking at points straight ahead; R12 = I, t12 = 0."""
    rng = np.random.default_rng(7)
    P = np.array([[0.1 * i, 0.05 * i, 4.0] for i in range(n)], np.float32)

    def kf(extra_kp=None):
        uv = np.stack([synth.FX * P[:, 0] / P[:, 2] + synth.CX, synth.FY * P[:, 1] / P[:, 2] + synth.CY], 1)
        kp = uv.astype(np.float32)
        if extra_kp is not None:
            kp = np.concatenate([kp, np.asarray(extra_kp, np.float32)])
        m = len(kp)
        begin, feat = synth.build_grid(kp)
        desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        state = np.zeros(m, np.uint8)
        state[:n] = 1
        pos = np.zeros((m, 3), np.float32)
        pos[:n] = P
        dmax = np.zeros(m, np.float32)
        dmax[:n] = 4.0
        dmin = (dmax / synth.scale_factors()[-1]).astype(np.float32)
        mdesc = desc.copy()
        return synth.Sim3KF(m, kp, np.zeros(m, np.int32), desc, begin, feat, np.eye(3, dtype=np.float32),
                            np.zeros(3, np.float32), state, pos, dmax, dmin, mdesc, np.arange(m))
    return kf, P


def run_tiny(kf1, kf2, m12=None):
    if m12 is None:
        m12 = np.full(kf1.n, -1, np.int32)
    I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    nf, out = ol.search_by_sim3(kf1, kf2, I, z, m12)
    pnf, pout = py_search(kf1, kf2, I, z, m12)
    assert nf == pnf and np.array_equal(out, pout)
    return nf, out


def matched_tiny(kf):
    a, b = kf(), kf()
    b.desc[0] = a.mp_desc[0]  # KF2's keypoint carries KF1's MapPoint descriptor and vice versa
    a.desc[0] = b.mp_desc[0]
    return a, b


def test_mutual_match_and_rejections():
    kf, P = tiny_pair(1)
    k1, k2 = matched_tiny(kf)
    nf, out = run_tiny(k1, k2)
    assert nf == 1 and out.tolist() == [0]
    # already matched (a MapPoint in vpMatches12 with or without an index in KF2) -> not searched
    assert run_tiny(k1, k2, np.array([0], np.int32))[0] == 0
    assert run_tiny(k1, k2, np.array([-2], np.int32))[0] == 0
    # bad MapPoint in KF1
    a, b = matched_tiny(kf)
    a.mp_state[0] = 2
    assert run_tiny(a, b)[0] == 0
    # octave outside [level-1, level]: predicted level 0 (dist == dmax), KF2's keypoint at octave 3
    a, b = matched_tiny(kf)
    b.octave[0] = 3
    assert run_tiny(a, b)[0] == 0
    # one direction only (KF2's MapPoint descriptor far from KF1's keypoint): no agreement
    a, b = matched_tiny(kf)
    a.desc[0] = np.bitwise_not(b.mp_desc[0])
    assert run_tiny(a, b)[0] == 0


def test_th_high_inclusive():
    kf, P = tiny_pair(1)
    k1, k2 = matched_tiny(kf)
    # KF2 keypoint at Hamming distance exactly 100 from KF1's MapPoint descriptor
    d = k1.mp_desc[0].copy()
    bits = np.arange(100)
    np.bitwise_xor.at(d, bits // 8, (1 << (bits % 8)).astype(np.uint8))
    k2.desc[0] = d
    assert run_tiny(k1, k2)[0] == 1
    np.bitwise_xor.at(d, np.array([100 // 8]), np.array([1 << (100 % 8)], np.uint8))
    k2.desc[0] = d
    assert run_tiny(k1, k2)[0] == 0


def test_golden_sim3match_traces():
    g = np.load(os.path.join(ROOT, "tests", "golden", "sim3match_traces.npz"))
    for k in range(int(g["cases"])):
        kfs = []
        for side in ("A", "B"):
            f = {x: g[f"c{k}_{side}_{x}"] for x in ("kp", "octave", "desc", "cell_begin", "cell_feat", "Rcw", "tcw",
                                                    "mp_state", "mp_pos", "mp_dmax", "mp_dmin", "mp_desc")}
            kfs.append(synth.Sim3KF(len(f["kp"]), mp_id=np.zeros(len(f["kp"]), np.int64), **f))
        nf, out = ol.search_by_sim3(kfs[0], kfs[1], g[f"c{k}_R12"], g[f"c{k}_t12"], g[f"c{k}_m12"])
        assert nf == int(g[f"c{k}_n"]) and nf > 0, k
        assert np.array_equal(out, g[f"c{k}_out"]), k
