"""Hand-built problems for MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (TEST-ONLY), one per rule,
each with the answer worked out by hand, and the seeded random problems of the size classes.

Descriptors are ``bits(a)``: the lowest a bits set, so the distance of bits(a) and bits(b) is |a - b| and a list of
descriptors is a list of numbers on a line.  The rank (int)(0.5*(N-1)) of a sorted row (the diagonal zero included)
is 0 for N <= 2, 1 for N = 3 and 4 (the distance to the nearest other descriptor), 2 for N = 5 and 6.

``cases()`` returns name -> (problem, expect); expect holds best_obs (list, None = untouched), desc (the number a of
the winner per point, None = not written) and, where worked out, normal / dmax / dmin as float32 values."""
from __future__ import annotations

import types

import numpy as np

from rsc import synth

f32 = np.float32
SF = synth.scale_factors()  # mvScaleFactors: 1.2^l, 8 levels


def bits(a: int) -> np.ndarray:
    d = np.zeros(32, np.uint8)
    for b in range(a):
        d[b // 8] |= 1 << (b % 8)
    return d


class Builder:
    def __init__(self):
        self.kfs, self.pts = [], []

    def kf(self, descs, octaves=None, Ow=(0.0, 0.0, 0.0), bad=False) -> int:
        """descs: numbers a (bits(a)) or 32-byte arrays."""
        d = np.array([bits(x) if np.isscalar(x) else np.asarray(x, np.uint8) for x in descs], np.uint8).reshape(-1, 32)
        o = np.zeros(len(d), np.int32) if octaves is None else np.asarray(octaves, np.int32)
        self.kfs.append(types.SimpleNamespace(n=len(d), desc=d, octave=o, scale=SF, Ow=np.asarray(Ow, f32), bad=bad))
        return len(self.kfs) - 1

    def point(self, pos, obs, ref=None, skip=False) -> int:
        """obs: [(kf, idx)] in mObservations order; ref: (kf, idx), default the first observation."""
        self.pts.append(dict(pos=pos, obs=list(obs), ref=ref if ref is not None else (obs[0] if obs else (0, 0)),
                             skip=skip))
        return len(self.pts) - 1

    def problem(self):
        n = len(self.pts)
        begin = np.zeros(n + 1, np.int32)
        begin[1:] = np.cumsum([len(p["obs"]) for p in self.pts])
        flat = [o for p in self.pts for o in p["obs"]]
        upd = types.SimpleNamespace(
            n_points=n, skip=np.array([p["skip"] for p in self.pts], np.uint8),
            pos=np.array([p["pos"] for p in self.pts], f32).reshape(n, 3), obs_begin=begin,
            obs_kf=np.array([o[0] for o in flat], np.int32), obs_idx=np.array([o[1] for o in flat], np.int32),
            kf_bad=np.array([k.bad for k in self.kfs], np.uint8),
            ref_kf=np.array([p["ref"][0] for p in self.pts], np.int32),
            ref_idx=np.array([p["ref"][1] for p in self.pts], np.int32))
        return types.SimpleNamespace(kfs=self.kfs, upd=upd)


def line(numbers, pos=(0.0, 0.0, 2.0), bad=(), Ows=None):
    """One point whose observation i is keypoint 0 of a KeyFrame of its own with descriptor bits(numbers[i])."""
    b = Builder()
    ks = [b.kf([a], Ow=(0.0, 0.0, 0.0) if Ows is None else Ows[i], bad=i in bad) for i, a in enumerate(numbers)]
    b.point(pos, [(k, 0) for k in ks])
    return b


def cases():
    out = {}
    # N = 1: the only row
    out["n1"] = (line([5], pos=(3.0, 0.0, 4.0)).problem(),
                 dict(best_obs=[0], desc=[5], normal=[(f32(3) / f32(5), f32(0), f32(4) / f32(5))], dmax=[f32(5)],
                      dmin=[f32(5) / SF[7]]))
    # N = 2: both medians are the diagonal zero, the first row stays
    out["n2_first"] = (line([10, 0]).problem(), dict(best_obs=[0], desc=[10]))
    # N = 3, rank 1: rows [0,7,10] -> 7, [0,3,10] -> 3, [0,3,7] -> 3.  Rows 1 and 2 tie: the first wins; a <= rule
    # would end on row 2, another descriptor
    out["tie_first_wins"] = (line([0, 10, 7]).problem(), dict(best_obs=[1], desc=[10], le_rule=[2]))
    # N = 4, rank 1 (the lower median): every row's nearest other descriptor is 1 away -> row 0.  The upper median
    # (rank 2) would be 5, 4, 4, 5 -> row 1
    out["even4_lower_median"] = (line([0, 1, 5, 6]).problem(), dict(best_obs=[0], desc=[0], upper_rule=[1]))
    # N = 5, rank 2: rows sorted [0,3,4,9,20] [0,1,3,6,17] [0,1,4,5,16] [0,5,6,9,11] [0,11,16,17,20] -> medians
    # 4, 3, 4, 6, 16 -> row 1
    out["odd5"] = (line([0, 3, 4, 9, 20]).problem(), dict(best_obs=[1], desc=[3], medians=[[4, 3, 4, 6, 16]]))
    # N = 6, rank 2: medians 11, 2, 1, 2, 3, 18 -> row 2; the upper median (rank 3) gives 12, 4, 3, 2, 4, 19 -> row 3
    out["even6_lower_median"] = (line([0, 10, 11, 12, 14, 30]).problem(),
                                 dict(best_obs=[2], desc=[11], medians=[[11, 2, 1, 2, 3, 18]], upper_rule=[3]))
    # duplicates: rows 1, 2, 3 are the same descriptor, each sees two zeros beside its own -> median 0, first of them
    out["duplicates"] = (line([4, 9, 9, 9]).problem(), dict(best_obs=[1], desc=[9], medians=[[5, 0, 0, 0]]))
    # a pair at distance 256: row 0 (all zeros) against two all-ones rows has the median 256
    out["distance_256"] = (line([0, 256, 256]).problem(), dict(best_obs=[1], desc=[256], medians=[[256, 0, 0]]))
    # a bad KeyFrame (observation 1) is dropped for the descriptor: kept [0, 10, 7] -> kept row 1 = observation 2.
    # With it the rows would be N = 4, rank 1: 1, 1, 3, 3 -> observation 0.  The normal counts all four:
    # the point (0,0,2) sees three centres at the origin and the bad one at (0,0,1): (0,0,1) each, sum 4, / 4
    out["bad_kf_skipped"] = (line([0, 1, 10, 7], bad={1}, Ows=[(0, 0, 0), (0, 0, 1), (0, 0, 0), (0, 0, 0)]).problem(),
                             dict(best_obs=[2], desc=[10], with_bad=[0], normal=[(f32(0), f32(0), f32(1))],
                                  dmax=[f32(2)], dmin=[f32(2) / SF[7]]))
    # every KeyFrame bad: no descriptor, the normal is written all the same
    out["all_kfs_bad"] = (line([3, 8], bad={0, 1}).problem(),
                          dict(best_obs=[-1], desc=[None], normal=[(f32(0), f32(0), f32(1))], dmax=[f32(2)],
                               dmin=[f32(2) / SF[7]], updated=[2]))
    # an empty list and a bad point are left untouched, next to a point that is updated
    b = Builder()
    k0, k1 = b.kf([6, 2]), b.kf([1])
    b.point((0.0, 0.0, 2.0), [])
    b.point((0.0, 0.0, 2.0), [(k0, 0), (k1, 0)], skip=True)
    b.point((0.0, 0.0, 2.0), [(k0, 1), (k1, 0)])
    out["untouched"] = (b.problem(), dict(best_obs=[None, None, 0], desc=[None, None, 2], updated=[0, 0, 3]))
    # the reference KeyFrame at every pyramid level, the top included: dist = 5, dmax = 5 * 1.2^l, dmin = dmax / 1.2^7
    b = Builder()
    k = b.kf([0] * 8, octaves=list(range(8)))
    for l in range(8):
        b.point((3.0, 0.0, 4.0), [(k, l)])
    out["ref_levels"] = (b.problem(), dict(best_obs=[0] * 8, desc=[0] * 8, dmax=[f32(5) * SF[l] for l in range(8)],
                                           dmin=[f32(f32(5) * SF[l]) / SF[7] for l in range(8)]))
    # the reference KeyFrame is not the first observation, and its index is not the observation's
    b = Builder()
    k0, k1 = b.kf([1, 2], octaves=[0, 3], Ow=(0.0, 0.0, 1.0)), b.kf([2, 3], octaves=[1, 5], Ow=(0.0, 0.0, -2.0))
    b.point((0.0, 0.0, 2.0), [(k0, 0), (k1, 0)], ref=(k1, 1))
    out["ref_elsewhere"] = (b.problem(), dict(best_obs=[0], desc=[1], normal=[(f32(0), f32(0), f32(1))],
                                              dmax=[f32(4) * SF[5]], dmin=[f32(f32(4) * SF[5]) / SF[7]]))
    # a point on a camera centre: 0/0, the normal is NaN; the depth comes from the other KeyFrame and is finite
    b = Builder()
    k0, k1 = b.kf([1], Ow=(1.0, 2.0, 3.0)), b.kf([2], Ow=(0.0, 0.0, 0.0))
    b.point((1.0, 2.0, 3.0), [(k1, 0), (k0, 0)], ref=(k1, 0))
    b.point((1.0, 2.0, 3.0), [(k0, 0)])
    out["at_camera_centre"] = (b.problem(), dict(best_obs=[0, 0], desc=[2, 1], nan_normal=[True, True],
                                                 nan_depth=[False, False]))  # dist = 0 gives dmax = dmin = 0
    # a list whose order shows in the bits of the normal (float addition is not associative)
    Ows = [(0.3, -1.7, 0.2), (5.1, 0.4, -0.9), (-2.2, 3.3, 0.7), (0.05, 0.01, -7.5), (1.9, -0.6, 1.1), (-4.4, -4.1, 0.3),
           (0.7, 0.8, -0.1)]
    out["order_matters"] = (line(list(range(7)), pos=(0.37, 0.11, 3.3), Ows=Ows).problem(),
                            dict(best_obs=[1], desc=[1], medians=[[3, 2, 2, 2, 2, 2, 3]]))  # rank 3 of 7
    return out


RANDOM_SEEDS = {"random_a": 31, "random_b": 32}
RANDOM_SIZES = (1, 2, 3, 63, 64, 65, 200, 1024)


def random_problem(seed: int, n_kf: int = 4, n_kp: int = 1100):
    """Four KeyFrames of 1,100 keypoints and one point per list length of RANDOM_SIZES (both size classes and the
    64 / 65 boundary in one call), then a few short ones.  Descriptors are a handful of centres with up to 40
    flipped bits, so rows tie on their medians; the observations of a list are distinct (KeyFrame, keypoint) pairs.
    random_b marks KeyFrame 2 bad."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    b = Builder()
    for k in range(n_kf):
        d = centres[rng.integers(0, len(centres), n_kp)].copy()
        for i in range(n_kp):
            for bit in rng.choice(256, int(rng.integers(0, 41)), replace=False):
                d[i, bit // 8] ^= 1 << (bit % 8)
        b.kf(d, octaves=rng.integers(0, 8, n_kp), Ow=rng.uniform(-3, 3, 3), bad=(seed == RANDOM_SEEDS["random_b"] and k == 2))
    for n in RANDOM_SIZES + (5, 12, 7, 30):
        pick = rng.choice(n_kf * n_kp, n, replace=False)
        obs = [(int(x) // n_kp, int(x) % n_kp) for x in pick]
        b.point(rng.uniform(-2, 2, 3) + (0, 0, 6), obs, ref=obs[int(rng.integers(0, n))])
    return b.problem()
