"""Sequential restatement of MapPoint::ComputeDistinctiveDescriptors() (src/MapPoint.cpp:224-289) and
MapPoint::UpdateNormalAndDepth() (:312-353), the reference the device kernel, the host emulation and the facade are
compared with bit for bit (TEST-ONLY).  numpy float32: every operation rounds to float, sums run in list order.
Written on its own, not from fusekf_ref.MapPoint.compute_distinctive_descriptors (tests/test_cpu_mpupdate.py checks
that the two agree).

A problem is a namespace: ``kfs`` (a list of namespaces with n, desc uint8 [n,32], octave int32 [n], scale float32
[n_levels], Ow float32 [3]) and ``upd`` (n_points, skip, pos, obs_begin, obs_kf, obs_idx, kf_bad, ref_kf, ref_idx:
rsc_mappoint_updates of include/rsc.h)."""
from __future__ import annotations

import numpy as np

f32 = np.float32
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)
INT_MAX = np.iinfo(np.int32).max
# what an entry holds that a call did not write (rsc.engine.MPUPDATE_FILL)
FILL = dict(desc=0xA5, best_obs=-7, normal=f32(-77.0), dmax=f32(-77.0), dmin=f32(-77.0))


def distances(descs) -> np.ndarray:
    """float Distances[N][N] (:257-267): DescriptorDistance of every pair, zero on the diagonal."""
    d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
    D = _POP[d[:, None, :] ^ d[None, :, :]].sum(axis=2, dtype=np.int32).astype(f32)
    np.fill_diagonal(D, f32(0))                                    # :260
    return D


def row_medians(descs) -> np.ndarray:
    """vDists[0.5*(N-1)] of every sorted row (:274-276)."""
    D = distances(descs)
    n = len(D)
    return np.sort(D, axis=1)[:, int(0.5 * (n - 1))].astype(np.int32)


def best_row(descs) -> int:
    """BestIdx (:270-283): a strict < from INT_MAX keeps the first row of the smallest median."""
    best_median, best = INT_MAX, 0
    for i, median in enumerate(row_medians(descs)):
        if median < best_median:
            best_median, best = int(median), i
    return best


def norm3(x):
    """Vector3f::norm(): sqrtf((x*x + y*y) + z*z)."""
    return np.sqrt(f32(f32(f32(x[0] * x[0]) + f32(x[1] * x[1])) + f32(x[2] * x[2])))


def normal_and_depth(pos, Ows, Ow_ref, level_scale, top_scale):
    """:330-352 given the camera centres of the list in order: (mNormalVector, mfMaxDistance, mfMinDistance)."""
    pos = np.asarray(pos, f32)
    normal = np.zeros(3, f32)                                       # :330
    with np.errstate(invalid="ignore", divide="ignore"):
        for Ow in Ows:                                              # :332-339
            normali = (pos - np.asarray(Ow, f32)).astype(f32)
            normal = (normal + (normali / norm3(normali)).astype(f32)).astype(f32)
        PC = (pos - np.asarray(Ow_ref, f32)).astype(f32)            # :341
        dist = norm3(PC)
        dmax = f32(dist * f32(level_scale))                         # :349
        dmin = f32(dmax / f32(top_scale))                           # :350
        normal = (normal / f32(len(Ows))).astype(f32)               # :351
    return normal, dmax, dmin


def update(problem, what: int = 3, reverse: bool = False):
    """Both functions over the batch.  Returns what rsc.engine.update_map_points_many returns; entries not written
    hold FILL.  reverse: every list is walked backwards (the order tests)."""
    kfs, u = problem.kfs, problem.upd
    n = int(u.n_points)
    out = dict(desc=np.full((n, 32), FILL["desc"], np.uint8), best_obs=np.full(n, FILL["best_obs"], np.int32),
               normal=np.full((n, 3), FILL["normal"], f32), dmax=np.full(n, FILL["dmax"], f32),
               dmin=np.full(n, FILL["dmin"], f32), updated=np.zeros(n, np.uint8))
    bad = np.zeros(len(kfs), np.uint8) if u.kf_bad is None else np.asarray(u.kf_bad, np.uint8)
    for p in range(n):
        obs = [(int(u.obs_kf[o]), int(u.obs_idx[o])) for o in range(int(u.obs_begin[p]), int(u.obs_begin[p + 1]))]
        if reverse:
            obs = obs[::-1]
        if u.skip[p] or not obs:                                    # :233, :238, :320, :327
            continue
        if what & 1:
            kept = [i for i, (k, _) in enumerate(obs) if not bad[k]]  # :247
            out["best_obs"][p] = -1
            if kept:                                                # :251
                b = kept[best_row([kfs[obs[i][0]].desc[obs[i][1]] for i in kept])]
                out["best_obs"][p] = b
                out["desc"][p] = kfs[obs[b][0]].desc[obs[b][1]]     # :287
                out["updated"][p] |= 1
        if what & 2:
            ref = kfs[int(u.ref_kf[p])]
            level = int(ref.octave[int(u.ref_idx[p])])              # :343
            out["normal"][p], out["dmax"][p], out["dmin"][p] = normal_and_depth(
                u.pos[p], [kfs[k].Ow for k, _ in obs], ref.Ow, ref.scale[level], ref.scale[len(ref.scale) - 1])
            out["updated"][p] |= 2
    return out


def same_floats(a, b) -> bool:
    """Bit for bit, but for NaNs: IEEE 754 leaves the sign and the payload of a NaN an operation produces to the
    implementation (x86 SSE gives 0/0 the sign bit, other hardware need not), so a NaN matches any NaN."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def same_result(got, want) -> str:
    """'' when two results agree (same_floats on the float fields), else the first field that differs."""
    for k in ("updated", "best_obs", "desc"):
        if not np.array_equal(got[k], want[k]):
            return k
    for k in ("normal", "dmax", "dmin"):
        if not same_floats(got[k], want[k]):
            return k
    return ""
