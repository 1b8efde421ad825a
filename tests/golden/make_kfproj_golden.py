"""Writes tests/golden/kfproj_traces.npz: the hand-built cases, the domino and two random crowded problems
(KeyFrame n = 600, 1,500 points) of the loop-closing SearchByProjection with the outputs of the sequential
restatement (tests/kfproj_ref.py), the round count of its fixed-point restatement, and a Fuse batch of five
KeyFrames against the first random point set.  Run from the repository root:

    python tests/golden/make_kfproj_golden.py

The asserts are the conditions the tests rely on, so that none of them can pass on empty results."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import kfproj_cases as kc  # noqa: E402
import kfproj_ref as kr  # noqa: E402


def record(d, name, p, random=False):
    tr = {}
    n, out = kr.search_by_projection_kf(p.kf, p.pts, p.Scw, p.already, p.occupied, p.th, tr)
    claim, rounds, exhausted = kr.fixed_point_rounds(p.kf, p.pts, p.Scw, p.already, p.occupied, p.th)
    assert np.array_equal(claim, tr["claim"]), name  # the fixed point is the sequential result
    moved = int((tr["claim"] != tr["free_best"]).sum())
    if random:
        assert n >= 100, (name, n)
        assert moved >= 10, (name, moved)
        assert exhausted >= 1, (name, exhausted)
    d.update(kc.to_arrays(p, name))
    d[f"{name}/out"] = out
    d[f"{name}/nmatches"] = np.array([n], np.int32)
    d[f"{name}/rounds"] = np.array([rounds], np.int32)
    d[f"{name}/round1"] = tr["free_best"]
    print(f"{name}: nmatches {n} rounds {rounds} moved {moved} exhausted {exhausted}")


def main():
    d, names = {}, []
    for name, (p, exp) in sorted(kc.cases().items()):
        record(d, name, p)
        assert np.array_equal(d[f"{name}/out"], kc.expected_out(p, exp)), name
        names.append(name)
    p, exp = kc.domino(40)
    record(d, "domino", p)
    assert int(d["domino/rounds"][0]) == 41 and np.array_equal(d["domino/out"], kc.expected_out(p, exp))
    round1 = np.full(p.kf.n, -1, np.int32)  # what one round alone would give: the lowest claimant per keypoint
    for i in range(p.pts.n - 1, -1, -1):
        if d["domino/round1"][i] >= 0:
            round1[d["domino/round1"][i]] = i
    assert not np.array_equal(round1, d["domino/out"])
    names.append("domino")
    for name, seed in sorted(kc.RANDOM_SEEDS.items()):
        record(d, name, kc.random_problem(seed), random=True)
        names.append(name)
    # Fuse: five KeyFrames against the point set of random_a
    p = kc.random_problem(kc.RANDOM_SEEDS["random_a"])
    batch = kc.fuse_batch(p)
    res = [kr.fuse(kf, p.pts, S, ik, 4.0) for kf, S, ik in batch]
    assert all(r["nfused"] >= 100 for r in res), [r["nfused"] for r in res]
    assert any((r["replace"] >= 0).sum() >= 10 and (r["added"] >= 0).sum() >= 10 for r in res)
    d["fuse/Scw"] = np.stack([S for _, S, _ in batch])
    d["fuse/in_kf"] = np.stack([ik for _, _, ik in batch])
    d["fuse/mp_state"] = np.stack([kf.mp_state for kf, _, _ in batch])
    d["fuse/best_idx"] = np.stack([r["best_idx"] for r in res])
    d["fuse/replace"] = np.stack([r["replace"] for r in res])
    d["fuse/added"] = np.stack([r["added"] for r in res])
    d["fuse/holder"] = np.stack([r["holder"] for r in res])
    assert all((r["holder"] >= 0).sum() >= 1 for r in res)  # a slot filled and found again within one call
    d["fuse/nfused"] = np.array([r["nfused"] for r in res], np.int32)
    d["fuse/th"] = np.array([4.0], np.float32)
    print("fuse: nfused", d["fuse/nfused"].tolist())
    d["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "kfproj_traces.npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
