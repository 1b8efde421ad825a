"""Writes tests/golden/mpupdate_traces.npz: the outputs of the sequential restatement (tests/mpupdate_ref.py) of
MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (what = 3) on the hand-built cases
(tests/mpupdate_cases.py) and on the two random problems of mpupdate_cases.RANDOM_SEEDS (four KeyFrames of 1,100
keypoints, lists of 1, 2, 3, 63, 64, 65, 200 and 1,024 observations and a few short ones).  The fixture keeps the
random problems' positions and observation indices so that a generator that drifted shows.  Run from the repository
root:

    python tests/golden/make_mpupdate_golden.py

The asserts are the conditions the tests rely on, so that none of them can pass on empty results."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import mpupdate_cases as mc  # noqa: E402
import mpupdate_ref as mr  # noqa: E402

FIELDS = ("desc", "best_obs", "normal", "dmax", "dmin", "updated")


def main():
    d, names = {}, []
    for name, (p, exp) in sorted(mc.cases().items()):
        r = mr.update(p, 3)
        want = [mr.FILL["best_obs"] if b is None else b for b in exp["best_obs"]]
        assert r["best_obs"].tolist() == want, (name, r["best_obs"].tolist(), want)
        for k in FIELDS:
            d[f"{name}/{k}"] = r[k]
        names.append(name)
    for name, seed in sorted(mc.RANDOM_SEEDS.items()):
        p = mc.random_problem(seed)
        r = mr.update(p, 3)
        sizes = np.diff(p.upd.obs_begin).tolist()
        assert sizes[:len(mc.RANDOM_SIZES)] == list(mc.RANDOM_SIZES)
        assert ((r["updated"] & 2) == 2).all() and (r["updated"] == 3).sum() >= 10 and np.isfinite(r["normal"]).all()
        assert len(set(r["best_obs"].tolist())) > 4  # not all the first row
        d[f"{name}/pos"] = p.upd.pos
        d[f"{name}/obs_idx"] = p.upd.obs_idx
        for k in FIELDS:
            d[f"{name}/{k}"] = r[k]
        print(name, "best_obs", r["best_obs"].tolist())
    d["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "mpupdate_traces.npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
