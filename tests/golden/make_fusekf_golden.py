"""Writes tests/golden/fusekf_traces.npz: the outputs of the sequential restatement (tests/fusekf_ref.py) of
ORBmatcher::Fuse(pKF, vpMapPoints, th) on the hand-built cases (tests/fusekf_cases.py) and on two random crowded
problems (KeyFrame n = 600 with 30 % stereo keypoints, 1,500 points, three target poses each).  The inputs are
drawn from the seeds of fusekf_cases.RANDOM_SEEDS; the fixture keeps the points' positions so that a generator that
drifted shows.  Run from the repository root:

    python tests/golden/make_fusekf_golden.py

The asserts are the conditions the tests rely on, so that none of them can pass on empty results."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import fusekf_cases as fc  # noqa: E402
import fusekf_ref as fr  # noqa: E402


def main():
    d, names = {}, []
    for name, (p, exp) in sorted(fc.cases().items()):
        best = fr.fuse_kf(p.kf, p.pts, p.skip, p.th)
        assert best.tolist() == exp, (name, best.tolist(), exp)
        d[f"{name}/best_idx"] = best
        names.append(name)
    for name, seed in sorted(fc.RANDOM_SEEDS.items()):
        pts, kfs, skips = fc.random_problem(seed)
        d[f"{name}/pt_pos"] = pts.pos
        for k, (kf, skip) in enumerate(zip(kfs, skips)):
            st = {}
            best = fr.fuse_kf(kf, pts, skip, fc.TH, st)
            n = int((best >= 0).sum())
            assert n >= 100, (name, k, n)
            assert st["level"] >= 1 and st["stereo"] >= 1 and st["mono"] >= 1, (name, k, st)
            d[f"{name}/{k}/best_idx"] = best
            d[f"{name}/{k}/stats"] = np.array([st[s] for s in ("level", "stereo", "mono", "windows", "largest")],
                                              np.int32)
            print(f"{name}/{k}: nfused {n} {st}")
    d["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "fusekf_traces.npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
