"""Writes tests/golden/stereo_traces.npz: the outputs of the sequential restatement (tests/stereo_ref.py) of
Frame::ComputeStereoMatches on the hand-built cases (tests/stereo_cases.py) and on the random frames of
stereo_cases.RANDOM_FRAMES.  The fixture keeps a digest of every random frame's inputs (sums of the coordinates,
octaves and descriptor bytes) so that a generator that drifted shows.  Run from the repository root:

    python tests/golden/make_stereo_golden.py

The asserts are the conditions the tests rely on, so that none of them can pass on empty results."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import stereo_cases as sc  # noqa: E402
import stereo_ref as sr  # noqa: E402

ARRAYS = ("u_right", "depth", "best_right", "best_dist")


def record(r):
    """The four scalars of a result as one float64 row (th_dist is a float32 and survives the trip)."""
    return np.array([r["n_candidates"], r["n_removed"], r["median"], float(r["th_dist"])], np.float64)


def main():
    d, names = {}, []
    for name, fr, exp in sc.cases():
        r = sr.compute(fr)
        assert sr.same(r, exp) == [], (name, sr.same(r, exp))
        for k in ARRAYS:
            d[f"{name}/{k}"] = r[k]
        d[f"{name}/result"] = record(r)
        names.append(name)
    total = dict(zero_disparity=0, tie_same_row=0, tie_other_row=0)
    for name, fr in sc.random_frames().items():
        r = sr.compute(fr)
        n = len(fr.kp)
        t = sc.traits(fr, r)
        for k in total:
            total[k] += t[k]
        if n >= 64:
            assert r["n_candidates"] >= 0.8 * n and 0.01 * r["n_candidates"] <= r["n_removed"] <= 0.5 * r["n_candidates"]
            assert r["n_candidates"] - r["n_removed"] >= 1
        for k in ARRAYS:
            d[f"{name}/{k}"] = r[k]
        d[f"{name}/result"] = record(r)
        d[f"{name}/digest"] = sc.digest(fr)
        print(name, "accepted", r["n_candidates"], "removed", r["n_removed"], "median", r["median"], t)
    assert all(v > 0 for v in total.values()), total
    d["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "stereo_traces.npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
