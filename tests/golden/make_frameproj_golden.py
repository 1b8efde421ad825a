"""Writes tests/golden/frameproj_traces.npz: the inputs of the hand-built SearchByProjection cases
(tests/frameproj_cases.py), the domino and two random crowded problems, each with the output of the
sequential Python reference (tests/frameproj_ref.py).  Run from the repository root:
    python tests/golden/make_frameproj_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

import frameproj_cases as fc  # noqa: E402
import frameproj_ref as fr  # noqa: E402


def problems():
    out = {name: p for name, (p, _) in fc.cases().items()}
    out["domino"] = fc.domino()[0]
    out["random_coarse"] = fc.random_problem(101, 150, 220, 10, 100, n_clusters=4)
    out["random_fine"] = fc.random_problem(102, 150, 220, 3, 64, n_clusters=4)
    return out


def main():
    d = {}
    names = []
    for name, p in problems().items():
        n, out = fr.search_by_projection(p.frame, p.kf, p.Tcw, p.already, p.frame_mp, p.th, p.orb_dist,
                                         p.check_orientation)
        d.update(fc.to_arrays(p, name))
        d[f"{name}/out"] = out
        d[f"{name}/nmatches"] = np.int32(n)
        names.append(name)
    d["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "frameproj_traces.npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "bytes,", len(names), "problems")


if __name__ == "__main__":
    main()
