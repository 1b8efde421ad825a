"""Writes tests/golden/localproj_traces.npz from the Python restatement only (tests/localproj_ref.py): the
hand-built cases, the domino and the two crowded random problems of tests/localproj_cases.py with the
restatement's out, track, nmatches, n_to_match, rounds and round-1 answer.  The crowded problems must show
every branch of the matcher often enough (CONDITIONS); the seeds in localproj_cases.RANDOM were chosen so
that they do.

    python tests/golden/make_localproj_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import localproj_cases as lc  # noqa: E402

# per crowded problem, in the restatement's trace
CONDITIONS = dict(matches=100, vetoes=10, promoted=10, lifted=10, overwrites=10, stereo=10)
COUNTERS = tuple(CONDITIONS)


def problems():
    """name -> problem, in fixture order."""
    ps = {n: p for n, (p, _) in lc.cases().items()}
    ps["domino"] = lc.domino()[0]
    for n, (seed, th) in lc.RANDOM.items():
        ps[n] = lc.random_problem(seed, th)
    return ps


def build() -> dict:
    d = {}
    names = []
    for n, p in problems().items():
        trace = {}
        r = lc.reference(p, trace)
        d.update(lc.to_arrays(p, n))
        d[f"{n}/out"] = r["out"]
        d[f"{n}/track"] = r["track"]
        d[f"{n}/counts"] = np.array([r["nmatches"], r["n_to_match"], r["rounds"]], np.int32)
        d[f"{n}/round1"] = r["round1"]
        d[f"{n}/trace"] = np.array([trace.get(k, 0) for k in COUNTERS], np.int32)
        names.append(n)
        if n in lc.RANDOM:
            for k, lo in CONDITIONS.items():
                assert trace[k] >= lo, f"{n}: {k} = {trace[k]} < {lo}"
    d["names"] = np.array(names)
    d["counters"] = np.array(COUNTERS)
    return d


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "localproj_traces.npz")
    np.savez_compressed(out, **build())
    print(out, os.path.getsize(out), "bytes")
