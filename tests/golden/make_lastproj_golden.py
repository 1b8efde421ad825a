"""Writes tests/golden/lastproj_traces.npz from the Python restatement only (tests/lastproj_ref.py): the
hand-built cases, the domino and the crowded random problems of tests/lastproj_cases.py with the restatement's
out, nmatches, mode, rounds, round-1 answer and census.  The crowded problems must show every branch of the
matcher often enough (CONDITIONS); the seeds in lastproj_cases.RANDOM were chosen so that they do.

    python tests/golden/make_lastproj_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lastproj_cases as lc  # noqa: E402

# per crowded problem, from the restatement's trace: matches; features with two or more claimers; features set
# to nullptr although their last claimer's bin was kept; rounds; slots that exhaust their four cached
# candidates and walk their window again
CONDITIONS = dict(nmatches=100, multi_claimed=5, nulled_surviving=1, rounds=3, walked=1)
COUNTERS = tuple(CONDITIONS)


def census(p, r, trace) -> dict:
    claim, bins, out = trace["claim"], trace["bin"], r["out"]
    last_writer = np.full(p.frame.n, -1, np.int64)
    for i in np.nonzero(claim >= 0)[0]:
        last_writer[claim[i]] = i
    kept_bins = {int(bins[last_writer[f]]) for f in np.nonzero(out >= 0)[0]}   # a kept feature's claimers are kept
    return dict(nmatches=int(r["nmatches"]), multi_claimed=int((trace["claimers"] >= 2).sum()),
                nulled_surviving=sum(1 for f in np.nonzero(out == -2)[0] if int(bins[last_writer[f]]) in kept_bins),
                rounds=int(r["rounds"]), walked=len(trace["walked"]))


def problems():
    """name -> problem, in fixture order."""
    ps = {n: p for n, (p, _) in lc.cases().items()}
    ps["domino"] = lc.domino()[0]
    for n, (seed, th, mode) in lc.RANDOM.items():
        ps[n] = lc.random_problem(seed, th, mode)
    return ps


def build() -> dict:
    d = {}
    names = []
    for n, p in problems().items():
        trace = {}
        r = lc.reference(p, trace)
        d.update(lc.to_arrays(p, n))
        d[f"{n}/out"] = r["out"]
        d[f"{n}/counts"] = np.array([r["nmatches"], r["mode"], r["rounds"]], np.int32)
        d[f"{n}/round1"] = r["round1"]
        d[f"{n}/reason"] = trace["reason"].astype(np.int8)
        d[f"{n}/claim"] = trace["claim"]
        d[f"{n}/bin"] = trace["bin"].astype(np.int8)
        cs = census(p, r, trace)
        d[f"{n}/census"] = np.array([cs[k] for k in COUNTERS], np.int32)
        names.append(n)
        if n in lc.RANDOM:
            for k, lo in CONDITIONS.items():
                assert cs[k] >= lo, f"{n}: {k} = {cs[k]} < {lo}"
            assert r["mode"] == lc.RANDOM[n][2]
    d["names"] = np.array(names)
    d["counters"] = np.array(COUNTERS)
    return d


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "lastproj_traces.npz")
    np.savez_compressed(out, **build())
    print(out, os.path.getsize(out), "bytes")
