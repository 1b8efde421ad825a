"""Problems that fill the rounds loop's walk list (proj_rounds, rsc_projrounds.h: walk[kProjWalkCap]) to its
capacity and beyond (TEST-ONLY), for the two matchers that list their walkers (kCoopWalk): the local-map matcher
(localproj.hip) and the last-frame matcher (lastproj.hip).  Built with the helpers of localproj_cases.py and
lastproj_cases.py; shared by tests/test_cpu_walk_list.py (which proves each case's condition from the
emulation) and tests/test_gpu_walk_list.py.

The construction: N identical points at (0, 0, 2), which project to (300, 200), and 12 features within 1 px of
that projection whose descriptors are at distances 3 + 5 k (k = 0..11) from the points' all-zero descriptor.
Every point caches the same four nearest features and the list was longer (kProjMore), so once the lower points
hold enough of the four, every later point walks its window in every round.

local-map matcher, all features at octave 0, every point with observations ("vetoed"): point k < 4 ends on
feature k (3 <= 0.8 * 8, 8 <= 0.8 * 13, 13 <= 0.8 * 18, 18 <= 0.8 * 23 = 18.4); every later point sees 23 and 28
free, 23 > 0.8f * 28 = 22.4: vetoed, -1.  Rounds 1-3 are answered from the cache (two of the four free); from
round 4 on fewer than two cached features are free for the points >= 3: N - 3 walkers in rounds 4, 5 and 6
(point 3 itself has one free cached feature, its own).  6 rounds, nmatches 4.

local-map matcher, octaves alternating 0 / 1 and points at level 1 ("features"): the best and the runner-up
are always at different levels, so the ratio veto never applies.  The first eight points have observations and
end on features 0..7; the others have none, block nobody, and all end on feature 8, the best free one: the
walkers' decisions are features.  N - 3 walkers in rounds 4..10, 10 rounds, nmatches N.

last-frame matcher (first free minimum, no veto), 8 features: slot k < 8 ends on feature k, the others on none;
from round 5 on all four cached features are held by lower slots for the slots >= 4: N - 4 walkers.  In the
"features" form the slots from 6 on have no observations and all end on feature 6; their angles spread over four
rotation bins of which the smallest is removed, which nulls feature 6 (the per-entry removal).
"""
from __future__ import annotations

import functools
import os
import re

import lastproj_cases as sc
import localproj_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def walk_cap() -> int:
    """kProjWalkCap as rsc_projrounds.h states it."""
    src = open(os.path.join(ROOT, "orb-slam2-optimized_amd", "csrc", "rsc_projrounds.h")).read()
    m = re.search(r"constexpr\s+int\s+kProjWalkCap\s*=\s*(\d+)\s*;", src)
    assert m, "kProjWalkCap not found in rsc_projrounds.h"
    return int(m.group(1))


N_FEATURES = 12
LOCAL_STATIC = 3   # points that never walk in the local-map construction: walkers = N - 3
LAST_FEATURES = 8
LAST_STATIC = 4    # slots that never walk in the last-frame construction: walkers = N - 4
# walkers in one round, relative to the cap -> the condition test_cpu_walk_list.py proves
EXCESS = {"at_cap": 0, "cap_plus_1": 1, "overflow": 101}  # overflow: 4,200 points for a cap of 4,096


def _u(k):
    return 299.6 + 0.07 * k  # within 1 px of u = 300, distinct, in visiting order


def local_vetoed(n_points: int):
    pts = [lc.pt(0.0, 0.0, 2.0) for _ in range(n_points)]
    fts = [lc.ft(_u(k), 200.0, 3 + 5 * k) for k in range(N_FEATURES)]
    return lc.build(pts, fts)


def local_features(n_points: int):
    pts = [lc.pt(0.0, 0.0, 2.0, level=1, has_obs=1 if i < 8 else 0) for i in range(n_points)]
    fts = [lc.ft(_u(k), 200.0, 3 + 5 * k, octave=k % 2) for k in range(N_FEATURES)]
    return lc.build(pts, fts)


def last_plain(n_slots: int):
    slots = [sc.sl(0.0, 0.0, 2.0) for _ in range(n_slots)]
    fts = [sc.ft(_u(k), 200.0, 3 + 5 * k) for k in range(LAST_FEATURES)]
    return sc.build(slots, fts)


def last_features(n_slots: int):
    def angle(i):
        if i < 6:
            return 0.0
        if i % 97 == 0:
            return 90.0   # bin 3: about 1 % of the claims, removed
        return 30.0 * (i % 3)  # bins 0, 1, 2: kept
    slots = [sc.sl(0.0, 0.0, 2.0, has_obs=1 if i < 6 else 0, angle=angle(i)) for i in range(n_slots)]
    fts = [sc.ft(_u(k), 200.0, 3 + 5 * k) for k in range(LAST_FEATURES)]
    return sc.build(slots, fts)


@functools.lru_cache(maxsize=None)
def local_cases():
    """name -> (problem, walkers in the fullest round relative to the cap)."""
    cap = walk_cap()
    c = {f"vetoed_{k}": (local_vetoed(cap + e + LOCAL_STATIC), e) for k, e in EXCESS.items()}
    c["features_overflow"] = (local_features(cap + EXCESS["overflow"] + LOCAL_STATIC), EXCESS["overflow"])
    return c


@functools.lru_cache(maxsize=None)
def last_cases():
    cap = walk_cap()
    c = {f"plain_{k}": (last_plain(cap + e + LAST_STATIC), e) for k, e in EXCESS.items()}
    c["features_overflow"] = (last_features(cap + EXCESS["overflow"] + LAST_STATIC), EXCESS["overflow"])
    return c


_refs = {}


def reference(kind: str, name: str):
    """The sequential restatement's answer for a case (kind: "local" or "last"), computed once per process."""
    if (kind, name) not in _refs:
        p = (local_cases() if kind == "local" else last_cases())[name][0]
        _refs[kind, name] = (lc if kind == "local" else sc).reference(p)
    return _refs[kind, name]


def local_regular():
    """The two regular problems a walk-list case stands between in a batch (th = 1, as the cases)."""
    cs = lc.cases()
    return [cs["promoted"][0], cs["veto_lifted"][0]]


def last_regular():
    cs = sc.cases()
    return [cs["greedy_promoted"][0], cs["two_claimers_kept"][0]]
