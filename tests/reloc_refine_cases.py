"""Entry states and events for Tracking::Relocalization's refinement chain (Tracking.cpp:1294-1323), shared
by the CPU and GPU tests (TEST-ONLY).  One scene (rsc.synth.make_reloc_refine_event); the branch a state
or event is meant to cover is asserted by the tests on the reference's own record."""
from __future__ import annotations

import functools
import types

import numpy as np

from rsc import synth


@functools.lru_cache(maxsize=None)
def scene():
    """(problem, candidates): candidate 0 = a KeyFrame that shares hundreds of MapPoints with the Frame
    and 35 correct + 10 wrong BoW matches; 1 = a KeyFrame with 30 shared MapPoints and 25 correct
    matches; 2 = 64 shared MapPoints, 25 correct + 3 wrong matches."""
    rng = np.random.default_rng(7)
    return synth.make_reloc_refine_event(rng, 600, 800, [(35, 10, None), (25, 0, 30), (25, 3, 64)])


def _entry(p, kf, n_entry):
    """mvpMapPoints = n_entry correct matches, sFound = their MapPoints."""
    good = np.nonzero(p.truth >= 0)[0]
    good = good[kf.mp_state[p.truth[good]] == 1][:n_entry]
    mp = np.full(p.frame.n, -1, np.int32)
    mp[good] = p.truth[good]
    found = np.zeros(kf.n, np.uint8)
    found[p.truth[good]] = 1
    return mp, found


def _rotated(T, angle):
    """The pose after a rotation of the camera about its y axis (a shift of ~435 * angle px)."""
    c, s = np.cos(angle), np.sin(angle)
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    out = np.eye(4)
    out[:3, :3] = Ry @ T[:3, :3]
    out[:3, 3] = Ry @ T[:3, 3]
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def chain_states():
    """stage1_short: few shared MapPoints, nadditional + nGood < 50.  stage1_only: the first search finds
    hundreds, the optimisation leaves nGood >= 50.  both_stages: 64 shared MapPoints and an entry pose 12 px
    off, so SearchByProjection(10, 100) misses the MapPoints of the two finest levels (radius 10 and 12 px),
    the optimisation on the rest gives 30 < nGood < 50 and SearchByProjection(3, 64) finds the missed ones
    with the corrected pose (n_good_in = 35 steers :1298)."""
    p, cs = scene()
    out = {}
    for name, c, n_good_in, rot in (("stage1_short", 1, 20, 0.0), ("stage1_only", 0, 20, 0.0),
                                    ("both_stages", 2, 35, 0.028)):
        kf = cs[c][0]
        mp, found = _entry(p, kf, 20)
        out[name] = types.SimpleNamespace(frame=p.frame, kf=kf, frame_mp=mp, found=found, n_good_in=n_good_in,
                                          Tcw_in=_rotated(p.Tcw_true, rot))
    return out


@functools.lru_cache(maxsize=None)
def events():
    """[(candidates [(kf, matches, scene)], seeds)] over the scene's Frame: event 0 = the first success
    has 10-49 good points and the chain lifts it to a match; event 1 = the chain on the first candidate
    fails and the next candidate matches; event 2 = no candidate reaches 50."""
    p, cs = scene()
    return p, [([cs[0]], [1]), ([cs[1], cs[0]], [2, 3]), ([cs[1]], [4])]
