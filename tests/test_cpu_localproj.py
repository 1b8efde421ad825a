"""Tracking::SearchLocalPoints (Tracking.cpp:1003-1028) = Frame::isInFrustum (Frame.cpp:336-392) and
ORBmatcher::SearchByProjection(Frame&, vector<MapPoint>&, th) (ORBmatcher.cpp:16-100), on the CPU:

* the sequential Python restatement (tests/localproj_ref.py) against answers worked out by hand, one case per
  rule (tests/localproj_cases.py);
* the host build of the kernels' per-point functions (tests/localproj_emu): its sequential loop and the
  fixed-point rounds the kernel runs equal the restatement on every case and on the golden fixture, in fused
  and in matcher-only mode: out, track, nmatches, n_to_match and rounds;
* the streaming best / second-best update equals "the two smallest under (distance, visiting order)", by brute
  force over all sequences of length <= 5;
* the largest runner-up distance that vetoes any best <= TH_HIGH, by enumeration of the 257 x 257 grid, and
  the candidate cache's cutoff derived from it;
* the generator reproduces the fixture, whose crowded problems show every branch often enough;
* the stand-alone program of the emulation, plain and under the host address / undefined-behaviour sanitizers.
Everything is compared bit for bit."""
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import localproj_cases as lc
import localproj_emu_lib as le
import localproj_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = lc.cases()
f32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "localproj_traces.npz"))


def same(a, ref, rounds=True):
    assert np.array_equal(a["out"], ref["out"])
    assert a["track"].tobytes() == np.ascontiguousarray(ref["track"], lr.TRACK).tobytes()
    assert a["nmatches"] == ref["nmatches"] and a["n_to_match"] == ref["n_to_match"]
    if rounds:
        assert a["rounds"] == ref["rounds"], (a["rounds"], ref["rounds"])


def check_emulation(p, ref):
    """fused: sequential loop and rounds == restatement; matcher-only on the restatement's records: the same"""
    same(le.search_sequential(p), ref, rounds=False)
    fp = le.search_fixed_point(p)
    same(fp, ref)
    same(le.search_sequential(p, ref["track"]), ref, rounds=False)
    same(le.search_fixed_point(p, ref["track"]), ref)
    return fp


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_known_answer(name):
    p, exp = CASES[name]
    keep = [a.copy() for a in (p.skip, p.has_obs, p.frame_occ)]
    r = lr.search_local_points(p.frame, p.pts, p.Tcw, p.skip, p.has_obs, p.frame_occ, p.cos_limit, p.th, p.nn_ratio)
    assert r["nmatches"] == exp["nmatches"]
    assert np.array_equal(r["out"], lc.expected_out(p, exp))
    assert r["track"]["in_view"].tolist() == exp["in_view"]
    assert r["n_to_match"] == sum(exp["in_view"])
    for a, b in zip((p.skip, p.has_obs, p.frame_occ), keep):
        assert np.array_equal(a, b)


def test_reference_track_record_by_hand():
    """(1, 0, 1) at level 0: u = 400, v = 200, xr = 400 - 40 = 360, viewCos = 2 / sqrt(2) (normal = the point);
    (0, 0, 1) with normal (0, 0, (float)0.998): viewCos = that float, radius 2.5 under the double compare."""
    p, _ = CASES["z_negative"]
    tr, n = lr.frustum_all(p.frame, p.pts, p.Tcw, p.skip, p.cos_limit)
    assert n == 1 and tr[0]["in_view"] == 0
    s2 = f32(np.sqrt(f32(2.0)))
    assert tuple(tr[1]) == (1, f32(400.0), f32(200.0), f32(360.0), 0, f32(f32(2.0) / s2))
    p, _ = CASES["radius_double_compare"]
    tr, _ = lr.frustum_all(p.frame, p.pts, p.Tcw, p.skip, p.cos_limit)
    assert tr[0]["view_cos"] == f32(0.998) and float(f32(0.998)) > 0.998
    assert lr.radius_by_viewing_cos(tr[0]["view_cos"]) == 2.5 == le.lib().lpe_radius(float(f32(0.998)))
    below = np.nextafter(f32(0.998), f32(0))
    assert lr.radius_by_viewing_cos(below) == 4.0 == le.lib().lpe_radius(float(below))


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulation_matches_reference_on_cases(name):
    p, _ = CASES[name]
    check_emulation(p, lc.reference(p))


def test_domino_needs_41_rounds():
    p, exp = lc.domino()
    ref = lc.reference(p)
    assert np.array_equal(ref["out"], lc.expected_out(p, exp)) and ref["nmatches"] == 40
    assert ref["rounds"] == 41
    assert not np.array_equal(ref["round1"], ref["out"])  # round 1 alone gives another answer
    check_emulation(p, ref)


def test_emulation_matches_fixture(golden):
    """Every problem of the fixture: out, track, nmatches, n_to_match, rounds, both modes."""
    walks = 0
    for n in (str(s) for s in golden["names"]):
        p = lc.from_arrays(golden, n)
        c = golden[f"{n}/counts"]
        ref = dict(out=golden[f"{n}/out"], track=golden[f"{n}/track"], nmatches=int(c[0]), n_to_match=int(c[1]),
                   rounds=int(c[2]))
        walks += check_emulation(p, ref)["walks"]
    assert walks > 0  # the fallback walk of the window is exercised


def test_crowded_problems_show_every_branch(golden):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_localproj_golden as mg
    counters = [str(s) for s in golden["counters"]]
    for n in lc.RANDOM:
        p = lc.from_arrays(golden, n)
        assert p.frame.n == 600 and p.pts.n == 1500
        got = dict(zip(counters, (int(v) for v in golden[f"{n}/trace"])))
        for k, lo in mg.CONDITIONS.items():
            assert got[k] >= lo, (n, k, got[k])
        frac_no_obs = 1.0 - p.has_obs.mean()
        frac_mono = (p.frame.u_right < 0).mean()
        assert 0.2 < frac_no_obs < 0.4 and 0.2 < frac_mono < 0.45
        assert (p.frame_occ == 1).sum() >= 10 and (p.frame_occ == 2).sum() >= 10


def test_generator_reproduces_fixture(golden):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_localproj_golden as mg
    d = mg.build()
    assert sorted(d) == sorted(golden.files)
    for k in d:
        a, b = np.asarray(d[k]), golden[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_streaming_top2_is_two_smallest_in_order():
    """ORBmatcher.cpp:73-85 (`<` for the best, `else if <` for the second) over every sequence of length <= 5
    with distances in a 3-value set and a level per position: the best is the first minimum, the runner-up the
    smallest of the rest under (distance, position); bestLevel2 = -1 and bestDist2 = 256 when there is none."""
    seqs = 0
    for n in range(0, 6):
        for ds in itertools.product((10, 20, 30), repeat=n):
            levels = list(range(n))  # distinct, so the level identifies the position
            order = sorted(range(n), key=lambda k: (ds[k], k))
            b = order[0] if n >= 1 else None
            s = order[1] if n >= 2 else None
            exp = (ds[b] if n >= 1 else 256, levels[b] if n >= 1 else -1, ds[s] if n >= 2 else 256,
                   levels[s] if n >= 2 else -1, b if n >= 1 else -1)
            assert le.top2(ds, levels) == exp, (ds, le.top2(ds, levels), exp)
            # and the restatement's own loop
            bd, bl, bd2, bl2, bi = 256, -1, 256, -1, -1
            for k in range(n):
                if ds[k] < bd:
                    bd2, bd, bl2, bl, bi = bd, ds[k], bl, levels[k], k
                elif ds[k] < bd2:
                    bl2, bd2 = levels[k], ds[k]
            assert (bd, bl, bd2, bl2, bi) == exp
            seqs += 1
    assert seqs == sum(3 ** n for n in range(6))


def test_cutoff_bound_by_enumeration():
    """The veto `bestDist > 0.8f * bestDist2` (int against a float product) over the whole 257 x 257 grid: the
    largest runner-up that vetoes some best <= 100 is 124 (0.8f * 125 = 100.0000015 rounds to 100.0f, and 100 >
    100.0f is false), so a cache that keeps candidates up to 124 loses no veto; TH_HIGH alone would."""
    r = f32(0.8)
    veto = np.zeros((257, 257), bool)
    for b in range(257):
        for s in range(257):
            veto[b, s] = f32(b) > f32(r * f32(s))
    can_veto = [s for s in range(257) if veto[:101, s].any()]
    assert max(can_veto) == 124 and can_veto == list(range(125))  # downward closed
    assert not veto[100, 125] and veto[100, 124]
    assert 100.0 > 0.8 * 124 and float(f32(r * f32(125.0))) == 100.0
    L = le.lib()
    assert L.lpe_veto_bound(0.8) == 124 and L.lpe_keep_max(0.8) == 124
    for b in range(257):
        for s in range(0, 257, 1):
            # same level: accepted iff within the cutoff and not vetoed; other levels: the cutoff alone
            assert L.lpe_accepts(b, 3, s, 3, 0.8) == int(b <= 100 and not veto[b, s])
        assert L.lpe_accepts(b, 3, 0, 2, 0.8) == int(b <= 100)
    # other ratios: the bound is the largest s with 100 > ratio * s, never below TH_HIGH for the cache
    for ratio in (0.0, 0.39, 0.6, 0.75, 0.9, 1.0, 2.0):
        ok = [s for s in range(257) if f32(100.0) > f32(f32(ratio) * f32(s))]
        assert L.lpe_veto_bound(ratio) == (max(ok) if ok else -1)
        assert L.lpe_keep_max(ratio) == max(100, max(ok) if ok else -1)


def test_standalone_program_plain_and_sanitized():
    le.lib()
    outs = []
    for exe in ("localproj_emu_main", "localproj_emu_main_san"):
        r = subprocess.run([os.path.join(le.DIR, "build", exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(json.loads(r.stdout))
    assert outs[0] == outs[1]
    assert outs[0]["mismatches"] == 0 and outs[0]["nmatches"] >= 100 and outs[0]["fallback_walks"] > 0
