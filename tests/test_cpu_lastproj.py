"""ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) (ORBmatcher.cpp:1173-1315), on the CPU:

* the sequential Python restatement (tests/lastproj_ref.py) against answers worked out by hand, one case per
  rule (tests/lastproj_cases.py);
* the host build of the kernels' per-point functions (tests/lastproj_emu): its literal sequential loop equals
  the restatement bit for bit, and the fixed-point rounds and table-based finish the kernel runs equal the
  sequential loop, on every case, the domino, the golden fixture and 200 seeded crowded problems;
* every rule switched off alone (lastproj_ref.PERTURBATIONS) changes the answer of some case; the two that
  cannot are proved unobservable instead;
* the generator reproduces the fixture, whose crowded problems meet the census conditions;
* the stand-alone program of the emulation, plain and under the host address / undefined-behaviour sanitizers.
Everything is compared bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lastproj_cases as lc
import lastproj_emu_lib as le
import lastproj_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_lastproj_golden as mk  # noqa: E402

CASES = lc.cases()
f32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "lastproj_traces.npz"))


def same(a, r, rounds=True):
    assert np.array_equal(a["out"], r["out"])
    assert a["nmatches"] == r["nmatches"] and a["mode"] == r["mode"]
    if rounds:
        assert a["rounds"] == r["rounds"], (a["rounds"], r["rounds"])


def check_emulation(p, r):
    same(le.search_sequential(p), r, rounds=False)
    fp = le.search_fixed_point(p)
    same(fp, r)
    return fp


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_known_answer(name):
    p, exp = CASES[name]
    keep = [a.copy() for a in (p.frame_occ, p.last.mp_state, p.last.mp_has_obs)]
    nmatches, out, mode = ref.search_by_projection_last(p)
    assert nmatches == exp["nmatches"]
    assert mode == exp["mode"]
    assert np.array_equal(out, lc.expected_out(p, exp))
    for a, b in zip((p.frame_occ, p.last.mp_state, p.last.mp_has_obs), keep):
        assert np.array_equal(a, b)


def test_reference_trace_by_hand():
    """reason codes, claims and bins of cases whose every slot can be followed by hand"""
    tr = {}
    ref.search_by_projection_last(CASES["depth_zero"][0], tr)
    assert tr["reason"].tolist() == [ref.BOUNDS, ref.BOUNDS, ref.NAN_PIXEL, ref.MATCHED]
    assert tr["claim"].tolist() == [-1, -1, -1, 1]
    ref.search_by_projection_last(CASES["depth_negative"][0], tr)
    assert tr["reason"].tolist() == [ref.DEPTH, ref.MATCHED]
    ref.search_by_projection_last(CASES["skipped_slots"][0], tr)
    assert tr["reason"].tolist() == [ref.OUTLIER, ref.NO_POINT, ref.MATCHED]
    ref.search_by_projection_last(CASES["cutoff"][0], tr)
    assert tr["reason"].tolist() == [ref.MATCHED, ref.ABOVE_TH]
    ref.search_by_projection_last(CASES["entry_with_obs"][0], tr)
    assert tr["reason"].tolist() == [ref.MATCHED] and tr["claim"].tolist() == [1]
    ref.search_by_projection_last(CASES["levels_backward_o0"][0], tr)
    assert tr["reason"].tolist() == [ref.MATCHED, ref.NO_FREE, ref.NO_FREE]
    ref.search_by_projection_last(CASES["bound_outside"][0], tr)
    assert tr["reason"].tolist() == [ref.BOUNDS] * 4
    ref.search_by_projection_last(CASES["first_claimer_removed"][0], tr)
    assert tr["claim"].tolist() == list(range(12)) + [12, 12]
    assert tr["bin"].tolist() == [0] * 12 + [3, 0] and tr["claimers"][12] == 2
    ref.search_by_projection_last(CASES["rot_wrap"][0], tr)
    assert tr["bin"].tolist() == [0] * 12 + [1, 1, 5, 5, 11, 11]


def test_mode_arithmetic():
    """tlc.z with a general pose: the emulation's float arithmetic equals the restatement's, sums left to right"""
    rng = np.random.default_rng(5)
    from rsc import synth
    for _ in range(200):
        Tc, Tl = np.eye(4, dtype=f32), np.eye(4, dtype=f32)
        Tc[:3, :3], Tl[:3, :3] = synth.random_rotation(rng), synth.random_rotation(rng)
        Tc[:3, 3], Tl[:3, 3] = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
        mb = float(f32(rng.uniform(0, 0.6)))
        assert le.lib().lse_mode(np.ascontiguousarray(Tc).reshape(-1), np.ascontiguousarray(Tl).reshape(-1), mb) == \
            ref.level_mode(Tc, Tl, mb)


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulation_equals_reference(name):
    p, _ = CASES[name]
    check_emulation(p, lc.reference(p))


def test_domino_takes_k_plus_one_rounds():
    p, exp = lc.domino(40)
    r = lc.reference(p)
    assert np.array_equal(r["out"], lc.expected_out(p, exp)) and r["nmatches"] == 40
    assert r["rounds"] == 41
    assert not np.array_equal(r["round1"], r["out"])      # one round is not enough
    assert check_emulation(p, r)["rounds"] == 41


def test_fixture_is_reproducible_and_emulation_matches(golden):
    ps = mk.problems()
    assert list(golden["names"]) == list(ps)
    for n, p in ps.items():
        q = lc.from_arrays(golden, n)
        for k, a in lc.to_arrays(p, n).items():
            assert np.array_equal(golden[k], a), k
        nm, mode, rounds = (int(v) for v in golden[f"{n}/counts"])
        r = dict(out=golden[f"{n}/out"], nmatches=nm, mode=mode, rounds=rounds)
        fp = check_emulation(q, r)
        if n in lc.RANDOM:
            cs = dict(zip(golden["counters"], golden[f"{n}/census"]))
            for k, lo in mk.CONDITIONS.items():
                assert cs[k] >= lo, (n, k, cs[k])
            assert fp["walks"] >= 1 and mode == lc.RANDOM[n][2]


@pytest.mark.parametrize("name", sorted(lc.RANDOM))
def test_random_problem_reference_and_census(golden, name):
    """the restatement, run here, gives the fixture's answer and the census conditions on the inputs"""
    p = lc.from_arrays(golden, name)
    tr = {}
    r = lc.reference(p, tr)
    assert np.array_equal(r["out"], golden[f"{name}/out"])
    assert [r["nmatches"], r["mode"], r["rounds"]] == golden[f"{name}/counts"].tolist()
    assert np.array_equal(tr["claim"], golden[f"{name}/claim"])
    cs = mk.census(p, r, tr)
    for k, lo in mk.CONDITIONS.items():
        assert cs[k] >= lo, (k, cs[k])
    # nmatches counts claims, not slots: the two differ on these inputs
    assert r["nmatches"] != int((r["out"] >= 0).sum())


def test_rounds_equal_sequential_on_seeded_problems():
    """200 small crowded problems over the three modes and both thresholds: kernel rounds == literal loop"""
    walks = nulled = 0
    for s in range(200):
        p = lc.random_problem(1000 + s, (7.0, 15.0)[s % 2], s % 3, n_frame=150, n_last=300, n_clusters=10,
                              cluster_kps=6, cluster_slots=14)
        a, b = le.search_sequential(p), le.search_fixed_point(p)
        assert np.array_equal(a["out"], b["out"]), s
        assert (a["nmatches"], a["mode"], a["claims"]) == (b["nmatches"], b["mode"], b["claims"]), s
        assert a["mode"] == s % 3
        walks += b["walks"]
        nulled += int((a["out"] == -2).sum())
    assert walks > 0 and nulled > 0


def _changed(p, base, off):
    n, out, _ = ref.search_by_projection_last(p, off=(off,))
    return n != base[0] or not np.array_equal(out, base[1])


def test_every_perturbation_changes_some_case():
    base = {n: ref.search_by_projection_last(p)[:2] for n, (p, _) in CASES.items()}
    for pert in ref.PERTURBATIONS:
        hits = [n for n, (p, _) in CASES.items() if _changed(p, base[n], pert)]
        if pert in ref.UNOBSERVABLE:
            assert not hits, (pert, hits)
        else:
            assert hits, pert


def test_unobservable_perturbations_are_proved():
    """invzc <= 0 and the float division cannot differ from the reference on defined inputs"""
    fmax = np.finfo(f32).max
    assert f32(1.0 / np.float64(fmax)) > 0 and f32(f32(1.0) / fmax) > 0          # invzc == 0 needs z = inf
    with np.errstate(invalid="ignore"):
        assert np.isnan(f32(0.0) * f32(np.inf)) and np.isnan(f32(f32(100.0) * f32(np.inf)) * f32(0.0))
    m = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3F800000)).view(f32)  # every significand in [1, 2)
    assert np.array_equal((1.0 / m.astype(np.float64)).astype(f32), f32(1.0) / m)


@pytest.mark.parametrize("exe", [le.MAIN, le.MAIN_SAN])
def test_standalone_program(exe):
    le.build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["mismatches"] == 0 and rec["nmatches"] > 600 and rec["fallback_walks"] > 0 and rec["nulled"] > 0
    assert rec["rounds"] >= 18        # six passes of at least three rounds
