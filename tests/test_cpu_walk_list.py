"""The walk-list cases of tests/walk_list_cases.py on the CPU: for every case the sequential restatement, the
sequential emulation and the fixed-point emulation (the kernel's rounds over the kernel's per-point functions)
agree, and the emulation proves the case's condition: the most window walks in one round stand at the walk
list's capacity (kProjWalkCap, read from rsc_projrounds.h), one past it, or at least 64 past it, within 16 rounds."""
import numpy as np
import pytest

import lastproj_emu_lib as se
import localproj_emu_lib as le
import walk_list_cases as wl

MAX_ROUNDS = 16  # the device runs every round with thousands of walkers: keeps the GPU test within seconds


def test_cap_is_read_from_the_header():
    cap = wl.walk_cap()
    assert cap >= 1024 and cap % 32 == 0  # walk[] is an LDS array handed out to subgroups of 16 lanes
    assert wl.EXCESS["at_cap"] == 0 and wl.EXCESS["cap_plus_1"] == 1 and wl.EXCESS["overflow"] >= 64


def _condition(fp, excess, n, static):
    cap = wl.walk_cap()
    assert fp["max_round_walks"] == n - static
    if excess >= 64:
        assert fp["max_round_walks"] >= cap + 64
    else:
        assert fp["max_round_walks"] == cap + excess
    assert fp["walks"] >= 3 * fp["max_round_walks"]  # the list is full in at least three rounds
    assert 4 <= fp["rounds"] <= MAX_ROUNDS


@pytest.mark.parametrize("name", sorted(wl.local_cases()))
def test_local_case(name):
    p, excess = wl.local_cases()[name]
    ref = wl.reference("local", name)
    seq, fp = le.search_sequential(p), le.search_fixed_point(p)
    for r in (seq, fp):
        assert np.array_equal(r["out"], ref["out"])
        assert r["track"].tobytes() == ref["track"].tobytes()
        assert (r["nmatches"], r["n_to_match"]) == (ref["nmatches"], ref["n_to_match"])
    assert fp["rounds"] == ref["rounds"]
    assert ref["n_to_match"] == p.pts.n
    _condition(fp, excess, p.pts.n, wl.LOCAL_STATIC)
    if name.startswith("vetoed"):  # worked out in walk_list_cases.py
        assert ref["out"].tolist() == [0, 1, 2, 3] + [-1] * 8 and ref["nmatches"] == 4 and ref["rounds"] == 6
        assert fp["walks"] == 3 * (p.pts.n - 3)
    else:  # the walkers' decisions are features: everyone matches, the last point stays on feature 8
        assert ref["out"].tolist() == list(range(8)) + [p.pts.n - 1, -1, -1, -1]
        assert ref["nmatches"] == p.pts.n and ref["rounds"] == 10


@pytest.mark.parametrize("name", sorted(wl.last_cases()))
def test_last_case(name):
    p, excess = wl.last_cases()[name]
    ref = wl.reference("last", name)
    seq, fp = se.search_sequential(p), se.search_fixed_point(p)
    for r in (seq, fp):
        assert np.array_equal(r["out"], ref["out"])
        assert (r["nmatches"], r["mode"]) == (ref["nmatches"], ref["mode"])
    assert fp["rounds"] == ref["rounds"]
    _condition(fp, excess, p.last.n, wl.LAST_STATIC)
    if name.startswith("plain"):
        assert ref["out"].tolist() == list(range(8)) and ref["nmatches"] == 8 and ref["rounds"] == 10
    else:  # feature 6 carries every later slot's claim and is nulled by the removed rotation bin
        assert ref["out"].tolist() == [0, 1, 2, 3, 4, 5, -2, -1]
        removed = sum(1 for i in range(6, p.last.n) if i % 97 == 0)
        assert removed > 0 and ref["nmatches"] == p.last.n - removed


def test_regular_neighbours_share_the_launch_arguments():
    """th (and check_orientation) are arguments of a launch: the regular problems of the batches use the cases'."""
    for cases, regular in ((wl.local_cases(), wl.local_regular()), (wl.last_cases(), wl.last_regular())):
        ths = {p.th for p, _ in cases.values()} | {p.th for p in regular}
        assert len(ths) == 1
    assert {p.check_ori for p, _ in wl.last_cases().values()} | {p.check_ori for p in wl.last_regular()} == {1}
