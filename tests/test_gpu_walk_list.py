"""The rounds loop's walk list (proj_rounds, rsc_projrounds.h) at and beyond its capacity on the device: the
cases of tests/walk_list_cases.py (their conditions are proved on the CPU by tests/test_cpu_walk_list.py: the
walkers of one round stand at kProjWalkCap, one past it and 101 past it) through the local-map matcher (fused
and matcher-only) and the last-frame matcher, each case alone and as the middle problem of a batch between two
regular problems.  Device == sequential restatement, bit for bit: out (with the entries the rotation check
nulled), track, nmatches, n_to_match, mode, rounds.  The points past the list fall back to the one-lane walk
inside the pick loop; the fixed point is the same."""
import numpy as np
import pytest

import lastproj_cases as sc
import localproj_cases as lc
import test_gpu_lastproj as gs
import test_gpu_localproj as gl
import walk_list_cases as wl

pytestmark = pytest.mark.gpu


def check_local(r, k, ref, where):
    assert int(r["nmatches"][k]) == ref["nmatches"], f"{where}: nmatches {int(r['nmatches'][k])}"
    assert int(r["n_to_match"][k]) == ref["n_to_match"], f"{where}: n_to_match {int(r['n_to_match'][k])}"
    assert np.array_equal(r["out"][k], ref["out"]), f"{where}: out {r['out'][k].tolist()}"
    assert np.asarray(r["track"][k]).tobytes() == ref["track"].tobytes(), f"{where}: track"
    assert int(r["rounds"][k]) == ref["rounds"], f"{where}: rounds {int(r['rounds'][k])}"


def check_last(r, k, ref, where):
    assert int(r["nmatches"][k]) == ref["nmatches"], f"{where}: nmatches {int(r['nmatches'][k])}"
    assert int(r["mode"][k]) == ref["mode"], f"{where}: mode"
    assert np.array_equal(r["out"][k], ref["out"]), f"{where}: out {r['out'][k].tolist()}"
    assert int(r["rounds"][k]) == ref["rounds"], f"{where}: rounds {int(r['rounds'][k])}"


@pytest.fixture(scope="module")
def regular_refs():
    return dict(local=[lc.reference(p) for p in wl.local_regular()], last=[sc.reference(p) for p in wl.last_regular()])


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", sorted(wl.local_cases()))
def test_local_alone_and_in_a_batch(name, fused, regular_refs):
    p = wl.local_cases()[name][0]
    ref = wl.reference("local", name)
    a, b = wl.local_regular()
    ra, rb = regular_refs["local"]
    tr = lambda *refs: None if fused else [x["track"].copy() for x in refs]
    r = gl.run_many([p], tr(ref))
    check_local(r, 0, ref, f"{name} alone")
    r = gl.run_many([a, p, b], tr(ra, ref, rb))
    check_local(r, 0, ra, f"{name} batch: first regular")
    check_local(r, 1, ref, f"{name} batch: middle")
    check_local(r, 2, rb, f"{name} batch: last regular")


@pytest.mark.parametrize("name", sorted(wl.last_cases()))
def test_last_alone_and_in_a_batch(name, regular_refs):
    p = wl.last_cases()[name][0]
    ref = wl.reference("last", name)
    a, b = wl.last_regular()
    ra, rb = regular_refs["last"]
    r = gs.run_many([p])
    check_last(r, 0, ref, f"{name} alone")
    if name == "features_overflow":
        assert (r["out"][0] == -2).sum() == 1  # the entry nulled by the removed rotation bin
    r = gs.run_many([a, p, b])
    check_last(r, 0, ra, f"{name} batch: first regular")
    check_last(r, 1, ref, f"{name} batch: middle")
    check_last(r, 2, rb, f"{name} batch: last regular")
