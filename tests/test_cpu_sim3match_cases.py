"""The hand-built SearchBySim3 cases (sim3match_cases.py) pinned on the CPU:

* on every case the independent restatement (sim3match_ref.py) equals the oracle's trace on vnMatch1, vnMatch2,
  both reason vectors, out12 and nFound, and both equal the hand-written expectations;
* the census shows every branch the cases were built for is really taken, in each direction;
* every perturbation of sim3match_ref.PERTURBATIONS (one rule switched off in one direction) changes the
  result on at least one case, so a kernel with that mistake cannot pass the GPU parity on these cases;
* the random pairs the older tests rest on miss the source/destination mix-ups (equal cameras and pyramids on
  both sides, KF1 at the origin) -- pinned, as the reason these cases exist;
* the committed fixture tests/golden/sim3match_cases.npz holds exactly these inputs and answers.
"""
import os

import numpy as np
import pytest

import oracle_lib as ol
import sim3match_cases as sc
import sim3match_ref as sr
from rsc import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sim3match_cases.npz")
GROUPS = sc.groups()
FLAT = [(g, name, th, c) for g, (th, cases) in GROUPS.items() for name, c in cases]
_traces = {}


def trace(g, name, th, c):
    """The restatement's trace of a case, computed once."""
    if (g, name) not in _traces:
        _traces[(g, name)] = sr.py_trace(c.kf1, c.kf2, c.R12, c.t12, c.m12, th)
    return _traces[(g, name)]


def holds(expected, got):
    """The hand-written vector, except where it is UNPINNED."""
    pinned = expected != sc.UNPINNED
    return np.array_equal(expected[pinned], got[pinned])


@pytest.mark.parametrize("group", list(GROUPS))
def test_restatement_oracle_and_hand_answers_agree(group):
    th, cases = GROUPS[group]
    assert 1 <= len(cases) <= 16
    for name, c in cases:
        assert max(c.kf1.n, c.kf2.n) <= 520
        t = trace(group, name, th, c)
        nf, out, m1, m2, r1, r2 = ol.search_by_sim3_trace(c.kf1, c.kf2, c.R12, c.t12, c.m12, th)
        assert np.array_equal(m1, t.m1) and np.array_equal(m2, t.m2), name
        assert np.array_equal(r1, t.reason1) and np.array_equal(r2, t.reason2), name
        assert np.array_equal(out, t.out) and nf == t.nfound, name
        assert holds(c.m1, m1) and holds(c.m2, m2) and holds(c.out, out), name
        assert nf == int((c.out >= 0).sum()), name
        # the wrapper is the trace without its extra outputs
        wn, wout = ol.search_by_sim3(c.kf1, c.kf2, c.R12, c.t12, c.m12, th)
        assert wn == nf and np.array_equal(wout, out), name
        # reasons and matches are consistent
        assert np.array_equal(r1 == sr.MATCHED, m1 >= 0) and np.array_equal(r2 == sr.MATCHED, m2 >= 0), name


def test_unpinned_slots_are_few_and_only_in_levels():
    for g, name, th, c in FLAT:
        n = int((c.m1 == sc.UNPINNED).sum() + (c.m2 == sc.UNPINNED).sum())
        assert n == 0 or (g == "levels" and n <= 40), (g, name, n)
        assert (c.out != sc.UNPINNED).all()


def test_largest_pair_is_fully_mutual():
    c = dict(GROUPS["shapes"][1])["513x513"]
    assert c.kf1.n == 513 and np.array_equal(np.sort(c.out), np.arange(513))


def test_census_conditions():
    cen = sr.census([trace(*f) for f in FLAT])
    for d in (0, 1):
        for reason in sr.REASONS:
            assert cen[d][reason] > 0, (d, reason)
        for k in ("tie", "best_100", "best_101", "level_clamp_low", "level_clamp_high", "clamp_min_x",
                  "clamp_max_x", "clamp_min_y", "clamp_max_y"):
            assert cen[d][k] > 0, (d, k)
    # the clamps come from the cases built for them
    edges = sr.census([trace(*f) for f in FLAT if f[0] == "edges"])
    assert all(edges[0][k] > 0 for k in ("clamp_min_x", "clamp_max_x", "clamp_min_y", "clamp_max_y"))
    ties = sr.census([trace(*f) for f in FLAT if f[0] == "ties"])
    assert ties[0]["tie"] == 7 and ties[1]["tie"] == 7 and ties[0]["best_100"] >= 1


def changed(base, t, d, name):
    """Does the perturbed trace differ where direction d's mistake can show?"""
    if name == "t_no_agreement":
        return not np.array_equal(base.out, t.out)
    return not np.array_equal(base.m1 if d == 0 else base.m2, t.m1 if d == 0 else t.m2)


# the groups that can notice anything in the remaining cases are small; `shapes` repeats one rule 3000 times
PERTURBED = [f for f in FLAT if f[0] != "shapes"]


@pytest.mark.parametrize("name", list(sr.PERTURBATIONS))
def test_every_perturbation_is_noticed(name):
    for d in sr.PERTURBATIONS[name][0]:
        hit = [(g, cn) for g, cn, th, c in PERTURBED
               if changed(trace(g, cn, th, c), sr.py_trace(c.kf1, c.kf2, c.R12, c.t12, c.m12, th, name, (d,)), d, name)]
        assert hit, (name, d)
        # the source/destination confusions are what the `frames` group is for
        if name[0] in "abefij":
            assert any(g == "frames" for g, _ in hit), (name, d)


# what the source/destination mix-ups look like on the generator's pairs: by construction both KeyFrames share
# intrinsics, bounds, pyramid and grid, and KF1's translation is zero
BLIND = {"a_dst_intrinsics", "a_src_intrinsics", "e_src_bounds", "f_no_min_in_cells", "i_src_log_factor",
         "i_src_levels", "j_src_scale_table"}


def test_random_pairs_miss_the_frame_confusions():
    """The first pair each seed of test_gpu_sim3match.py draws (smaller, for the Python restatement's sake:
    the blindness is structural, not statistical)."""
    pairs = []
    for seed in (201, 202, 203, 204):
        rng = np.random.default_rng(seed)
        pairs.append(synth.make_sim3match_pair(rng, 160, 50, 0.3))
    unnoticed = set(sr.PERTURBATIONS)
    for kf1, kf2, R12, t12, m12 in pairs:
        assert not np.asarray(kf1.tcw).any()
        base = sr.py_trace(kf1, kf2, R12, t12, m12)
        assert base.nfound > 5
        for name in sorted(unnoticed):
            t = sr.py_trace(kf1, kf2, R12, t12, m12, 7.5, name)
            if not (np.array_equal(base.m1, t.m1) and np.array_equal(base.m2, t.m2) and
                    np.array_equal(base.out, t.out)):
                unnoticed.discard(name)
    print("perturbations the random pairs do not notice:", sorted(unnoticed))
    assert BLIND <= unnoticed
    # KF1's translation is zero, so ignoring the source's translation is invisible in the KF1 -> KF2 direction
    for kf1, kf2, R12, t12, m12 in pairs:
        base = sr.py_trace(kf1, kf2, R12, t12, m12)
        t = sr.py_trace(kf1, kf2, R12, t12, m12, 7.5, "b_no_src_translation", (0,))
        assert np.array_equal(base.m1, t.m1) and np.array_equal(base.out, t.out)


def load_golden():
    """(group, case name) -> dict(kf1, kf2, R12, t12, m12, th, m1, m2, out, nfound); the layout is that of
    tests/golden/make_sim3match_cases_golden.py."""
    g = np.load(GOLDEN)
    ko, fo, so = g["kf_off"], g["feat_off"], g["sf_off"]
    kfs = []
    for k in range(len(ko) - 1):
        a, b = int(ko[k]), int(ko[k + 1])
        f = {x: g[x][a:b] for x in ("kp", "octave", "desc", "mp_state", "mp_pos", "mp_dmax", "mp_dmin", "mp_desc")}
        fx, fy, cx, cy, x0, x1, y0, y1, lg, gw, gh = (float(v) for v in g["geom"][k])
        kfs.append(synth.Sim3KF(b - a, mp_id=np.full(b - a, -1, np.int64), cell_begin=g["cell_begin"][k],
                                cell_feat=g["cell_feat"][int(fo[k]):int(fo[k + 1])], Rcw=g["Rcw"][k], tcw=g["tcw"][k],
                                scale_factors=g["scale_factors"][int(so[k]):int(so[k + 1])], fx=fx, fy=fy, cx=cx,
                                cy=cy, min_x=x0, max_x=x1, min_y=y0, max_y=y1, log_scale_factor=lg, grid_w_inv=gw,
                                grid_h_inv=gh, **f))
    cases = {}
    o1, o2 = g["c1_off"], g["c2_off"]
    for k, key in enumerate(g["names"]):
        grp, name = str(key).split(":", 1)
        a, b = (int(v) for v in g["case_kf"][k])
        s1, s2 = slice(int(o1[k]), int(o1[k + 1])), slice(int(o2[k]), int(o2[k + 1]))
        cases[(grp, name)] = dict(kf1=kfs[a], kf2=kfs[b], th=float(g["case_th"][k]), nfound=int(g["case_n"][k]),
                                  R12=g["case_R12"][k], t12=g["case_t12"][k], m12=g["m12"][s1], m1=g["m1"][s1],
                                  out=g["out"][s1], m2=g["m2"][s2])
    return cases


def test_golden_fixture_holds_these_cases():
    gold = load_golden()
    assert set(gold) == {(g, name) for g, name, th, c in FLAT}
    for g, name, th, c in FLAT:
        w = gold[(g, name)]
        for x in ("kp", "octave", "desc", "cell_begin", "cell_feat", "Rcw", "tcw", "mp_state", "mp_pos", "mp_dmax",
                  "mp_dmin", "mp_desc", "scale_factors"):
            for a, b in ((c.kf1, w["kf1"]), (c.kf2, w["kf2"])):
                assert np.array_equal(np.asarray(getattr(a, x)), getattr(b, x), equal_nan=x == "mp_pos"), (name, x)
        assert w["th"] == th and np.array_equal(w["m12"], c.m12) and np.array_equal(w["R12"], c.R12)
        nf, out, m1, m2, _, _ = ol.search_by_sim3_trace(w["kf1"], w["kf2"], w["R12"], w["t12"], w["m12"], w["th"])
        assert nf == w["nfound"] and np.array_equal(out, w["out"]), name
        assert np.array_equal(m1, w["m1"]) and np.array_equal(m2, w["m2"]), name
        assert holds(c.m1, w["m1"]) and holds(c.m2, w["m2"]) and holds(c.out, w["out"]), name
