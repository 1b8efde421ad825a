"""MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth without a GPU: the sequential restatement
(tests/mpupdate_ref.py) against the answers worked out by hand (tests/mpupdate_cases.py) and against the golden
fixture it wrote; the host build of the kernels' per-point arithmetic in the kernels' lane decompositions
(tests/mpupdate_emu) against the restatement, bit for bit, on every case and on random lists of every size class;
the limit; and the stand-alone emulation program under the host sanitizers."""
import json
import os
import subprocess

import numpy as np
import pytest

import fusekf_ref as fr
import mpupdate_cases as mc
import mpupdate_emu_lib as me
import mpupdate_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mc.cases()
FIELDS = ("desc", "best_obs", "normal", "dmax", "dmin", "updated")
f32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "mpupdate_traces.npz"))


@pytest.fixture(scope="module")
def randoms():
    return {name: mc.random_problem(seed) for name, seed in mc.RANDOM_SEEDS.items()}


def from_golden(golden, name, what=3):
    """The fixture's what = 3 result cut down to what a call with `what` writes."""
    r = {k: golden[f"{name}/{k}"].copy() for k in FIELDS}
    if not what & 1:
        r["desc"][:] = mr.FILL["desc"]
        r["best_obs"][:] = mr.FILL["best_obs"]
    if not what & 2:
        for k in ("normal", "dmax", "dmin"):
            r[k][:] = mr.FILL[k]
    r["updated"] &= what
    return r


def check_expectation(name, r):
    """The hand-worked answers of a case against a result of what = 3."""
    p, exp = CASES[name]
    n = p.upd.n_points
    for i in range(n):
        b, a = exp["best_obs"][i], exp["desc"][i]
        assert int(r["best_obs"][i]) == (mr.FILL["best_obs"] if b is None else b), (name, i)
        want = np.full(32, mr.FILL["desc"], np.uint8) if a is None else mc.bits(a)
        assert np.array_equal(r["desc"][i], want), (name, i)
    for k in ("normal", "dmax", "dmin"):
        if k in exp:
            assert mr.same_floats(r[k], np.array(exp[k], f32)), (name, k, r[k], exp[k])
    assert r["updated"].tolist() == exp.get("updated", [3] * n), name
    if "nan_normal" in exp:
        assert np.isnan(r["normal"]).all(axis=1).tolist() == exp["nan_normal"]
        assert np.isnan(r["dmax"]).tolist() == exp["nan_depth"] and np.isnan(r["dmin"]).tolist() == exp["nan_depth"]
    for i in range(n):  # untouched points keep every byte
        if r["updated"][i] == 0:
            assert (r["normal"][i] == mr.FILL["normal"]).all() and r["dmax"][i] == mr.FILL["dmax"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_known_answer(name, golden):
    r = mr.update(CASES[name][0], 3)
    check_expectation(name, r)
    assert mr.same_result(r, from_golden(golden, name)) == ""
    for what in (1, 2):
        assert mr.same_result(mr.update(CASES[name][0], what), from_golden(golden, name, what)) == "", what


def test_cases_cover_the_fixture(golden):
    assert sorted(str(s) for s in golden["names"]) == sorted(CASES)


def test_rules_are_not_vacuous():
    """The other rule each case is there to exclude picks another, distinct descriptor."""
    def numbers(name):
        p, _ = CASES[name]
        return [p.kfs[k].desc[i] for k, i in zip(p.upd.obs_kf, p.upd.obs_idx)]
    for name, key in (("tie_first_wins", "le_rule"), ("even4_lower_median", "upper_rule"),
                      ("even6_lower_median", "upper_rule")):
        d, exp = numbers(name), CASES[name][1]
        D = np.sort(mr.distances(d), axis=1)
        n = len(d)
        if key == "le_rule":  # `median <= BestMedian` keeps the last row of the smallest median
            med = D[:, int(0.5 * (n - 1))]
            other = int(np.nonzero(med == med.min())[0][-1])
        else:                 # the upper median of an even N
            other = int(np.argmin(D[:, n // 2]))
        assert [other] == exp[key] and other != exp["best_obs"][0]
        assert not np.array_equal(d[other], d[exp["best_obs"][0]])
    p, exp = CASES["bad_kf_skipped"]  # with the bad KeyFrame's observation kept the answer is another one
    d = numbers("bad_kf_skipped")
    assert [mr.best_row(d)] == exp["with_bad"] and exp["with_bad"] != exp["best_obs"]
    for name in CASES:
        if "medians" in CASES[name][1]:
            assert mr.row_medians(numbers(name)).tolist() == CASES[name][1]["medians"][0], name


def test_list_order_shows_in_the_normal():
    """Reversing the list changes bits of the normal (the sum is not associative), by rounding only; the emulation
    has the bits of the list order."""
    p, _ = CASES["order_matters"]
    a, b = mr.update(p, 2), mr.update(p, 2, reverse=True)
    assert not np.array_equal(a["normal"].view(np.uint32), b["normal"].view(np.uint32))
    assert np.allclose(a["normal"], b["normal"], rtol=1e-6, atol=1e-7)
    assert me.update(p, 2)["normal"].view(np.uint32).tolist() == a["normal"].view(np.uint32).tolist()


def test_agrees_with_the_fuse_model_in_keyframe_id_order():
    """fusekf_ref.MapPoint.compute_distinctive_descriptors walks the observations in KeyFrame-id order: with the
    list given in that order the two independent restatements pick the same descriptor."""
    rng = np.random.default_rng(77)
    for n in (1, 2, 3, 4, 9, 20):
        b = mc.Builder()
        centre = rng.integers(0, 256, 32, dtype=np.uint8)
        ks = []
        for _ in range(n):
            d = centre.copy()
            for bit in rng.choice(256, int(rng.integers(0, 30)), replace=False):
                d[bit // 8] ^= 1 << (bit % 8)
            ks.append(b.kf([d]))
        b.point((0.0, 0.0, 2.0), [(k, 0) for k in ks])
        p = b.problem()
        m = fr.MapPoint(0, np.zeros(3, f32), np.zeros(3, f32), f32(1), f32(1), np.zeros(32, np.uint8))
        for k in reversed(ks):  # inserted in any order, iterated by id
            kf = fr.KeyFrame.__new__(fr.KeyFrame)
            kf.id, kf.desc, kf.stereo = k, p.kfs[k].desc, np.zeros(1, bool)
            m.add_observation(kf, 0)
        m.compute_distinctive_descriptors()
        r = mr.update(p, 1)
        assert np.array_equal(m.desc, r["desc"][0]), n


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulation_hand_built(name):
    p, exp = CASES[name]
    for what in (1, 2, 3):
        want = mr.update(p, what)
        for mode in (0, 1):
            assert mr.same_result(me.update(p, what, mode), want) == "", (what, mode)
    if "medians" in exp:
        assert me.medians(p, 0) == exp["medians"][0]


@pytest.mark.parametrize("name", sorted(mc.RANDOM_SEEDS))
def test_emulation_random(name, golden, randoms):
    """Lists of 1, 2, 3, 63, 64 (one row per lane), 65, 200 and 1,024 observations (strided rows)."""
    p = randoms[name]
    assert np.array_equal(p.upd.pos, golden[f"{name}/pos"]) and np.array_equal(p.upd.obs_idx, golden[f"{name}/obs_idx"])
    assert mr.same_result(mr.update(p, 3), from_golden(golden, name)) == ""
    for what in (1, 2, 3):
        for mode in (0, 1):
            assert mr.same_result(me.update(p, what, mode), from_golden(golden, name, what)) == "", (what, mode)
    if name == "random_b":  # KeyFrame 2 is bad there: the long lists lose a quarter of their rows
        assert p.upd.kf_bad.tolist() == [0, 0, 1, 0]
        assert not np.array_equal(golden["random_b/best_obs"], mr.update(_without_bad(p), 1)["best_obs"])


def _without_bad(p):
    import copy
    q = copy.copy(p)
    q.upd = copy.copy(p.upd)
    q.upd.kf_bad = None
    return q


def test_limit():
    """1,024 observations are served, 1,025 refused before anything is written; a skipped point's list is not read."""
    b = mc.Builder()
    k = b.kf([i % 200 for i in range(1100)])
    b.point((0.0, 0.0, 2.0), [(k, i) for i in range(1024)])
    p = b.problem()
    assert mr.same_result(me.update(p, 3, 1), mr.update(p, 3)) == ""
    b.point((0.0, 0.0, 2.0), [(k, i) for i in range(1025)])
    assert me.update(b.problem(), 3, 1) is None and me.update(b.problem(), 3, 0) is None
    b.pts[-1]["skip"] = True
    assert me.update(b.problem(), 3, 1)["updated"].tolist() == [3, 0]


@pytest.mark.parametrize("prog", ["mpupdate_emu_main", "mpupdate_emu_main_san"])
def test_standalone_program(prog):
    me.lib()  # builds the directory
    path = os.path.join(me.DIR, "build", prog)
    assert os.path.exists(path), path
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mismatches"] == 0 and out["refused"] == 2 and out["updated"] >= 20
