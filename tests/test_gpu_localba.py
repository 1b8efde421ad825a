"""rsc_local_bundle_adjustment_many on the device against the sequential host restatement (tests/localba_emu, mode
0: g2o's control flow line by line), byte for byte on every output: poses, points, edge flags, the erase list, the
chi2 doubles of both phases and every counter.  The cases are those of tests/localba_cases.py, each at the
smallest shape that exercises what its name says."""
import numpy as np
import pytest

import localba_cases as lc
import localba_emu_lib as le
from gpu_common import ctx
from rsc import engine

pytestmark = pytest.mark.gpu

_ref = {}


def problem(name):
    if name not in _ref:
        p = lc.build(name)
        st, r = le.run(p, 0)
        assert st == 0
        _ref[name] = (p, r)
    return _ref[name]


def assert_same(g, r, where):
    for k in ("Tcw", "pos", "edge_flags", "erase"):
        assert g[k].shape == r[k].shape, f"{where} {k} shape"
        assert np.array_equal(g[k].view(np.uint8), r[k].view(np.uint8)), f"{where} {k}\n{g[k]}\n{r[k]}"
    for k in ("n_erase", "n_level1", "status", "branches"):
        assert g[k] == r[k], f"{where} {k}: {g[k]} vs {r[k]}"
    for i in range(2):
        for k, v in r["phase"][i].items():
            w = g["phase"][i][k]
            # every double is compared by its bytes, but where the host's chi2 is a NaN the device's must be one: the
            # sign an invalid operation gives its NaN is the processor's (x86 sets it, the device does not).  Only
            # the cases of NAN_CHI2 may have one.
            same = np.float64(v).tobytes() == np.float64(w).tobytes() if isinstance(v, np.float64) else v == w
            if not same and isinstance(v, np.float64) and np.isnan(v) and np.isnan(w):
                assert any(n in where for n in NAN_CHI2), f"{where} phase {i} {k}: a NaN chi2 outside {NAN_CHI2}"
                same = True
            assert same, f"{where} phase {i} {k}: {w!r} vs {v!r}"


# the cases whose chi2 is a NaN in some field of the host result (a NaN anywhere else fails)
NAN_CHI2 = ("edge_nan_pos", "edge_inf_pos", "edge_nan_pose", "edge_nan_fixed_pose")
REGULAR_LIKE = [n for n in lc.CASES if not n.startswith("edge_")]


def test_nan_chi2_cases_are_the_expected_ones():
    has_nan = [n for n in lc.CASES
               if any(np.isnan(q[k]) for q in problem(n)[1]["phase"] for k in ("chi2_first", "chi2_last"))]
    assert sorted(has_nan) == sorted(NAN_CHI2)


@pytest.mark.parametrize("name", REGULAR_LIKE)
def test_case(name):
    p, r = problem(name)
    g = engine.local_bundle_adjustment(ctx(), p)
    assert_same(g, r, name)


@pytest.mark.parametrize("kind", lc.EDGE_KINDS)
def test_edge_kind_between_regular_problems(kind):
    """NaN / Inf / z == 0 / zero and negative information / NaN poses, each between two regular problems of one
    call: the neighbours' results are those of their own calls."""
    names = ["small_mixed", "edge_" + kind, "ids_shuffled"]
    got = engine.local_bundle_adjustment_many(ctx(), [problem(n)[0] for n in names])
    for n, g in zip(names, got):
        assert_same(g, problem(n)[1], f"{kind}/{n}")


def test_count_three_equals_three_calls():
    names = ["two_groups", "outliers", "mono_once"]
    many = engine.local_bundle_adjustment_many(ctx(), [problem(n)[0] for n in names])
    for n, g in zip(names, many):
        one = engine.local_bundle_adjustment(ctx(), problem(n)[0])
        assert_same(g, one, n)
        assert_same(g, problem(n)[1], n)


def test_independent_of_staging_history():
    """The same call after every staging buffer was filled with 0xA5 (and after a larger problem ran) gives the
    same bytes: nothing is read that the call did not write."""
    c = ctx()
    p, r = problem("lose_all")
    first = engine.local_bundle_adjustment(c, p)
    engine.local_bundle_adjustment(c, problem("limit_free64")[0])
    assert c.fill_staging(0xA5) > 0
    again = engine.local_bundle_adjustment(c, p)
    assert_same(again, first, "after fill")
    assert_same(again, r, "after fill vs host")


def test_count_zero_and_timing():
    c = ctx()
    assert engine.local_bundle_adjustment_many(c, []) == []
    c.enable_timing(True)
    try:
        engine.local_bundle_adjustment(c, problem("small_mixed")[0])
        assert c.last_timing()["refine_ms"] > 0.0
    finally:
        c.enable_timing(False)


REFUSALS = ["kf_id twice", "too many free KeyFrames"] + ["NULL " + f for f in (
    "kf_id", "fixed", "Tcw", "cam", "mp_id", "pos", "bad", "obs_begin", "obs_kf", "uv", "u_right", "inv_sigma2")]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_leave_outputs_and_context(what):
    """rsc_local_bundle_adjustment_many itself, on a live context: a refused call returns its code, leaves the
    outputs as they were and the context usable."""
    c = ctx()
    p = dict(problem("small_mixed")[0])
    code = -1
    if what == "kf_id twice":
        p["kf_id"] = p["kf_id"].copy()
        p["kf_id"][1] = p["kf_id"][0]
    elif what == "too many free KeyFrames":
        p = dict(problem("limit_free64")[0])
        p["fixed"] = np.zeros_like(p["fixed"])
        code = -4
    q, keep = engine.localba_pack(p)
    if what.startswith("NULL "):
        setattr(q, what[5:], None)
    arrays = engine.localba_outputs(p)
    before = {k: v.copy() for k, v in arrays.items()}
    o = engine.LocalBAOut()
    for k, v in arrays.items():
        setattr(o, k, v.ctypes.data)
    import ctypes as C
    r = engine.LocalBAResult()
    st = engine.load_library().rsc_local_bundle_adjustment_many(c.h, C.byref(q), 1, C.byref(o), C.byref(r))
    assert st == code
    for k, v in arrays.items():
        assert np.array_equal(v.view(np.uint8), before[k].view(np.uint8)), k
    g = engine.local_bundle_adjustment(c, problem("small_mixed")[0])
    assert_same(g, problem("small_mixed")[1], "after a refusal")
