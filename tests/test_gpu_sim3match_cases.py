"""GPU parity of ORBmatcher::SearchBySim3 on the hand-built cases (sim3match_cases.py): one batch per group
through rsc_search_by_sim3_many, with both directions read back (rsc_diag_sim3match_directions).  vnMatch1,
vnMatch2, out12 and nFound are bit-equal to the oracle's trace, to the committed fixture
(tests/golden/sim3match_cases.npz) and to the hand-written answers; test_cpu_sim3match_cases.py proves that
every single-rule mistake of sim3match_ref.PERTURBATIONS changes one of these vectors on some case."""
import copy
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import sim3match_cases as sc
from gpu_common import ctx
from rsc import engine
from test_cpu_sim3match_cases import holds, load_golden

pytestmark = pytest.mark.gpu
GROUPS = sc.groups()
RSC_ERR_ARG = -1
_gold = {}


def gold():
    if not _gold:
        _gold.update(load_golden())
    return _gold


def run(cases, th):
    """[(out, nfound, m1, m2)] of one batch."""
    s = engine.Sim3Search(ctx(), [(c.kf1, c.kf2, c.R12, c.t12, c.m12) for c in cases], th)
    outs, nf = s.run()
    return [(outs[k].copy(), int(nf[k])) + s.directions(k) for k in range(len(cases))]


@pytest.mark.parametrize("group", list(GROUPS))
def test_group_parity(group):
    th, cases = GROUPS[group]
    got = run([c for _, c in cases], th)
    for (name, c), (out, nf, m1, m2) in zip(cases, got):
        on, oout, om1, om2, _, _ = ol.search_by_sim3_trace(c.kf1, c.kf2, c.R12, c.t12, c.m12, th)
        assert np.array_equal(m1, om1) and np.array_equal(m2, om2), name
        assert np.array_equal(out, oout) and nf == on, name
        w = gold()[(group, name)]
        assert np.array_equal(m1, w["m1"]) and np.array_equal(m2, w["m2"]), name
        assert np.array_equal(out, w["out"]) and nf == w["nfound"], name
        assert holds(c.m1, m1) and holds(c.m2, m2) and holds(c.out, out), name
    if group == "shapes":
        assert max(nf for _, nf, _, _ in got) == 513


@pytest.mark.parametrize("group", ["shapes", "agree"])
def test_reversed_batch_and_single_pair(group):
    th, cases = GROUPS[group]
    cs = [c for _, c in cases]
    fwd = run(cs, th)
    rev = run(cs[::-1], th)[::-1]
    for (name, _), a, b in zip(cases, fwd, rev):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
    k = max(range(len(cs)), key=lambda i: cs[i].kf1.n)   # count == 1: the largest pair alone
    one = run([cs[k]], th)[0]
    assert all(np.array_equal(x, y) for x, y in zip(one, fwd[k])), cases[k][0]


def test_readback_argument_errors():
    L = engine.load_library()
    fresh = engine.Context(0)
    a1, a2 = np.zeros(16, np.int32), np.zeros(16, np.int32)
    # no SearchBySim3 call on this context yet
    assert L.rsc_diag_sim3match_directions(fresh.h, 0, a1, 1, a2, 1) == RSC_ERR_ARG
    th, cases = GROUPS["agree"]
    c = cases[0][1]
    s = engine.Sim3Search(fresh, [(c.kf1, c.kf2, c.R12, c.t12, c.m12)], th)
    s.run()
    n1, n2 = c.kf1.n, c.kf2.n
    assert L.rsc_diag_sim3match_directions(fresh.h, 0, a1, n1, a2, n2) == 0
    assert holds(c.m1, a1[:n1]) and holds(c.m2, a2[:n2])
    for pair, k1, k2 in ((1, n1, n2), (-1, n1, n2), (0, n1 - 1, n2), (0, n1, n2 + 1)):
        assert L.rsc_diag_sim3match_directions(fresh.h, pair, a1, k1, a2, k2) == RSC_ERR_ARG
    with pytest.raises(RuntimeError):
        s.directions(1)


def test_undefined_conversions_are_refused():
    """A non-finite mfMaxDistance / mfMinDistance of a good MapPoint, a non-finite th and a radius beyond 2^30
    cells return RSC_ERR_ARG before any launch (include/rsc.h): the reference's float -> int conversions are
    undefined there."""
    L = engine.load_library()
    c0 = ctx()
    th, cases = GROUPS["agree"]
    c = cases[0][1]
    good = next(i for i in range(c.kf1.n) if c.kf1.mp_state[i] == 1)
    null = next(i for i in range(c.kf1.n) if c.kf1.mp_state[i] == 0)
    for field, value in (("mp_dmax", np.inf), ("mp_dmax", np.nan), ("mp_dmin", np.inf), ("mp_dmin", -np.inf)):
        for slot, status in ((good, RSC_ERR_ARG), (null, 0)):   # only slots with mp_state == 1 are looked at
            kf = copy.copy(c.kf1)
            arr = np.array(getattr(kf, field), np.float32)
            arr[slot] = value
            setattr(kf, field, arr)
            k, keep = engine.sim3_kf_struct(kf)
            h = C.c_void_p()
            assert L.rsc_kfview_create(c0.h, C.byref(k), C.byref(h)) == status, (field, value, slot)
            if status == 0:
                L.rsc_kfview_destroy(h)
    top = float(c.kf1.scale_factors[-1]) * max(c.kf1.grid_w_inv, c.kf1.grid_h_inv)
    limit = np.float32(2.0 ** 30)
    over = np.float32(limit / np.float32(top))
    while np.float32(np.float32(over * c.kf1.scale_factors[-1]) * np.float32(c.kf1.grid_w_inv)) < limit:
        over = np.nextafter(over, np.float32(np.inf))
    for bad in (np.inf, -np.inf, np.nan, float(over), 1e30):
        s = engine.Sim3Search(c0, [(c.kf1, c.kf2, c.R12, c.t12, c.m12)], bad)
        st = L.rsc_search_by_sim3_many(c0.h, s.h1, s.h2, 1, s.R, s.t, s.th, s.pin, s.pout, s.nfound)
        assert st == RSC_ERR_ARG, bad
        assert (s.out[0] == -7).all()   # nothing was written
        with pytest.raises(RuntimeError):   # the failed call left nothing to read back
            s.directions(0)
    # a large but admissible radius (the whole grid is searched) still agrees with the oracle
    big = 1.0e6
    out, nf, m1, m2 = run([c], big)[0]
    on, oout, om1, om2, _, _ = ol.search_by_sim3_trace(c.kf1, c.kf2, c.R12, c.t12, c.m12, big)
    assert nf == on and np.array_equal(out, oout) and np.array_equal(m1, om1) and np.array_equal(m2, om2)
