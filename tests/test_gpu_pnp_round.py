"""GPU parity of the PnP speculation round's launch set (descriptor upload -> eigen stage -> betas
stage -> scan) on the shapes where its bookkeeping can go wrong, bit for bit against the oracle's
trace (every hypothesis' sample, inlier count and float pose), the way
test_gpu_configs.test_config2_exhaustive_batch_every_hypothesis does it:

* scan chunks of unequal size: per-solver budgets {1, 7, 15, 16, 33} over N in {5, 255, 256, 257,
  2000}, so a problem's hypotheses are cut into scan workgroups of 8 and 7, 8 and 8, 7 7 7 6 6 ...
  (rsc_api.cpp pnp_scan_partition), exhaustive and with qualifying hypotheses (masks flushed from
  chunks of unequal size, Refine);
* both eigen-stage forms at their boundary: iterate(5) of one solver (rows form, the small betas
  wave) and 1,500 hypotheses at N = 64 (75 eigen workgroups: split form, and the pair form);
* the selection among the three beta approximations when errors are not finite (coplanar and
  repeated sample points) and, over 1,500 ordinary hypotheses, by pose equality (the oracle's trace
  does not record which approximation won);
* descriptors of consecutive rounds on one context: the solver set changing 5 -> 3 -> 5 with fresh
  seeds, and a round whose descriptor blob is no multiple of 16 B x the eigen grid.

NaN poses are compared as NaN at the same positions (the sign / payload of a NaN is not an
IEEE-specified result: x86 produces the negative default NaN, gfx950 the positive one); every other
value by its bits."""
import numpy as np
import pytest

from gpu_common import assert_pnp_equal, bits, ctx
import oracle_lib as ol
from rsc import synth
from rsc import workloads as wl

pytestmark = pytest.mark.gpu


def _nan_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _oracle(sc, seed, params, its, trace=True):
    o = ol.OraclePnP(sc, int(seed))
    o.set_ransac_parameters(*params)
    if trace:
        o.enable_trace()
    ro = o.iterate(int(its))
    return o, ro


def _assert_trace(g, o, ms, where, nan_ok=False):
    """Every hypothesis of the solver's last round against the oracle's trace."""
    ints, fl = o.trace()
    cnt, pos = g.last_hypotheses(400)
    smp = g.last_samples(400)
    assert len(cnt) == len(ints) == len(smp), f"{where} hypotheses {len(cnt)} vs {len(ints)}"
    assert np.array_equal(smp[:, :ms], ints[:, :ms]), f"{where} samples"
    assert np.array_equal(cnt, ints[:, 8]), f"{where} counts"
    if nan_ok:
        assert _nan_equal(pos, fl), f"{where} poses"
    else:
        assert np.array_equal(bits(pos), bits(fl)), f"{where} poses"
    return ints, fl


def _raw_out(rec, g):
    """One record of SolverBatch.iterate_raw as the dict assert_pnp_equal takes."""
    inl = g.last_inliers() if rec["ok"] else None
    return dict(ok=bool(rec["ok"]), no_more=bool(rec["no_more"]), n_inliers=int(rec["n_inliers"]),
                iterations=int(rec["iterations"]), T=np.array(rec["T"], np.float32).reshape(4, 4),
                inliers=inl if inl is not None else np.zeros(0, bool))


# ------------------------------------------------------------------------------------------------
# uneven scan chunks
# ------------------------------------------------------------------------------------------------
UNEVEN_N = (5, 255, 256, 257, 2000)
UNEVEN_BUDGETS = np.array([1, 7, 15, 16, 33], np.int32)
# PnPsolver::iterate(n) runs until BOTH mRansacMaxIts and n are used up (the reference's `||` loop
# condition), so max iterations = 1 lets the per-solver budget alone set the hypothesis count; min
# inliers 5 keeps the N = 5 solver alive (N >= minInliers) without being reachable by its 2 or 3
# true inliers, and max(5, epsilon N) is the threshold of the others.
UNEVEN_EXHAUSTIVE = (0.99, 5, 1, 4, 0.5, 5.991)  # N / 2 of 40 % inliers: out of reach
UNEVEN_REFINE = (0.99, 5, 1, 4, 0.3, 5.991)      # 0.3 N of 60 % inliers: reached by clean samples


def _uneven_batch(ratio, seed0, params):
    from rsc import engine
    rng = np.random.default_rng(seed0)
    scenes = [synth.make_pnp_scene(rng, n, ratio) for n in UNEVEN_N]
    seeds = [seed0 + 1 + i for i in range(len(scenes))]
    gs = [engine.PnPSolver(ctx(), sc, s) for sc, s in zip(scenes, seeds)]
    b = engine.SolverBatch(gs)
    b.set_ransac_parameters(*params)
    return scenes, seeds, gs, b


def test_uneven_chunks_exhaustive():
    """40 % inliers: minInliers is out of reach, every budgeted hypothesis is evaluated and compared."""
    scenes, seeds, gs, b = _uneven_batch(0.4, 4100, UNEVEN_EXHAUSTIVE)
    raw = b.iterate_raw(UNEVEN_BUDGETS)
    recs = [_raw_out(raw[i], gs[i]) for i in range(len(gs))]
    for i, (sc, s) in enumerate(zip(scenes, seeds)):
        o, ro = _oracle(sc, s, UNEVEN_EXHAUSTIVE, UNEVEN_BUDGETS[i])
        assert_pnp_equal(recs[i], ro, f"cand {i}")
        assert not ro["ok"] and recs[i]["iterations"] == ro["iterations"] == UNEVEN_BUDGETS[i]
        ints, _ = _assert_trace(gs[i], o, 4, f"cand {i}")
        assert len(ints) == UNEVEN_BUDGETS[i]


def test_uneven_chunks_with_refine():
    """60 % inliers: hypotheses reach minInliers, so masks are flushed from chunks of unequal size
    and the Refine runs (device-side selection of the small round)."""
    scenes, seeds, gs, b = _uneven_batch(0.6, 4200, UNEVEN_REFINE)
    raw = b.iterate_raw(UNEVEN_BUDGETS)
    recs = [_raw_out(raw[i], gs[i]) for i in range(len(gs))]
    refined = 0
    for i, (sc, s) in enumerate(zip(scenes, seeds)):
        o, ro = _oracle(sc, s, UNEVEN_REFINE, UNEVEN_BUDGETS[i])
        assert_pnp_equal(recs[i], ro, f"cand {i}")
        assert recs[i]["iterations"] == ro["iterations"]
        assert gs[i].state()["max_rows"] == o.info()["max_rows"], f"cand {i} max_rows"
        ints, _ = o.trace()
        refined += int((ints[:, 8] >= o.info()["min_inliers"]).any())
    assert refined >= 3  # qualifying hypotheses (and their Refine) in the 15-, 16- and 33-hypothesis candidates


# ------------------------------------------------------------------------------------------------
# eigen-stage forms
# ------------------------------------------------------------------------------------------------
def test_rows_form_one_solver_iterate5():
    """One solver, iterate(5) rounds of exactly 5 hypotheses (max iterations 1, see UNEVEN_EXHAUSTIVE):
    one eigen workgroup in the rows form and the small betas wave."""
    from rsc import engine
    params = (0.99, 10, 1, 4, 0.5, 5.991)
    rng = np.random.default_rng(4300)
    sc = synth.make_pnp_scene(rng, 300, 0.4)
    g = engine.PnPSolver(ctx(), sc, 77)
    g.set_ransac_parameters(*params)
    o = ol.OraclePnP(sc, 77)
    o.set_ransac_parameters(*params)
    o.enable_trace()
    for rnd in range(3):
        rg, ro = g.iterate(5), o.iterate(5)
        assert_pnp_equal(rg, ro, f"round {rnd}")
        assert rg["iterations"] == ro["iterations"] == 5 * (rnd + 1)
        ints, fl = o.trace()
        cnt, pos = g.last_hypotheses(16)
        assert len(cnt) == 5 and len(ints) == 5 * (rnd + 1)
        assert np.array_equal(cnt, ints[-5:, 8]), f"round {rnd} counts"
        assert np.array_equal(bits(pos), bits(fl[-5:])), f"round {rnd} poses"
        assert np.array_equal(g.last_samples(16)[:, :4], ints[-5:, :4]), f"round {rnd} samples"


_N64 = {}


def _n64_reference():
    """5 solvers x 300 hypotheses at N = 64 and their oracle traces, computed once."""
    if not _N64:
        rng = np.random.default_rng(4400)
        scenes = [synth.make_pnp_scene(rng, 64, 0.4) for _ in range(5)]
        seeds = [4401 + i for i in range(5)]
        refs = []
        for sc, s in zip(scenes, seeds):
            o, ro = _oracle(sc, s, wl.RELOC, 300)
            assert not ro["ok"] and ro["iterations"] == 300
            refs.append((o, ro))
        _N64.update(scenes=scenes, seeds=seeds, refs=refs)
    return _N64["scenes"], _N64["seeds"], _N64["refs"]


@pytest.mark.parametrize("form", ["split", "pairs"])
def test_eigen_forms_above_the_rows_range(form):
    """1,500 hypotheses = 75 eigen workgroups, above the rows form's 64: the split form (default)
    and the pair form.  Pose equality over all 1,500 is also the check of the three-way selection
    on ordinary hypotheses."""
    from rsc import engine
    scenes, seeds, refs = _n64_reference()
    c = engine.Context(0)
    c.set_eig_split(form == "split")
    gs = [engine.PnPSolver(c, sc, s) for sc, s in zip(scenes, seeds)]
    b = engine.SolverBatch(gs)
    b.set_ransac_parameters(*wl.RELOC)
    outs = b.iterate(300, with_masks=True)
    total = 0
    for i, (o, ro) in enumerate(refs):
        assert_pnp_equal(outs[i], ro, f"{form} cand {i}")
        ints, _ = _assert_trace(gs[i], o, 4, f"{form} cand {i}")
        total += len(ints)
    assert total == 1500
    for g in gs:
        g.close()
    c.close()


# ------------------------------------------------------------------------------------------------
# selection among the beta approximations
# ------------------------------------------------------------------------------------------------
def test_selection_with_non_finite_errors():
    """Coplanar points with repeated correspondences (exactly planar, planar up to rounding, and a
    frustum scene with repeats): samples whose approximations end with NaN / inf errors next to
    ordinary ones.  A NaN error never wins over an earlier approximation (`<` is false)."""
    from rsc import engine
    rng = np.random.default_rng(4500)
    scenes = [synth.make_planar_pnp_scene(rng, 200, 0.4, "tilted"), synth.make_planar_pnp_scene(rng, 120, 0.4, "floor"),
              synth.make_planar_pnp_scene(rng, 260, 0.4, "duplicates")]
    for sc in scenes[:2]:  # repeat a quarter of the planar scenes' correspondences too
        n = len(sc.p2d)
        k = n // 4
        src = rng.choice(n - k, size=k)
        for a in (sc.p2d, sc.p3dw, sc.sigma2):
            a[n - k:] = a[src]
    seeds = [4501, 4502, 4503]
    gs = [engine.PnPSolver(ctx(), sc, s) for sc, s in zip(scenes, seeds)]
    b = engine.SolverBatch(gs)
    b.set_ransac_parameters(*wl.RELOC)
    outs = b.iterate(300, with_masks=True)
    n_nan = n_fin = 0
    for i, (sc, s) in enumerate(zip(scenes, seeds)):
        o, ro = _oracle(sc, s, wl.RELOC, 300)
        assert_pnp_equal(outs[i], ro, f"cand {i}")
        _, fl = _assert_trace(gs[i], o, 4, f"cand {i}", nan_ok=True)
        bad = ~np.isfinite(fl).all(1)
        n_nan += int(bad.sum())
        n_fin += int((~bad).sum())
    assert n_nan > 0 and n_fin > 0


# ------------------------------------------------------------------------------------------------
# descriptors of consecutive rounds
# ------------------------------------------------------------------------------------------------
def test_solver_set_changes_between_rounds():
    """Three rounds on one context, 5 -> 3 -> 5 solvers with fresh seeds: a round must not see the
    previous round's problem or launch records."""
    from rsc import engine
    c = engine.Context(0)
    rng = np.random.default_rng(4600)
    scenes = [synth.make_pnp_scene(rng, n, 0.4) for n in (300, 90, 700, 257, 64)]
    gs = [engine.PnPSolver(c, sc, 1) for sc in scenes]
    for g in gs:
        g.set_ransac_parameters(*wl.RELOC)
    for rnd, pick in enumerate([(0, 1, 2, 3, 4), (4, 1, 2), (3, 0, 4, 2, 1)]):
        seeds = [4610 + 10 * rnd + k for k in range(len(pick))]
        for k, s in zip(pick, seeds):
            gs[k].reset(s)
        its = np.array([40 + 7 * k for k in range(len(pick))], np.int32)
        outs = engine.pnp_iterate_many([gs[k] for k in pick], its)
        for j, (k, s) in enumerate(zip(pick, seeds)):
            o, ro = _oracle(scenes[k], s, wl.RELOC, its[j])
            assert_pnp_equal(outs[j], ro, f"round {rnd} slot {j}")
            _assert_trace(gs[k], o, 4, f"round {rnd} slot {j}")
    for g in gs:
        g.close()
    c.close()


def test_blob_size_not_a_multiple_of_the_grid():
    """7 solvers x 35 hypotheses (iterate(30) runs to the 35 of mRansacMaxIts): 14 eigen workgroups (rows form) and a descriptor blob of
    7 problem + 7 launch + 7 selection records, no multiple of 16 B x 14 — every record must arrive."""
    from rsc import engine
    rng = np.random.default_rng(4700)
    scenes = [synth.make_pnp_scene(rng, 100 + 13 * i, 0.4) for i in range(7)]
    seeds = [4701 + i for i in range(7)]
    gs = [engine.PnPSolver(ctx(), sc, s) for sc, s in zip(scenes, seeds)]
    b = engine.SolverBatch(gs)
    b.set_ransac_parameters(*wl.RELOC)
    outs = b.iterate(30, with_masks=True)
    for i, (sc, s) in enumerate(zip(scenes, seeds)):
        o, ro = _oracle(sc, s, wl.RELOC, 30)
        assert_pnp_equal(outs[i], ro, f"cand {i}")
        _assert_trace(gs[i], o, 4, f"cand {i}")
