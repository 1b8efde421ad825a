"""The two descriptor paths of the PnP speculation round, in one process through
rsc_context_set_round_args: the argument path (default: per-solver records in the kernels' argument
blocks, the rand() window worked out from the seed on the device, the problem table resident) and
the blob path (every round uploads problems + launch records with their 31-word windows) must agree
byte for byte — every hypothesis' sample (rsc_pnp_last_samples), inlier count and float pose
(rsc_pnp_last_hypotheses) and the result records — and the argument path is checked against the
oracle's trace the way tests/test_gpu_pnp_round.py does.

Shapes: N in {12, 70} correspondences, H in {8, 21} hypotheses per solver, C in {1, 3} solvers; the
three solvers have min_set 4, 5 and 6 (three eigen-stage groups in one round; a single solver takes
each in turn over the cases); exhaustive scenes (40 % inliers, minInliers out of reach) and scenes
whose hypotheses qualify, so the fused select / Refine kernel runs with its records as arguments too.
Seeds from the closed form's edge list (0, 1, 2, 127773, 2^31 - 2, 2^31 - 1, 2^31, 2^31 + 1,
2^32 - 1), every one used.  These rounds are small, so their eigen stage runs in the rows form; a round of
1,290 hypotheses with the rows form switched off runs the three sample sizes in the split and in the pair
form.  The counters of rsc_diag_round_paths say which path a round took, so a
silent fall-back cannot pass as parity."""
import itertools

import numpy as np
import pytest

from gpu_common import assert_pnp_equal, ctx
import oracle_lib as ol
from rsc import synth

pytestmark = pytest.mark.gpu

EDGE_SEEDS = [0, 1, 2, 127773, 2**31 - 2, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 1]
CASES = list(itertools.product((12, 70), (8, 21), (1, 3), ("exhaustive", "refine")))


def _params(kind, ms):
    # max iterations 1: iterate(n) runs exactly n hypotheses unless it succeeds (the reference's `||`)
    return (0.99, 10, 1, ms, 0.5, 5.991) if kind == "exhaustive" else (0.99, 6, 1, ms, 0.3, 5.991)


def _nan_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _run(c, on, scenes, seeds, sets, H):
    """One round of the solvers under the given path: results, samples, hypotheses, path counters."""
    from rsc import engine
    c.set_round_args(on)
    before = c.round_paths()
    gs = [engine.PnPSolver(c, sc, s) for sc, s in zip(scenes, seeds)]
    for g, (kind, ms) in zip(gs, sets):
        g.set_ransac_parameters(*_params(kind, ms))
    outs = engine.pnp_iterate_many(gs, H)
    rec = []
    for g, o in zip(gs, outs):
        cnt, pos = g.last_hypotheses(64)
        rec.append(dict(out=o, smp=g.last_samples(64).copy(), cnt=cnt.copy(), pos=pos.copy(), state=g.state()))
        g.close()
    after = c.round_paths()
    return rec, {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("case", range(len(CASES)))
def test_paths_agree_and_match_the_oracle(case):
    N, H, C, kind = CASES[case]
    rng = np.random.default_rng(9100 + case)
    ratio = 0.4 if kind == "exhaustive" else 0.8
    scenes = [synth.make_pnp_scene(rng, N, ratio) for _ in range(C)]
    seeds = [EDGE_SEEDS[(4 * case + i) % len(EDGE_SEEDS)] for i in range(C)]
    sets = [(kind, 4 + (i if C == 3 else case % 3)) for i in range(C)]
    c = ctx()
    try:
        a, da = _run(c, True, scenes, seeds, sets, H)
        b, db = _run(c, False, scenes, seeds, sets, H)
    finally:
        c.set_round_args(True)
    assert da["args"] >= 1 and da["blob"] == 0, da
    assert db["blob"] >= 1 and db["args"] == 0 and db["table_uploads"] == 0, db
    for i in range(C):
        where = f"N {N} H {H} C {C} {kind} solver {i} seed {seeds[i]}"
        ms = sets[i][1]
        ra, rb = a[i], b[i]
        # byte equality of the two paths
        assert np.array_equal(ra["smp"], rb["smp"]), f"{where} samples"
        assert np.array_equal(ra["cnt"], rb["cnt"]), f"{where} counts"
        assert ra["pos"].tobytes() == rb["pos"].tobytes(), f"{where} poses"
        assert ra["state"] == rb["state"], f"{where} state"
        oa, ob = ra["out"], rb["out"]
        for k in ("ok", "no_more", "n_inliers", "iterations"):
            assert oa[k] == ob[k], f"{where} {k}"
        assert oa["T"].tobytes() == ob["T"].tobytes() and np.array_equal(oa["inliers"], ob["inliers"]), f"{where} T"
        # the argument path against the oracle
        o = ol.OraclePnP(scenes[i], int(seeds[i]))
        o.set_ransac_parameters(*_params(kind, ms))
        o.enable_trace()
        ro = o.iterate(H)
        assert_pnp_equal(oa, ro, where)
        assert oa["iterations"] == ro["iterations"], where
        assert ra["state"]["max_rows"] == o.info()["max_rows"], f"{where} max_rows"
        if kind == "refine":
            continue  # launches after a Refine start anew: the result, the rows and the iterations are the check
        ints, fl = o.trace()
        assert len(ra["cnt"]) == len(ints) == H, f"{where} hypotheses {len(ra['cnt'])} vs {len(ints)}"
        assert np.array_equal(ra["smp"][:, :ms], ints[:, :ms]), f"{where} samples vs oracle"
        assert np.array_equal(ra["cnt"], ints[:, 8]), f"{where} counts vs oracle"
        assert _nan_equal(ra["pos"], fl), f"{where} poses vs oracle"


@pytest.mark.parametrize("form", ["split", "pairs"])
def test_large_round_in_the_split_and_pair_forms(form):
    """3 solvers x 430 hypotheses = 1,290, min_set 4, 5 and 6, with the rows form switched off: every
    sample size's eigen stage runs in the split form (pnp_eig_split_kernel, the headline's) or in the pair
    form (pnp_eig_group_kernel) with the argument block, against the blob path and the oracle."""
    from rsc import engine
    H = 430
    rng = np.random.default_rng(9200)
    scenes = [synth.make_pnp_scene(rng, 70, 0.4) for _ in range(3)]
    seeds = [EDGE_SEEDS[8], EDGE_SEEDS[0], EDGE_SEEDS[6]]
    c = engine.Context(0)
    c.set_eig_rows(0)
    c.set_eig_split(form == "split")
    runs = {}
    try:
        for on in (True, False):
            c.set_round_args(on)
            before = c.round_paths()
            gs = [engine.PnPSolver(c, sc, s) for sc, s in zip(scenes, seeds)]
            for i, g in enumerate(gs):
                g.set_ransac_parameters(*_params("exhaustive", 4 + i))
            outs = engine.pnp_iterate_many(gs, H)
            recs = []
            for g, o in zip(gs, outs):
                cnt, pos = g.last_hypotheses(512)
                recs.append(dict(out=o, smp=g.last_samples(512).copy(), cnt=cnt.copy(), pos=pos.copy()))
                g.close()
            after = c.round_paths()
            runs[on] = (recs, {k: after[k] - before[k] for k in after})
    finally:
        c.close()
    assert runs[True][1] == dict(args=1, blob=0, table_uploads=1), runs[True][1]
    assert runs[False][1] == dict(args=0, blob=1, table_uploads=0), runs[False][1]
    for i in range(3):
        where, ms = f"{form} solver {i} seed {seeds[i]}", 4 + i
        ra, rb = runs[True][0][i], runs[False][0][i]
        assert np.array_equal(ra["smp"], rb["smp"]) and np.array_equal(ra["cnt"], rb["cnt"]), f"{where} paths"
        assert ra["pos"].tobytes() == rb["pos"].tobytes(), f"{where} poses of the paths"
        o = ol.OraclePnP(scenes[i], int(seeds[i]))
        o.set_ransac_parameters(*_params("exhaustive", ms))
        o.enable_trace()
        ro = o.iterate(H)
        assert_pnp_equal(ra["out"], ro, where)
        ints, fl = o.trace()
        assert len(ra["cnt"]) == len(ints) == H and not ro["ok"], where
        assert np.array_equal(ra["smp"][:, :ms], ints[:, :ms]), f"{where} samples vs oracle"
        assert np.array_equal(ra["cnt"], ints[:, 8]), f"{where} counts vs oracle"
        assert _nan_equal(ra["pos"], fl), f"{where} poses vs oracle"


def test_every_edge_seed_is_used():
    used = set()
    for case, (N, H, C, kind) in enumerate(CASES):
        used.update(EDGE_SEEDS[(4 * case + i) % len(EDGE_SEEDS)] for i in range(C))
    assert used == set(EDGE_SEEDS)
