"""Where the argument path of the PnP round must fall back to the blob path, and where its resident
problem table must be refreshed.  Every scenario runs under the default setting and with the switch off
(rsc_context_set_round_args): the two must agree byte for byte (result records, samples, counts, poses
of every round) and the default one is checked against the oracle.  The counters of
rsc_diag_round_paths (rounds on the argument path, rounds on the blob path, uploads of the resident
table) are asserted per round, so a fall-back cannot hide as a pass and a missing refresh cannot hide
behind a table that happens to be right.

* C = capacity (64) and capacity + 1 solvers at N = 8, H = 2: the larger round takes the blob path;
* a solver whose rand() window has moved: 4,000 hypotheses at N = 8 (16,000 draws of the table's
  16,394 from a seed window) on the argument path, the next call moves the window: blob path;
* a solver bound to a shared stream: blob path whatever the setting;
* consecutive rounds with an unchanged table (no upload), a changed th2 (in the table: one upload), a
  minInliers changed from 30 to 29, still out of reach (it travels in the round's records, not in the table:
  exactly one round on the argument path and no upload), and a minInliers low enough for a solver to
  succeed (the result changes with it; its Refine may upload);
* rounds after a failed and after a successful Refine (iterate(5) x 20 on two scenes whose Refine fails
  at least once): the rows of the EPnP buffers change, the table is uploaded again;
* a solver set that changes between rounds (5 -> 3 -> 5 with fresh seeds): one upload per round."""
import numpy as np
import pytest

from gpu_common import REFINE_FAIL_CASES, assert_pnp_equal, refine_fail_scene
import oracle_lib as ol
from rsc import synth
from rsc import workloads as wl

pytestmark = pytest.mark.gpu

CAP = 64  # rsc_kernels.h kRoundArgsCap


def _nan_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


class Log:
    """What a scenario leaves per round: the solvers' records and the path counters' increments."""

    def __init__(self, c):
        self.c, self.rounds = c, []

    def round(self, gs, outs, cap=64):
        after = self.c.round_paths()
        recs = []
        for g, o in zip(gs, outs):
            cnt, pos = g.last_hypotheses(cap)
            recs.append(dict(out=o, smp=g.last_samples(cap).copy(), cnt=cnt.copy(), pos=pos.copy(), state=g.state()))
        self.rounds.append((recs, {k: after[k] - self.before[k] for k in after}))

    def mark(self):
        self.before = self.c.round_paths()


def _both(scenario):
    """The scenario under both settings, on a context of its own: its resident table starts empty, so the
    upload counts do not depend on what earlier tests left behind."""
    from rsc import engine
    c = engine.Context(0)
    logs = []
    try:
        for on in (True, False):
            c.set_round_args(on)
            log = Log(c)
            scenario(c, log)
            logs.append(log)
    finally:
        c.close()
    a, b = logs
    assert len(a.rounds) == len(b.rounds)
    for r, ((ra, _), (rb, db)) in enumerate(zip(a.rounds, b.rounds)):
        assert db["args"] == 0 and db["table_uploads"] == 0 and db["blob"] >= 1, f"round {r} with the switch off: {db}"
        for i, (x, y) in enumerate(zip(ra, rb)):
            where = f"round {r} solver {i}"
            assert np.array_equal(x["smp"], y["smp"]) and np.array_equal(x["cnt"], y["cnt"]), where
            assert x["pos"].tobytes() == y["pos"].tobytes(), f"{where} poses"
            assert x["state"] == y["state"], f"{where} state"
            for k in ("ok", "no_more", "n_inliers", "iterations"):
                assert x["out"][k] == y["out"][k], f"{where} {k}"
            assert x["out"]["T"].tobytes() == y["out"]["T"].tobytes(), f"{where} T"
            assert np.array_equal(x["out"]["inliers"], y["out"]["inliers"]), f"{where} inliers"
    return a.rounds


def _oracle_round(o, its, rec, ms, where):
    """One iterate(its) of the oracle against the solver's record of that round: the result, and every
    hypothesis of an exhaustive call (one launch) against the call's trace."""
    n0 = len(o.trace()[0]) if o.traced else 0
    ro = o.iterate(int(its))
    assert_pnp_equal(rec["out"], ro, where)
    assert rec["out"]["iterations"] == ro["iterations"], f"{where} iterations"
    ints, fl = o.trace()
    ints, fl = ints[n0:], fl[n0:]  # this call's hypotheses
    if ro["ok"] or len(ints) != its or (ints[:, 8] >= o.info()["min_inliers"]).any():
        return ro  # a Refine ran: launches after it start anew, the result and the iterations are the check
    assert len(rec["cnt"]) == its, f"{where} hypotheses {len(rec['cnt'])} vs {its}"
    assert np.array_equal(rec["smp"][:, :ms], ints[:, :ms]), f"{where} samples vs oracle"
    assert np.array_equal(rec["cnt"], ints[:, 8]), f"{where} counts vs oracle"
    assert _nan_equal(rec["pos"], fl), f"{where} poses vs oracle"
    return ro


def _oracle(sc, seed, params):
    o = ol.OraclePnP(sc, int(seed))
    o.set_ransac_parameters(*params)
    o.enable_trace()
    o.traced = True
    return o


# ------------------------------------------------------------------------------------------------
# capacity
# ------------------------------------------------------------------------------------------------
SMALL = (0.99, 8, 1, 4, 0.5, 5.991)  # N = 8 with outliers: minInliers 8 is out of reach, exactly n hypotheses


@pytest.mark.parametrize("count", [CAP, CAP + 1])
def test_capacity_and_one_more(count):
    from rsc import engine
    rng = np.random.default_rng(9300)
    scenes = [synth.make_pnp_scene(rng, 8, 0.4) for _ in range(count)]
    seeds = [9301 + 7 * i for i in range(count)]

    def scenario(c, log):
        gs = [engine.PnPSolver(c, sc, s) for sc, s in zip(scenes, seeds)]
        for g in gs:
            g.set_ransac_parameters(*SMALL)
        log.mark()
        log.round(gs, engine.pnp_iterate_many(gs, 2))
        for g in gs:
            g.close()

    (recs, d), = _both(scenario)
    if count <= CAP:
        assert d == dict(args=1, blob=0, table_uploads=1), d
    else:
        assert d == dict(args=0, blob=1, table_uploads=0), d
    for i in range(count):
        _oracle_round(_oracle(scenes[i], seeds[i], SMALL), 2, recs[i], 4, f"C {count} solver {i}")


# ------------------------------------------------------------------------------------------------
# moved window, shared stream
# ------------------------------------------------------------------------------------------------
def test_window_moved_past_the_tables_reach():
    from rsc import engine
    rng = np.random.default_rng(9400)
    sc = synth.make_pnp_scene(rng, 8, 0.4)

    def scenario(c, log):
        g = engine.PnPSolver(c, sc, 9401)
        g.set_ransac_parameters(*SMALL)
        for its in (4000, 200, 7):
            log.mark()
            log.round([g], [g.iterate(its)], cap=4096)
        g.close()

    rounds = _both(scenario)
    # 310 + 16,000 draws fit the table's 16,704 rows; 800 more do not: the window moves and stays moved
    assert rounds[0][1] == dict(args=1, blob=0, table_uploads=1), rounds[0][1]
    assert rounds[1][1] == dict(args=0, blob=1, table_uploads=0), rounds[1][1]
    assert rounds[2][1] == dict(args=0, blob=1, table_uploads=0), rounds[2][1]
    o = _oracle(sc, 9401, SMALL)
    for r, its in enumerate((4000, 200, 7)):
        _oracle_round(o, its, rounds[r][0][0], 4, f"round {r}")
        assert len(rounds[r][0][0]["cnt"]) == its


def test_solver_bound_to_a_shared_stream():
    from rsc import engine
    rng = np.random.default_rng(9500)
    scenes = [synth.make_pnp_scene(rng, 8, 0.4) for _ in range(2)]

    def scenario(c, log):
        st = engine.Stream(c, 1)
        gs = [engine.PnPSolver(c, sc, 99) for sc in scenes]
        for g in gs:
            g.set_ransac_parameters(*SMALL)
            g.bind_stream(st)
        for _ in range(2):
            for g in gs:
                log.mark()
                log.round([g], [g.iterate(3)])
        for g in gs:
            g.bind_stream(None)
            g.close()
        st.close()

    rounds = _both(scenario)
    for _, d in rounds:
        assert d == dict(args=0, blob=1, table_uploads=0), d
    os_ = [ol.OraclePnP(sc, 99) for sc in scenes]
    for o in os_:
        o.set_ransac_parameters(*SMALL)
        o.use_libc_rand()
    ol.libc_srand(1)
    k = 0
    for _ in range(2):
        for o in os_:
            ro = o.iterate(3)
            rec = rounds[k][0][0]
            assert_pnp_equal(rec["out"], ro, f"call {k}")
            assert rec["out"]["iterations"] == ro["iterations"]
            k += 1


# ------------------------------------------------------------------------------------------------
# table refreshes
# ------------------------------------------------------------------------------------------------
def test_changed_th2_and_min_inliers_between_rounds():
    from rsc import engine
    rng = np.random.default_rng(9600)
    scenes = [synth.make_pnp_scene(rng, n, 0.6) for n in (70, 40, 33)]
    seeds = [9601, 9602, 9603]
    steps = [(0.99, 30, 1, 4, 0.9, 5.991),   # minInliers out of reach
             (0.99, 30, 1, 4, 0.9, 5.991),   # the same again: nothing to upload
             (0.99, 30, 1, 4, 0.9, 0.25),    # th2 is in the table
             (0.99, 29, 1, 4, 0.9, 0.25),    # minInliers alone, still out of reach: records only, no upload
             (0.99, 5, 1, 4, 0.3, 0.25)]     # within reach: a solver succeeds (its Refine changes the rows)

    def scenario(c, log):
        gs = [engine.PnPSolver(c, sc, s) for sc, s in zip(scenes, seeds)]
        for params in steps:
            for g, s in zip(gs, seeds):
                g.reset(s)
                g.set_ransac_parameters(*params)
            log.mark()
            log.round(gs, engine.pnp_iterate_many(gs, 21))
        for g in gs:
            g.close()

    rounds = _both(scenario)
    assert rounds[0][1] == dict(args=1, blob=0, table_uploads=1), rounds[0][1]
    assert rounds[1][1] == dict(args=1, blob=0, table_uploads=0), rounds[1][1]
    assert rounds[2][1] == dict(args=1, blob=0, table_uploads=1), rounds[2][1]
    assert rounds[3][1] == dict(args=1, blob=0, table_uploads=0), rounds[3][1]
    assert rounds[4][1]["blob"] == 0 and rounds[4][1]["args"] >= 1, rounds[4][1]
    changed = 0
    for r, params in enumerate(steps):
        for i in range(3):
            ro = _oracle_round(_oracle(scenes[i], seeds[i], params), 21, rounds[r][0][i], 4, f"step {r} solver {i}")
            if r == 2:
                changed += int(not np.array_equal(rounds[2][0][i]["cnt"], rounds[1][0][i]["cnt"]))
            if r == 3:  # the solver's threshold is max(minInliers, int(N * epsilon), minSet) in float: 63, 36, 29
                want = max(29, int(np.float32(scenes[i].n) * np.float32(0.9)))
                assert rounds[3][0][i]["state"]["min_inliers"] == want, (i, rounds[3][0][i]["state"])
                if i == 2:  # N = 33: the one whose threshold the step really changed
                    assert rounds[2][0][i]["state"]["min_inliers"] == 30 and want == 29
            if r == 4:
                changed += int(ro["ok"])
    assert changed >= 2  # the tighter th2 changed counts, the lower minInliers let a solver succeed


@pytest.mark.parametrize("case", REFINE_FAIL_CASES[:2])
def test_rounds_after_failed_and_successful_refines(case):
    from rsc import engine
    sc, seed = refine_fail_scene(case)

    def scenario(c, log):
        g = engine.PnPSolver(c, sc, seed)
        g.set_ransac_parameters(*wl.RELOC)
        for _ in range(20):
            log.mark()
            log.round([g], [g.iterate(5)])
        g.close()

    rounds = _both(scenario)
    assert len(rounds) == 20
    o = ol.OraclePnP(sc, seed)
    o.set_ransac_parameters(*wl.RELOC)
    # iterate() begins with set_maximum_number_of_correspondences(mRansacMinSet): the first launch sees 4 rows
    rows_at_start, uploads, refreshed, quiet = [4], 0, 0, 0
    for r, (recs, d) in enumerate(rounds):
        ro = o.iterate(5)
        assert_pnp_equal(recs[0]["out"], ro, f"round {r}")
        assert recs[0]["out"]["iterations"] == ro["iterations"], f"round {r}"
        assert recs[0]["state"]["max_rows"] == o.info()["max_rows"], f"round {r} max_rows"
        assert d["blob"] == 0, (r, d)  # 400 draws: the window never moves
        # A Refine (failed or successful) of round r - 1 left other rows than that round started with: round
        # r's first launch, at the latest, finds a changed table.  These intervals do not overlap, so each
        # needs an upload of its own, beside the first round's.
        if r > 0 and d["args"] >= 1 and rows_at_start[r] != rows_at_start[r - 1]:
            refreshed += 1
        uploads += d["table_uploads"]
        rows_at_start.append(recs[0]["state"]["max_rows"])
        # no Refine in the round before (rows as that round found them) and none in this one: the table is the
        # one the device holds, whatever the round's outcome — a build that uploads every round fails here
        if r > 0 and rows_at_start[r - 1] == rows_at_start[r] == rows_at_start[r + 1]:
            assert d["table_uploads"] == 0, (r, d, rows_at_start)
            quiet += 1
    assert rounds[0][1]["table_uploads"] >= 1
    assert refreshed >= 1 and uploads >= 1 + refreshed, (refreshed, uploads, rows_at_start)
    assert quiet >= 5, (quiet, rows_at_start)


def test_solver_set_changes_between_rounds():
    from rsc import engine
    rng = np.random.default_rng(9700)
    scenes = [synth.make_pnp_scene(rng, n, 0.4) for n in (70, 12, 40, 25, 64)]
    picks = [(0, 1, 2, 3, 4), (4, 1, 2), (3, 0, 4, 2, 1)]

    def scenario(c, log):
        gs = [engine.PnPSolver(c, sc, 1) for sc in scenes]
        for g in gs:
            g.set_ransac_parameters(*SMALL[:2], 1, 4, 0.9, 5.991)
        for rnd, pick in enumerate(picks):
            for j, k in enumerate(pick):
                gs[k].reset(9710 + 10 * rnd + j)
            log.mark()
            log.round([gs[k] for k in pick], engine.pnp_iterate_many([gs[k] for k in pick], 8 + rnd))
        for g in gs:
            g.close()

    rounds = _both(scenario)
    params = (SMALL[0], SMALL[1], 1, 4, 0.9, 5.991)
    for rnd, pick in enumerate(picks):
        assert rounds[rnd][1] == dict(args=1, blob=0, table_uploads=1), (rnd, rounds[rnd][1])
        for j, k in enumerate(pick):
            _oracle_round(_oracle(scenes[k], 9710 + 10 * rnd + j, params), 8 + rnd, rounds[rnd][0][j], 4,
                          f"round {rnd} slot {j}")
