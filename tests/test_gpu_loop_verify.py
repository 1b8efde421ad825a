"""The closing stage of LoopClosing::ComputeSim3 on the device (rsc_loop_verify_many) after the gated loop
events (rsc_loop_events_gated): the synthetic event of tests/loop_verify_cases.py with three mvpLoopMapPoints
lists in one launch — 39 matches (rejected), 40 (accepted) and the full list — against the restatement
(tests/kfproj_ref.loop_verify), bit for bit."""
import numpy as np
import pytest

import loop_verify_cases as lv
from gpu_common import ctx
from rsc import events as rev

pytestmark = pytest.mark.gpu


def test_gate_then_verify():
    from rsc import engine
    b = lv.build()
    v1 = engine.KFView(ctx(), b.kf1)
    v2s = [engine.KFView(ctx(), kf2) for kf2, _, _ in b.cands]
    solvers = [[engine.Sim3Solver(ctx(), pair, s) for (_, _, pair), s in zip(b.cands, b.seeds)]]
    eb = engine.EventBatch(solvers)
    eb.batch.reset(np.array(b.seeds, np.uint32))
    eb.batch.set_ransac_parameters(*rev.LOOP_PARAMS)
    res, matches = eb.run_loop_gated([[(v1, v2, m12) for v2, (_, m12, _) in zip(v2s, b.cands)]])
    g = res[0]
    assert int(g["status"]) == 1 and int(g["winner"]) == b.gate["winner"]
    assert np.array_equal(np.asarray(g["S"]).view(np.uint64), np.asarray(b.gate["S"]).view(np.uint64))
    assert np.array_equal(matches[0], b.gate["matches"])
    vm = v2s[int(g["winner"])]
    k = len(b.lists)
    mps = [engine.MPView(ctx(), p) for p, _, _ in b.lists]
    out, projected = engine.loop_verify_many(ctx(), [v1] * k, [vm] * k, mps, [np.asarray(g["S"])] * k,
                                             [matches[0]] * k, [a for _, a, _ in b.lists])
    for c, (p, a, exp) in enumerate(b.lists):
        r = out[c]
        assert (r.accepted, r.n_projected, r.n_total) == (exp["accepted"], exp["n_projected"], exp["n_total"]), c
        assert np.array_equal(np.array(r.Scw_sim3[:]).view(np.uint64), exp["Scw_sim3"].view(np.uint64)), c
        assert np.array_equal(np.array(r.Scw[:], np.float32).view(np.uint32), exp["Scw"].view(np.uint32)), c
        assert np.array_equal(projected[c], exp["projected"]), c
    assert [out[c].n_total for c in range(2)] == [39, 40] and [out[c].accepted for c in range(3)] == [0, 1, 1]
    # projected may be NULL
    L = engine.load_library()
    one = (engine.LoopVerifyResult * 1)()
    Sd = np.ascontiguousarray(np.asarray(g["S"], np.float64).reshape(1, 8))
    m0 = np.ascontiguousarray(matches[0], np.int32)
    a0 = np.ascontiguousarray(b.lists[1][1], np.uint8)
    assert L.rsc_loop_verify_many(ctx().h, engine._handles([v1]), engine._handles([vm]), engine._handles([mps[1]]), 1,
                                  Sd, engine._ptrs([m0]), engine._ptrs([a0]), one, None) == 0
    assert one[0].n_total == 40 and one[0].accepted == 1
