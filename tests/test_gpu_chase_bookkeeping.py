"""The split eigen stage's chase wave with tridiag_qr's mirror() / any_lane() hooks (indexed reads of
the (diag, sub) slab instead of select chains; deflation tests trimmed to the ranges some lane still
needs), forced onto small launches (set_eig_rows(0), set_eig_split(True)) whose hypothesis counts sit
on the edges of the split kernel's layout: a unit is 20 hypotheses, a workgroup 4 units.  Every
hypothesis against the oracle trace (samples, counts, poses with NaN-aware bit equality), as
test_gpu_variants.py::test_eig_rows_every_hypothesis; the lane-pair form (whose sink has no hooks) on
the same inputs gives the same bits."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
from rsc import synth

pytestmark = pytest.mark.gpu

HYPS = [1, 19, 20, 21, 79, 80, 81]  # below / at / above one unit and one workgroup
CORRS = [40, 133, 230]              # correspondences per candidate


def _nan_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _params(ms, hyps):
    return (0.99, 10, hyps, ms, 0.5, 5.991)  # at most 45 % inliers: minInliers N/2 unreachable


@pytest.fixture(scope="module")
def ctxs():
    from rsc import engine
    out = {}
    for form in ("split", "pairs"):
        c = engine.Context(0)
        c.set_eig_rows(0)  # no launch in the rows form
        c.set_eig_split(form == "split")
        out[form] = c
    yield out
    for c in out.values():
        c.close()


@functools.lru_cache(maxsize=None)
def _scenes(ms):
    rng = np.random.default_rng(7100 + ms)
    sc = [synth.make_pnp_scene(rng, CORRS[0], 0.4), synth.make_pnp_scene(rng, CORRS[1], 0.35),
          synth.make_planar_pnp_scene(rng, 120, 0.4, "floor"),  # coplanar samples: NaN blocks in the chase
          synth.make_pnp_scene(rng, CORRS[2], 0.45)]
    return sc, [61 + i for i in range(len(sc))]


@functools.lru_cache(maxsize=None)
def _oracle(ms, cand, hyps):
    """(samples, counts, poses) of the first `hyps` hypotheses of candidate `cand`."""
    scenes, seeds = _scenes(ms)
    o = ol.OraclePnP(scenes[cand], seeds[cand])
    o.set_ransac_parameters(*_params(ms, hyps))
    o.enable_trace()
    ro = o.iterate(hyps)
    assert not ro["ok"] and ro["iterations"] == hyps
    ints, fl = o.trace()
    assert len(ints) == hyps
    return ints, fl


def _run(ctx, ms, cands, hyps):
    """One launch set: candidate cands[i] runs hyps[i] hypotheses; returns (counts, poses, samples) each."""
    from rsc import engine
    scenes, seeds = _scenes(ms)
    gs = [engine.PnPSolver(ctx, scenes[c], seeds[c]) for c in cands]
    for g, h in zip(gs, hyps):
        g.set_ransac_parameters(*_params(ms, h))
    engine.SolverBatch(gs).iterate(np.asarray(hyps, np.int32))
    out = []
    for g in gs:
        cnt, pos = g.last_hypotheses(128)
        out.append((cnt, pos, g.last_samples(128)))
        g.close()
    return out


def _check(ms, cands, hyps, ctxs):
    got = {form: _run(ctxs[form], ms, cands, hyps) for form in ("split", "pairs")}
    for i, (c, h) in enumerate(zip(cands, hyps)):
        ints, fl = _oracle(ms, c, h)
        for form in ("split", "pairs"):
            cnt, pos, smp = got[form][i]
            tag = f"{form} ms={ms} cand {c} hyps {h}"
            assert len(cnt) == h, tag
            assert np.array_equal(smp[:, :ms], ints[:, :ms]), tag + " samples"
            assert np.array_equal(cnt, ints[:, 8]), tag + " counts"
            assert _nan_equal(pos, fl), tag + " poses"
        assert _nan_equal(got["split"][i][1], got["pairs"][i][1]), f"split vs pairs ms={ms} cand {c}"
        assert np.array_equal(got["split"][i][0], got["pairs"][i][0]), f"split vs pairs ms={ms} cand {c}"


@pytest.mark.parametrize("hyps", HYPS)
@pytest.mark.parametrize("ms", [4, 5, 6])
def test_unit_and_workgroup_edges(ms, hyps, ctxs):
    _check(ms, [0, 1, 2, 3], [hyps] * 4, ctxs)


@pytest.mark.parametrize("ms", [4, 5, 6])
def test_mixed_launch_with_empty_units(ms, ctxs):
    # 1 + 5 units: the second workgroup holds two units and two empty ones
    _check(ms, [2, 1], [1, 81], ctxs)
    _check(ms, [3, 2], [81, 1], ctxs)
