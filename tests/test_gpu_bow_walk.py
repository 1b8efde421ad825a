"""GPU parity of ORBmatcher::SearchByBoW on the adversarial cases of tests/bow_walk_cases.py
(contested nodes, rescans, exact thresholds and ties, float32 ratio edges, thousands of nodes,
orientation histograms on the 10 % rule): engine.BowSearch against the oracle, match vectors and
counts bit-exact.  tests/test_cpu_bow_walk.py shows what these inputs make the reference do and that
single wrong rules change their outputs; the random views of tests/test_gpu_orbmatch.py cannot.

Every group runs its pairs of an overload in one batch, pairs of different inner size classes side
by side; views are uploaded once per module."""
import copy

import numpy as np
import pytest

import bow_walk_cases as bc
import oracle_lib as ol
from gpu_common import ctx
from rsc import engine

pytestmark = pytest.mark.gpu

_views = {}


def views(v):
    """(device view, oracle view) of a case view, made once."""
    if id(v) not in _views:
        _views[id(v)] = (v, engine.BowView(ctx(), v), ol.OracleBow(v))
    return _views[id(v)][1:]


def check_batch(b, nnratio, check, order=None):
    order = list(range(len(b.others))) if order is None else order
    gs, osh = views(b.shared)
    go, oo = zip(*[views(b.others[k]) for k in order])
    g_out, g_nm = engine.BowSearch(ctx(), gs, list(go), b.frame, nnratio, check).run()
    o_out, o_nm = ol.search_by_bow_many(b.frame, list(oo), osh, nnratio, check)
    where = (b.name, nnratio, check, [b.labels[k] for k in order])
    assert np.array_equal(g_nm, o_nm), (where, g_nm, o_nm)
    for k, row in enumerate(order):
        bad = np.flatnonzero(g_out[k] != o_out[k])
        assert bad.size == 0, (where, b.labels[row], bad[:8], g_out[k][bad[:8]], o_out[k][bad[:8]])
    return g_out.copy(), g_nm.copy()


def check_group(group):
    total = 0
    for b in bc.batches(group):
        for r in b.ratios:
            for check in b.checks:
                total += int(check_batch(b, r, check)[1].sum())
    return total


def test_size_classes():
    """Contested clustered nodes of every inner size class (matched-set representation, segment
    count, LDS staging), every ratio, orientation check on and off."""
    assert check_group("size") > 1000


def test_exact_distances():
    """d1 in {49, 50, 51}, equal first minima across the 64 / segment / staging boundaries, d1 = d2,
    and every (d1, d2) on the float32 ratio boundary."""
    assert check_group("exact") > 1000


def test_many_nodes():
    """255 .. 8192 outer nodes (one and several nodes per thread of the join kernel, walk grids in
    the thousands), half the node ids shared, wide nodes in between."""
    assert check_group("many") > 1000


def test_orientation():
    """Four populated bins, the third maximum on either side of the 10 % rule."""
    for b in bc.batches("ori"):
        _, nm = check_batch(b, 0.9, True)
        _, raw = check_batch(b, 0.9, False)
        for (keep, plan), n, t in zip(b.meta, nm, raw):
            assert t == sum(plan) and n == t - plan[3] - (0 if keep else plan[2])


def test_batch_order_independence():
    """The same pairs in reversed order: every pair's result is the same."""
    for group in ("size", "many"):
        for b in bc.batches(group):
            fwd, fnm = check_batch(b, 0.9, True)
            order = list(range(len(b.others)))[::-1]
            rev, rnm = check_batch(b, 0.9, True, order)
            assert np.array_equal(fnm, rnm[::-1]) and np.array_equal(fwd, rev[::-1])


def test_set_valid_on_contested_nodes():
    """KeyFrame overload: the hot inner features of the contested 65-256 nodes lose and regain their
    map points between searches."""
    b = bc.batches("size")[1]
    k = b.labels.index("65-256")
    inner = copy.copy(b.others[k])
    hot = []
    for node in b.nodes[k]:
        j = int(np.flatnonzero(inner.node_id == node.id)[0])
        feats = inner.feat[inner.node_begin[j]:inner.node_begin[j + 1]]
        hot += [int(f) for f in feats[node.hot[0]]]  # one of the two hot groups of every node
    g_outer, o_outer = views(b.shared)
    g_inner = engine.BowView(ctx(), inner)
    results = []
    for drop in (False, True, False):
        inner.valid = b.others[k].valid.copy()
        if drop:
            inner.valid[hot] = 0
        g_inner.set_valid(inner.valid)
        out, nm = engine.BowSearch(ctx(), g_outer, [g_inner], False, 0.9, True).run()
        o_nm, o_out = ol.search_by_bow(False, o_outer, ol.OracleBow(inner), 0.9, True)
        assert nm[0] == o_nm and np.array_equal(out[0], o_out), drop
        results.append(out[0].copy())
    assert np.array_equal(results[0], results[2]) and not np.array_equal(results[0], results[1])
    assert not np.isin(results[1], hot).any()
