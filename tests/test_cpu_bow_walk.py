"""The adversarial SearchByBoW cases (tests/bow_walk_cases.py) are what they claim, on the CPU:

* the numpy restatement (tests/bow_walk_census.py) equals the C oracle on every case: vector and
  count, both overloads, orientation check on and off, every ratio;
* the census of the size-class cases (properties of the inputs and the reference alone) shows, per
  inner size class and overload, contested nodes: rescan-condition features, stolen nearest
  neighbours, both outcomes of the ratio test and features on its boundary;
* every perturbation (a)-(h) of the restatement changes the output vector of some case in every
  size class where it applies, which is what makes the device test (tests/test_gpu_bow_walk.py)
  sensitive to that class of error.
"""
import collections

import numpy as np
import pytest

import bow_walk_cases as bc
import bow_walk_census as cz
import oracle_lib as ol

_oracle_views = {}


def oracle_view(v):
    if id(v) not in _oracle_views:
        _oracle_views[id(v)] = (v, ol.OracleBow(v))
    return _oracle_views[id(v)][1]


@pytest.mark.parametrize("group", ["size", "exact", "many", "ori"])
def test_restatement_equals_oracle(group):
    for b in bc.batches(group):
        for lab, A, B in b.pairs():
            for r in b.ratios:
                for check in b.checks:
                    nm, out, _ = cz.walk(b.frame, A, B, r, check)
                    onm, oout = ol.search_by_bow(b.frame, oracle_view(A), oracle_view(B), r, check)
                    assert nm == onm and np.array_equal(out, oout), (b.name, lab, r, check, nm, onm)


def test_case_geometry():
    """Sizes, boundaries and validity patterns the case module promises."""
    frame, kf = bc.batches("size")
    assert frame.shared.n <= 8192 and kf.shared.n <= 8192
    nbs = sorted(n.nb for g in frame.nodes for n in g)
    for nb in (1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 255, 256, 257, 511, 512, 513, 2049, 2305):
        assert nb in nbs, nb
    assert {n.na for g in frame.nodes for n in g} >= {1, 63, 64, 65, 130}
    for g in frame.nodes:
        for n in g:
            hot = set(n.hot[0] + n.hot[1])
            L = cz.segment_length(n.nb)
            want = {0, n.nb - 1, 63, 64, 65, 255, 256, 257, L - 1, L, L + 1}
            if L > cz.STAGE:
                want |= {cz.STAGE - 1, cz.STAGE, 7 * L + cz.STAGE - 1, 7 * L + cz.STAGE}
            assert {p for p in want if 0 <= p < n.nb} <= hot or n.nb <= 6, (n.nb, sorted(hot))
            assert not (set(n.hot[0]) & set(n.hot[1]))
    small = frame.nodes[0]
    assert any(n.nb == 6 and int(n.valid_b.sum()) == 4 for n in small)
    assert any(n.nb == 5 and int(n.valid_b.sum()) == 0 for n in small)
    assert cz.segment_length(2049) > cz.STAGE and cz.segment_length(2305) > cz.STAGE
    for b in bc.batches("many"):
        counts = sorted(len(v.node_id) for v in b.others + [b.shared])
        assert counts == [255, 256, 257, 1000, 6000, 8192]
        big = max(b.others + [b.shared], key=lambda v: len(v.node_id))
        assert big.n == 8192
        for v in b.others:  # about half the ids shared with the shared view, not as a prefix
            common = np.isin(v.node_id, b.shared.node_id)
            assert 0.25 < common.mean() < 0.75 or len(b.shared.node_id) == 1000
            assert common[:len(common) // 2].any() and common[len(common) // 2:].any()
            assert not common[:len(common) // 2].all()
        # wide and narrow nodes on both sides, interleaved in node order
        for v in b.others[:3]:
            w = np.diff(v.node_begin) >= 128
            assert w.any() and not w.all() and np.flatnonzero(w).max() - np.flatnonzero(w).min() > 100


def test_ratio_edge_enumeration():
    """Every ratio run has (d1, d2 <= 50) pairs exactly on the float32 boundary; the float32 and the
    double product disagree for 0.6 (d1 = 9, d2 = 15) and for the searched ratio."""
    for r in bc.ALL_RATIOS:
        pairs = cz.ratio_equal_pairs(r)
        assert len(pairs) >= 2 and all(np.float32(d1) == np.float32(r) * np.float32(d2) for d1, d2 in pairs)
    assert (9, 15) in cz.float_double_pairs(0.6)
    assert not cz.float_double_pairs(0.75) and not cz.float_double_pairs(1.0)  # exact products
    fd = cz.float_double_pairs(bc.SEARCHED_RATIO)
    assert fd and min(d2 for _, d2 in fd) <= 50
    for d1, d2 in fd:
        r = np.float32(bc.SEARCHED_RATIO)
        assert (float(d1) < float(r) * d2) and not (np.float32(d1) < r * np.float32(d2))


def size_census():
    """{(overload, size class): Counter} summed over the ratios run, and the table."""
    tot, text = {}, []
    for b in bc.batches("size"):
        full = collections.defaultdict(collections.Counter)
        for lab, A, B in b.pairs():
            for r in b.ratios:
                _, _, c = cz.walk(b.frame, A, B, r, False)
                assert set(k for k, _ in c) == {lab}  # a pair holds nodes of one size class only
                cz.add(full, c)
        text.append(cz.table(full, b.name))
        for cls, c in cz.by_class(full).items():
            tot[(b.frame, cls)] = c
    return tot, "\n".join(text)


def test_census_conditions():
    tot, text = size_census()
    print(text)
    for frame in (True, False):
        for cls in cz.SIZE_CLASSES:
            c = tot[(frame, cls)]
            where = (frame, cls, dict(c))
            assert c["rescan"] >= 5, where
            assert c["stolen"] >= 5, where
            assert c["accepted"] >= 0.1 * c["candidates"], where
            assert c["rej_ratio"] >= 0.1 * c["candidates"], where
            assert c["near_ratio"] >= 10, where
            assert c["d49_50"] >= 1 and c["ties"] >= 1, where
            assert c["accepted"] + c["rej_ratio"] + c["rej_thresh"] == c["candidates"]


def changed_by(letter, frame, cls):
    """The first (ratio, check) at which perturbation `letter` changes the output vector of the
    size-class pair, or None."""
    b = bc.batches("size")[0 if frame else 1]
    lab, A, B = list(b.pairs())[b.labels.index(cls)]
    check = letter == "h"
    for r in (0.9, 1.0, 0.75, bc.SEARCHED_RATIO, 0.6, bc.TIE_RATIO):
        _, ref, _ = cz.walk(frame, A, B, r, check)
        _, out, _ = cz.walk(frame, A, B, r, check, perturb=letter)
        if not np.array_equal(ref, out):
            return r, check
    return None


@pytest.mark.parametrize("letter", sorted(cz.PERTURBATIONS))
def test_perturbation_changes_every_class(letter):
    for cls in cz.SIZE_CLASSES:
        if letter == "e" and cls == "<=64":
            continue  # one segment
        hits = {frame: changed_by(letter, frame, cls) for frame in ((False,) if letter == "f" else (True, False))}
        print(letter, cls, hits)
        assert all(h is not None for h in hits.values()), (letter, cz.PERTURBATIONS[letter], cls, hits)
        # at a ratio a caller would use; only the winner of a tie needs nnratio > 1 to show
        assert letter == "d" or all(h[0] <= 1.0 for h in hits.values()), (letter, cls, hits)
    if letter == "f":  # the Frame overload ignores inner validity by itself
        for cls in cz.SIZE_CLASSES:
            assert changed_by("f", True, cls) is None


def test_exact_cases_decide_on_the_edge():
    """Threshold, tie and ratio-edge nodes: the rule each is built on changes its output."""
    frame, kf = bc.batches("exact")
    for b in (frame, kf):
        pairs = {lab: (A, B) for lab, A, B in b.pairs()}
        A, B = pairs["threshold"]
        assert not np.array_equal(cz.walk(b.frame, A, B, 0.75, False)[1],
                                  cz.walk(b.frame, A, B, 0.75, False, perturb="c")[1])
        A, B = pairs["ties"]
        nm1, _, c = cz.walk(b.frame, A, B, 1.0, False)  # d1 == d2: rejected at nnratio 1.0
        nm, ref, _ = cz.walk(b.frame, A, B, bc.TIE_RATIO, False)
        assert nm1 == 0 and nm == sum(x["ties"] for x in c.values()) == 14
        last = cz.walk(b.frame, A, B, bc.TIE_RATIO, False, perturb="d")[1]
        assert (ref >= 0).sum() == (last >= 0).sum() == 14 and (ref != last).sum() >= 14
        A, B = pairs["ratio-edges"]
        for r in bc.FD_RATIOS:
            assert not np.array_equal(cz.walk(b.frame, A, B, r, False)[1],
                                      cz.walk(b.frame, A, B, r, False, perturb="g")[1])


def test_orientation_cases_straddle_the_ten_percent_rule():
    for b in bc.batches("ori"):
        for (lab, A, B), (keep, plan) in zip(b.pairs(), b.meta):
            total = cz.walk(b.frame, A, B, 0.9, False)[0]
            nm, out, _ = cz.walk(b.frame, A, B, 0.9, True)
            loose = cz.walk(b.frame, A, B, 0.9, True, perturb="h")[0]
            assert total == sum(plan) and all(x >= 1 for x in plan)  # four bins populated
            assert loose == total - plan[3]  # three maxima without the rule: only the fourth bin goes
            assert nm == (loose if keep else loose - plan[2]), (lab, plan, nm)
