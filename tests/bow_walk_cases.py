"""Adversarial ORBmatcher::SearchByBoW inputs, deterministic (fixed seeds), built by hand from
synth.BowFeatures / synth._feature_vector: views on which the reference's running second minimum,
its "already matched" exclusion, its thresholds and its first-minimum ties decide the output.
tests/test_cpu_bow_walk.py shows (with the census and the perturbations of bow_walk_census.py) that
the cases are what they claim; tests/test_gpu_bow_walk.py runs them on the device.

A *batch* is one engine.BowSearch call: a shared view and several others.  In the Frame overload
SearchByBoW(pKF = others[c], F = shared) the shared view is the inner (searched) side, in the
KeyFrame overload SearchByBoW(pKF1 = shared, pKF2 = others[c]) it is the outer side.  Both overloads
of a group use the same node contents, assembled once per side.

Groups
* SIZE: clustered nodes with two contested hot sets each, one node per inner size of interest, the
  hot inner positions on the boundaries the device code has (matched-set words at 64 and 256,
  segment edges, LDS staging edges); one pair per inner size class, all in one batch per overload.
  The largest node of every class also carries isolated features at exact distances (TH_LOW edge,
  a first-minimum tie, float/double ratio pairs) and two matches in minor orientation bins.
* EXACT: nodes built from set bit ranges: d1 in {49, 50, 51}, equal first minima across the
  boundaries, every (d1, d2) on the float32 ratio boundary of each ratio run, float/double pairs.
* MANY: views of 255 / 256 / 257 / 1000 / 6000 nodes against one of 8192 single-feature nodes and
  against the 1000-node view, sharing about half their node ids, with a few wide nodes (wide in
  some views, single in others) in between.
* ORI: clustered views whose matches (nnratio 0.9) fill four orientation bins with the third
  maximum the smallest that ComputeThreeMaxima's 10 % rule keeps, and the largest that it drops.

Ratios.  RATIOS are run everywhere.  First-minimum ties always have d2 = d1, which no ratio <= 1
accepts, so the winner of a tie is visible only with nnratio > 1: TIE_RATIO = 1.25 is run as well.
SEARCHED_RATIO is the first float32 of a seeded uniform(0.5, 1) sequence that has a float/double
pair (float32 and double products of the same operands on different sides of d1) with d2 <= 50;
such pairs exist for many ratios (0.6 among them: d1 = 9, d2 = 15), so condition (g) applies.
"""
import dataclasses

import numpy as np

import bow_walk_census as cz
from rsc import synth

RATIOS = (0.6, 0.75, 0.9, 1.0)
TIE_RATIO = 1.25


def _searched_ratio():
    rng = np.random.default_rng(20260)
    for _ in range(200):
        r = float(np.float32(rng.uniform(0.5, 1.0)))
        if any(d2 <= 50 for _, d2 in cz.float_double_pairs(r, d2max=50)):
            return r
    raise AssertionError("no float/double pair found")


SEARCHED_RATIO = _searched_ratio()
ALL_RATIOS = RATIOS + (SEARCHED_RATIO, TIE_RATIO)
FD_RATIOS = (0.6, SEARCHED_RATIO)  # ratios whose float/double pairs are planted


@dataclasses.dataclass
class Node:
    """One FeatureVector node of both sides, rows in FeatureVector (position) order."""
    id: int
    desc_a: np.ndarray
    desc_b: np.ndarray
    valid_a: np.ndarray
    valid_b: np.ndarray
    angle_a: np.ndarray
    angle_b: np.ndarray

    @property
    def na(self):
        return len(self.desc_a)

    @property
    def nb(self):
        return len(self.desc_b)


@dataclasses.dataclass
class Batch:
    name: str
    frame: bool
    shared: synth.BowFeatures
    others: list
    labels: list      # per other: size class or description
    ratios: tuple
    checks: tuple = (True, False)
    nodes: list = None  # per other: its Node list (groups built from nodes)
    meta: list = None   # per other: what the group's generator planned

    def pairs(self):
        """(label, A = outer, B = inner) per search of the batch."""
        for o, lab in zip(self.others, self.labels):
            yield (lab, o, self.shared) if self.frame else (lab, self.shared, o)


# ---- descriptors --------------------------------------------------------------------------------
def flip(rng, base, counts):
    """len(counts) copies of `base` (uint8[32]) with counts[i] distinct random bits flipped."""
    counts = np.asarray(counts)
    rank = np.argsort(rng.random((len(counts), 256)), axis=1).argsort(axis=1)
    return np.bitwise_xor(base[None, :], np.packbits(rank < counts[:, None], axis=1))


def bit_range(k, start=0):
    """A descriptor with bits start .. start + k - 1 set (tests/test_cpu_orbmatch.py's bits())."""
    d = np.zeros(256, np.uint8)
    d[start:start + k] = 1
    return np.packbits(d, bitorder="little")


def dist(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def boundary_positions(nb):
    """Groups of inner positions on the boundaries of the device code, inside [0, nb)."""
    L = cz.segment_length(nb)
    groups = [(0,), (nb - 1,), (63, 64, 65), (255, 256, 257), (L - 1, L, L + 1)]
    if L > cz.STAGE:  # staging edges inside the first and the last segment
        groups += [(cz.STAGE - 1, cz.STAGE, cz.STAGE + 1),
                   tuple((cz.segments(nb) - 1) * L + cz.STAGE + x for x in (-1, 0, 1))]
    return [tuple(p for p in g if 0 <= p < nb) for g in groups]


def clustered_node(seed, node_id, na, nb, valid_b=None, hot_frac=0.7):
    """Common centre with 6..22 flips on both sides, two hot sub-clusters (sub-centre with 1..4
    flips on 6..12 inner boundary positions, 0..4 flips on ~35 % of the outer features each)."""
    rng = np.random.default_rng(seed)
    centre = rng.integers(0, 256, 32, dtype=np.uint8)
    A = flip(rng, centre, rng.integers(6, 23, na))
    B = flip(rng, centre, rng.integers(6, 23, nb))
    hot = [[], []]
    for k, g in enumerate(boundary_positions(nb)):
        hot[k % 2] += [p for p in g if p not in hot[0] + hot[1]]
    for g in range(2):
        want = max(int(rng.integers(6, 13)), len(hot[g]))
        spare = [p for p in rng.permutation(nb) if p not in hot[0] + hot[1]]
        hot[g] = (hot[g] + [int(p) for p in spare])[:min(want, max(1, (nb + 1 - g) // 2))]
    if nb == 1:
        hot[1] = []
    group = rng.integers(0, 2, na)
    is_hot = rng.random(na) < hot_frac
    for g in range(2):
        sub = flip(rng, centre, [10])[0]
        if hot[g]:
            B[hot[g]] = flip(rng, sub, rng.integers(1, 5, len(hot[g])))
        sel = np.flatnonzero(is_hot & (group == g))
        A[sel] = flip(rng, sub, rng.integers(0, 5, len(sel)))
    va = (rng.random(na) < 0.85).astype(np.uint8)
    if valid_b is None:
        vb = (rng.random(nb) < 0.8).astype(np.uint8)
        vb[hot[0] + hot[1]] = 1
    else:
        vb = np.asarray(valid_b, np.uint8)
    if na == 1:
        va[:] = 1
    n = Node(node_id, A, B, va, vb, np.zeros(na, np.float32), np.zeros(nb, np.float32))
    n.hot = hot
    return n


def plant(node, seed):
    """Overwrite non-hot rows of a clustered node with isolated features: an outer descriptor Z far
    from everything else and inner rows at exact distances from it.  Returns the node."""
    rng = np.random.default_rng(seed)
    taken = set(node.hot[0] + node.hot[1])
    free_b = [int(p) for p in rng.permutation(node.nb) if p not in taken]
    free_a = [int(p) for p in rng.permutation(node.na)]
    # inner distances per outer feature: the TH_LOW edge, a first-minimum tie, float/double pairs
    trios = [(50,), (49,), (51,), (20, 20)]
    trios += [min(cz.float_double_pairs(r), key=lambda p: p[1]) for r in FD_RATIOS]
    planted = []
    for ds in trios:
        while True:
            z = rng.integers(0, 256, 32, dtype=np.uint8)
            far_b = cz.distances(z[None], node.desc_b)[0].min()
            far_a = cz.distances(z[None], node.desc_a)[0].min()
            if far_b > 100 and far_a > 100 and all(dist(z, q) > 100 for q in planted):
                break
        planted.append(z)
        a = free_a.pop()
        node.desc_a[a] = z
        node.valid_a[a] = 1
        pos = sorted(free_b.pop() for _ in ds)
        for k, (p, d) in enumerate(zip(pos, ds)):
            # distinct bit ranges per row: equal distances from z without equal descriptors
            node.desc_b[p] = np.bitwise_xor(z, bit_range(d, 60 * k))
            node.valid_b[p] = 1
    return node


def matched_outer(nodes, frame, nnratio):
    """(node, outer position) of every unfiltered match of the overload over these nodes."""
    A, B = assemble(0, nodes, "a"), assemble(0, nodes, "b")
    _, out, _ = cz.walk(frame, A, B, nnratio, False)
    matched = sorted(int(a) for a in (out[out >= 0] if frame else np.flatnonzero(out >= 0)))
    where = {}
    for k, nid in enumerate(A.node_id):
        node = next(n for n in nodes if n.id == nid)
        for p, f in enumerate(A.feat[A.node_begin[k]:A.node_begin[k + 1]]):
            where[int(f)] = (node, p)
    return [where[a] for a in matched]


def minor_bins(nodes):
    """Angles of a size class: all zero (every match in bin 0) except two Frame-overload matches
    (nnratio 1.0) of the last node, which go to bins 1 and 2: 1 < 0.1f * max1, so the 10 % rule
    removes them."""
    m = matched_outer(nodes, True, 1.0)
    last = [(n, p) for n, p in m if n is nodes[-1]]
    assert len(m) >= 13 and len(last) >= 2, (len(m), len(last))
    for b, (n, p) in enumerate(last[-2:]):
        n.angle_a[p] = 30.0 * (b + 1)


def assemble(seed, nodes, side):
    """One view holding side 'a' or 'b' of the nodes: the nodes' features interleaved at random,
    each node's rows in ascending feature index (so FeatureVector position = row)."""
    rng = np.random.default_rng(seed)
    rows = [n.desc_a if side == "a" else n.desc_b for n in nodes]
    labels = rng.permutation(np.concatenate([np.full(len(r), n.id, np.uint32) for n, r in zip(nodes, rows)]))
    n = len(labels)
    desc, angle, valid = np.zeros((n, 32), np.uint8), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    for nd, r in zip(nodes, rows):
        slots = np.flatnonzero(labels == nd.id)
        desc[slots] = r
        angle[slots] = nd.angle_a if side == "a" else nd.angle_b
        valid[slots] = nd.valid_a if side == "a" else nd.valid_b
    return synth.BowFeatures(n, desc, angle, valid, *synth._feature_vector(labels))


def batches_of(name, groups, ratios, seed, checks=(True, False)):
    """Frame and KeyFrame batches of labelled node groups: the shared view holds every node."""
    every = [n for _, g in groups for n in g]
    labels = [lab for lab, _ in groups]
    out = []
    for frame in (True, False):
        shared = assemble(seed, every, "b" if frame else "a")
        others = [assemble(seed + 1 + k, g, "a" if frame else "b") for k, (_, g) in enumerate(groups)]
        out.append(Batch(f"{name}-{'frame' if frame else 'kf'}", frame, shared, others, labels, ratios, checks,
                         [g for _, g in groups]))
    return out


# ---- group SIZE ---------------------------------------------------------------------------------
# (inner size, outer size); the last node of each class carries the planted features
SIZE_NODES = {
    "<=64": [(1, 1), (2, 63), (3, 1), (4, 64), (5, 65), (63, 64), (64, 130)],
    "65-256": [(65, 64), (128, 63), (129, 65), (255, 64), (256, 130)],
    "257-512": [(257, 65), (511, 64), (512, 130)],
    ">512": [(700, 64), (513, 130)],
    ">2048": [(2049, 130), (2305, 130)],
}


def size_groups():
    groups, nid = [], 11
    for ci, cls in enumerate(cz.SIZE_CLASSES):
        nodes = []
        for k, (nb, na) in enumerate(SIZE_NODES[cls]):
            nodes.append(clustered_node(1000 + 37 * nid, nid, na, nb))
            nid += 1
        if cls == "<=64":
            # exactly 4 valid of 6 inner features (a full record of a complete list) and an inner
            # node without any valid feature
            nodes.insert(0, clustered_node(1000 + 37 * nid, nid, 63, 6, valid_b=[1, 0, 1, 1, 0, 1]))
            nodes.insert(0, clustered_node(1000 + 37 * (nid + 1), nid + 1, 64, 5, valid_b=[0] * 5))
            nid += 2
        plant(nodes[-1], 7000 + ci)
        minor_bins(nodes)
        groups.append((cls, nodes))
    return groups


# ---- group EXACT --------------------------------------------------------------------------------
def exact_node(node_id, outer_rows, inner_rows):
    a, b = np.array(outer_rows, np.uint8), np.array(inner_rows, np.uint8)
    return Node(node_id, a, b, np.ones(len(a), np.uint8), np.ones(len(b), np.uint8),
                np.zeros(len(a), np.float32), np.zeros(len(b), np.float32))


def tie_node(node_id, nb, pairs, d, seed):
    """One outer feature per (p, q) of `pairs`: a random descriptor whose inner positions p < q are
    both at distance d from it (different bits); every other inner row random, ~128 away."""
    rng = np.random.default_rng(seed)
    B = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    Z = rng.integers(0, 256, (len(pairs), 32), dtype=np.uint8)
    for z, (p, q) in zip(Z, pairs):
        B[p], B[q] = np.bitwise_xor(z, bit_range(d, 0)), np.bitwise_xor(z, bit_range(d, 100))
    D = cz.distances(Z, B)
    for k, (p, q) in enumerate(pairs):
        assert D[k, p] == D[k, q] == d and np.sort(D[k])[2] > 80
    return exact_node(node_id, Z, B)


def exact_groups():
    nid = 11
    thr = []
    for d1 in (49, 50, 51):
        thr.append(exact_node(nid, [bit_range(0)], [bit_range(d1)]))
        thr.append(exact_node(nid + 1, [bit_range(0)], [bit_range(d1), bit_range(100, 100)]))
        thr.append(exact_node(nid + 2, [bit_range(0)], [bit_range(100, 100), bit_range(d1)]))
        nid += 3
    ties = []
    for nb in (65, 300, 513):
        L = cz.segment_length(nb)
        for p, q in ((63, 64), (L - 1, L), (0, nb - 1)):
            ties.append(tie_node(nid, nb, [(p, q)], 20, 9000 + nid))
            nid += 1
    L = cz.segment_length(2305)  # one wide node with a tie on each of its boundaries
    ties.append(tie_node(nid, 2305, [(63, 64), (L - 1, L), (0, 2304), (cz.STAGE - 1, cz.STAGE),
                                     (7 * L + cz.STAGE - 1, 7 * L + cz.STAGE)], 20, 9000 + nid))
    nid += 1
    edges = []
    for r in ALL_RATIOS:
        pairs = set()
        for d1, d2 in cz.ratio_equal_pairs(r) + cz.float_double_pairs(r):
            pairs |= {(d, d2) for d in (d1 - 1, d1, d1 + 1) if 0 <= d <= min(d2, 51)}
        for d1, d2 in sorted(pairs):
            edges.append(exact_node(nid, [bit_range(0)], [bit_range(d1), bit_range(d2)]))
            edges.append(exact_node(nid + 1, [bit_range(0)], [bit_range(d2), bit_range(d1)]))
            nid += 2
    return [("threshold", thr), ("ties", ties), ("ratio-edges", edges)]


# ---- group MANY ---------------------------------------------------------------------------------
WIDE_IDS = (6, 1001, 4094, 4097, 8190, 8192, 8193, 12000, 12001, 15000, 16001, 16382)


def many_view(seed, ids, base, wide_prob=0.6, wide_size=130):
    """One feature per node id (the node's base row with 0..60 flips); every id of WIDE_IDS in
    `ids` becomes, with probability wide_prob, a node of wide_size features clustered on its base
    row."""
    rng = np.random.default_rng(seed)
    rows, labels = [], []
    for i in ids:
        k = wide_size if (i in WIDE_IDS and rng.random() < wide_prob) else 1
        flips = rng.integers(4, 20, k) if k > 1 else rng.integers(0, 61, 1)
        rows.append(flip(rng, base[i], flips))
        labels.append(np.full(k, i, np.uint32))
    labels = np.concatenate(labels)
    perm = rng.permutation(len(labels))
    desc, labels = np.concatenate(rows)[perm], labels[perm]
    n = len(labels)
    return synth.BowFeatures(n, desc, rng.uniform(0, 360, n).astype(np.float32),
                             (rng.random(n) < 0.9).astype(np.uint8), *synth._feature_vector(labels))


def many_batches():
    """Node counts around the 256 threads of the join kernel and far beyond.  `big` has 8192
    single-feature nodes on the even ids; the others draw their ids from all of 0..16383, so about
    half are shared, interleaved; the WIDE_IDS are in every other view, wide in some, single in
    others, so wide and narrow nodes and scans alternate in node order."""
    rng = np.random.default_rng(4242)
    base = rng.integers(0, 256, (16384, 32), dtype=np.uint8)
    big = many_view(1, range(0, 16384, 2), base, wide_prob=0.0)
    assert big.n == 8192 and len(big.node_id) == 8192
    others, labels = [], []
    for k, n_nodes in enumerate((255, 256, 257, 1000, 6000)):
        ids = rng.choice(np.setdiff1d(np.arange(16384), WIDE_IDS), n_nodes - len(WIDE_IDS), replace=False)
        ids = np.sort(np.concatenate([ids, WIDE_IDS]))
        others.append(many_view(10 + k, [int(i) for i in ids], base))
        assert len(others[-1].node_id) == n_nodes
        labels.append(f"{n_nodes} nodes")
    mid = others[3]  # 1000 nodes: the shared view of the second pair of batches
    rest = others[:3] + others[4:] + [big]
    rest_labels = labels[:3] + labels[4:] + ["8192 nodes"]
    return [Batch("many-frame", True, big, others, labels, RATIOS),
            Batch("many-kf", False, big, others, labels, RATIOS),
            Batch("many1000-frame", True, mid, rest, rest_labels, RATIOS),
            Batch("many1000-kf", False, mid, rest, rest_labels, RATIOS)]


# ---- group ORI ----------------------------------------------------------------------------------
def histogram_plan(total, keep):
    """Bin counts (m1, m2, m3, m4) summing to `total` with m3 the smallest third maximum that
    ComputeThreeMaxima keeps (not m3 < 0.1f * m1), or the largest one it drops."""
    def counts(m3):
        m2, m4 = m3 + 2, min(2, m3)
        return total - m2 - m3 - m4, m2, m3, m4
    m3 = 1
    while np.float32(m3) < np.float32(0.1) * np.float32(counts(m3)[0]):
        m3 += 1
    c = counts(m3 if keep else m3 - 1)
    assert c[0] > c[1] > c[2] >= c[3] >= 1, c
    return c


def set_histogram(nodes, frame, keep):
    """Outer angles such that the matches of the overload at nnratio 0.9 fall in bins 0..3 with
    the counts of histogram_plan (inner angles are 0)."""
    m = matched_outer(nodes, frame, 0.9)
    plan = histogram_plan(len(m), keep)
    for (node, p), b in zip(m, np.repeat(np.arange(4), plan)):
        node.angle_a[p] = 30.0 * b
    return plan


def ori_batches():
    """Per overload two clustered pairs whose matches at nnratio 0.9 fill four orientation bins,
    the third maximum on either side of the 10 % rule (meta: (kept, bin counts) per pair)."""
    out = []
    for frame in (True, False):
        groups, meta = [], []
        for k, keep in enumerate((True, False)):
            nodes = [clustered_node(5000 + 11 * k + j, 11 + 10 * k + j, 130, nb)
                     for j, nb in enumerate((96, 200, 520))]
            plan = set_histogram(nodes, frame, keep)
            groups.append((f"third maximum {'kept' if keep else 'dropped'}", nodes))
            meta.append((keep, plan))
        out.append(batches_of("ori", groups, (0.9,), 300)[0 if frame else 1])
        out[-1].meta = meta
    return out


_cache = {}


def batches(group):
    """The batches of a group ('size', 'exact', 'many', 'ori'), built once per process."""
    if group not in _cache:
        if group == "size":
            _cache[group] = batches_of("size", size_groups(), ALL_RATIOS, 100)
        elif group == "exact":
            _cache[group] = batches_of("exact", exact_groups(), ALL_RATIOS, 200)
        elif group == "many":
            _cache[group] = many_batches()
        else:
            _cache[group] = ori_batches()
    return _cache[group]
