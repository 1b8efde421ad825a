"""Shared inputs of the vocabulary-transform tests (tests/test_cpu_bowvoc.py, tests/test_gpu_bowvoc.py,
tests/golden/make_bowvoc_golden.py): small seeded vocabularies and descriptor sets, one per mechanism."""
import copy

import numpy as np

from rsc import synth


def tiny_vocabulary():
    """k = 2, L = 2, hand-built: nodes 1, 2 under the root, words 3, 4 under node 1 and 5, 6 under
    node 2 (word ids 0..3).  Descriptors are bytes of all-0 / all-1 patterns, so distances are easy:
    node 1 = 0x00.., node 2 = 0xFF..; word 3 = 0x00.., word 4 = first 8 bytes 0xFF; word 5 = 0xFF..,
    word 6 = last 8 bytes 0x00."""
    desc = np.zeros((7, 32), np.uint8)
    desc[2] = 0xFF
    desc[4, :8] = 0xFF
    desc[5] = 0xFF
    desc[6, :24] = 0xFF
    weight = np.array([0, 0, 0, 0.1, 0.7, 1.5, 0.0])  # word 6 (id 3) is stopped
    return synth.Vocabulary(2, 2, 0, 0, np.array([0, 0, 0, 1, 1, 2, 2], np.int32),
                            np.array([0, 0, 0, 1, 1, 1, 1], np.uint8), desc, weight)


def bits(*ranges):
    """A descriptor with the given byte ranges set to 0xFF."""
    d = np.zeros(32, np.uint8)
    for a, b in ranges:
        d[a:b] = 0xFF
    return d


def golden_case():
    """The committed fixture's inputs: a 40-node vocabulary (k = 3, L = 3) with stopped words and
    duplicated siblings, 64 descriptors."""
    rng = np.random.default_rng(7001)
    voc = synth.make_vocabulary(rng, 3, 3, zero_weight_frac=0.15, duplicate_frac=0.2)
    desc = synth.sample_descriptors(rng, voc, 64, mean_flips=10.0, random_frac=0.2)
    return voc, desc


def irregular_vocabulary():
    """Nodes with 1, 2, 16, 17 and 32 children, leaves at depths 2-5 (L = 5)."""
    rng = np.random.default_rng(7002)
    return synth.make_vocabulary(rng, 10, 5, child_counts=(17, 1, 2, 16, 32), leaf_prob=0.9, min_leaf_depth=2,
                                 zero_weight_frac=0.05)


def depths(voc):
    d = np.zeros(voc.n_nodes, np.int32)
    for i in range(1, voc.n_nodes):
        d[i] = d[voc.parent[i]] + 1
    return d


def with_loader_quirk(voc):
    """The reference loader's trailing-newline node: one more child of the root, not a word, weight
    0, here with a chosen descriptor (the reference's is uninitialised memory)."""
    v = copy.deepcopy(voc)
    rng = np.random.default_rng(7003)
    extra = rng.integers(0, 256, size=(1, 32), dtype=np.uint8)
    v.parent = np.concatenate([v.parent, np.zeros(1, np.int32)])
    v.is_leaf = np.concatenate([v.is_leaf, np.zeros(1, np.uint8)])
    v.desc = np.concatenate([v.desc, extra])
    v.weight = np.concatenate([v.weight, np.zeros(1)])
    return v, extra[0]


def write_text_vocabulary(voc, path, trailing_newline=True):
    """The ORBvoc.txt format: `k L scoring weighting`, then `parent isLeaf b0 .. b31 weight` per node
    (the root has no line).  Weights are written with repr(), which round-trips a double."""
    lines = [f"{voc.k} {voc.L} {voc.scoring} {voc.weighting}"]
    for i in range(1, voc.n_nodes):
        lines.append(f"{int(voc.parent[i])} {int(voc.is_leaf[i])} " + " ".join(str(int(b)) for b in voc.desc[i]) +
                     f" {float(voc.weight[i])!r}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + ("\n" if trailing_newline else ""))
