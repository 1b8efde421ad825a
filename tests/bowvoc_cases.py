"""Shared inputs of the vocabulary-transform tests (tests/test_cpu_bowvoc.py, tests/test_gpu_bowvoc.py,
tests/golden/make_bowvoc_golden.py): small seeded vocabularies and descriptor sets, one per mechanism."""
import copy

import numpy as np

import ref_dbow2_io
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


def with_loader_quirk(voc, observed=False):
    """The reference loader's trailing-newline node, whose parent and nIsLeaf are
    uninitialised reads.  observed=False: the shape C++11's "0 on failure" would give if the
    extraction were attempted: one more child of the root, not a word, weight 0, here with a chosen
    descriptor.  observed=True: what the built reference does (tests/golden/ref_dbow2.npz): the
    previous line's values are reused, so it is one more child of the LAST LINE'S PARENT and a WORD
    of weight 0; its descriptor is never written (32 zero bytes under the stand-in Mat::create)."""
    v = copy.deepcopy(voc)
    if observed:
        extra = np.zeros((1, 32), np.uint8)
        parent, leaf = v.parent[-1:], v.is_leaf[-1:]
    else:
        extra = np.random.default_rng(7003).integers(0, 256, size=(1, 32), dtype=np.uint8)
        parent, leaf = np.zeros(1, np.int32), np.zeros(1, np.uint8)
    v.parent = np.concatenate([v.parent, parent.astype(np.int32)])
    v.is_leaf = np.concatenate([v.is_leaf, leaf.astype(np.uint8)])
    v.desc = np.concatenate([v.desc, extra])
    v.weight = np.concatenate([v.weight, np.zeros(1)])
    return v, extra[0]


def q21_vocabulary():
    """k = 3, L = 2 with a sparse node 3 (8 bits set) whose children are >= 24 bits away from it: a
    feature equal to node 3's descriptor is nearer to 32 zero bytes than to any child of node 3."""
    voc = synth.make_vocabulary(np.random.default_rng(15), 3, 2)
    assert voc.n_nodes == 13 and voc.parent[-1] == 3
    rng = np.random.default_rng(7021)
    voc.desc[3] = 0
    voc.desc[3, :8] = 1
    for c in (10, 11, 12):
        assert voc.parent[c] == 3
        m = np.zeros(256, np.uint8)
        m[rng.choice(256, size=24 + 4 * (c - 10), replace=False)] = 1
        voc.desc[c] = voc.desc[3] ^ np.packbits(m)
    return voc


def q21_descriptors(voc):
    """90 descriptors for q21_vocabulary(); every third one is node 3's descriptor, half of those one
    bit away -> (descriptors, indices of those features)."""
    desc = synth.sample_descriptors(np.random.default_rng(150), voc, 90, mean_flips=5.0, random_frac=0.0)
    hit = np.arange(0, 90, 3)
    desc[hit] = voc.desc[3]
    desc[hit[::2], 31] ^= 0x80
    return desc, hit


def fixture_vocabulary(z, name):
    """Vocabulary `name` of tests/golden/ref_dbow2.npz as the built reference holds it after loading
    its text file: the nodes of the file, and for a file with a trailing newline the extra word in the
    shape the reference gave it (recorded in the fixture: its node id, parent and weight)."""
    voc = synth.Vocabulary(int(z[f"voc.{name}.k"]), int(z[f"voc.{name}.L"]), 0, 0, z[f"voc.{name}.parent"].copy(),
                           z[f"voc.{name}.is_leaf"].copy(), z[f"voc.{name}.desc"].copy(), z[f"voc.{name}.weight"].copy())
    if bool(z[f"voc.{name}.newline"]):
        last = z[f"voc.{name}.chain"][-1]
        quirk, _ = with_loader_quirk(voc, observed=True)
        assert last[0] == voc.n_nodes and last[1] == quirk.parent[-1] and z[f"voc.{name}.wweight_tail"].tolist() == [0.0]
        return quirk
    return voc


def write_text_vocabulary(voc, path, trailing_newline=True):
    """The ORBvoc.txt format, through its one writer (tests/ref_dbow2_io.py)."""
    ref_dbow2_io.write_vocabulary(path, voc.k, voc.L, voc.parent, voc.is_leaf, voc.desc, voc.weight, trailing_newline)
