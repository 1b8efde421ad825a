"""The vocabulary transform's semantics without a GPU: hand-built known answers on a k = 2, L = 2 tree
for the sequential restatement (tests/bowvoc_ref.py) and the C++ sequential loop (tests/bowvoc_emu), the
committed golden fixture, the synthetic vocabulary generator, and the facade's text loader."""
import math
import os
import subprocess

import numpy as np
import pytest

import bowvoc_cases as bc
from bowvoc_emu_lib import DIR as EMU_DIR, EmuVocabulary, lib as emu_lib
from bowvoc_ref import RefVocabulary, UninitialisedNodeId, assert_same
from rsc import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPLS = [RefVocabulary, EmuVocabulary]


@pytest.fixture(params=IMPLS, ids=["restatement", "emu"])
def tiny(request):
    return request.param(bc.tiny_vocabulary())


def test_word_numbering():
    r = RefVocabulary(bc.tiny_vocabulary())
    assert r.size() == 4 and r.word_id[3:] == [0, 1, 2, 3]
    # a childless node that is not a word keeps word id 0 and its weight
    v = bc.tiny_vocabulary()
    v.is_leaf[4] = 0
    r = RefVocabulary(v)
    assert r.size() == 3 and r.word_id[3:] == [0, 0, 1, 2]
    t = r.transform(np.stack([bc.bits(), bc.bits((0, 8))]), 1, normalize=False)
    assert t["word_id"].tolist() == [0] and t["word_value"][0] == 0.1 + 0.7 and t["feat"].tolist() == [0, 1]


def test_descent_and_ties(tiny):
    d = np.stack([bc.bits(),            # node 1, word 3 exactly
                  bc.bits((0, 32)),     # node 2, word 5 exactly
                  bc.bits((0, 16)),     # 128 from both children of the root: node 1; then word 4 (64 < 128)
                  bc.bits((0, 4)),      # node 1; 32 from word 3 and from word 4: word 3
                  bc.bits((0, 8))])     # node 1, word 4 exactly
    t = tiny.transform(d, 1)
    assert t["node_id"].tolist() == [1, 2] and t["node_begin"].tolist() == [0, 4, 5]
    assert t["feat"].tolist() == [0, 2, 3, 4, 1]
    assert t["word_id"].tolist() == [0, 1, 2]
    s = (0.1 + 0.1) + (0.7 + 0.7) + 1.5
    assert t["word_value"].tolist() == [(0.1 + 0.1) / s, (0.7 + 0.7) / s, 1.5 / s]


def test_stopped_word_is_in_neither_vector(tiny):
    d = np.stack([bc.bits((0, 24)), bc.bits(), bc.bits((0, 24))])  # word 6 (weight 0), word 3, word 6
    t = tiny.transform(d, 1)
    assert t["word_id"].tolist() == [0] and t["word_value"].tolist() == [1.0]
    assert t["node_id"].tolist() == [1] and t["feat"].tolist() == [1]
    t = tiny.transform(d[::2], 1)  # every feature stopped: empty vectors, no division
    assert len(t["word_id"]) == 0 and len(t["node_id"]) == 0 and t["node_begin"].tolist() == [0]


@pytest.mark.parametrize("levelsup,nodes", [(0, [3, 5]), (1, [1, 2]), (2, [0]), (3, [0]), (7, [0])])
def test_levelsup(tiny, levelsup, nodes):
    t = tiny.transform(np.stack([bc.bits(), bc.bits((0, 32))]), levelsup)
    assert t["node_id"].tolist() == nodes
    assert sorted(t["feat"].tolist()) == [0, 1]


def test_uninitialised_node_id_is_refused():
    v = bc.tiny_vocabulary()
    v.L = 3  # nid_level = 3 - 0 lies below every leaf (depth 2)
    with pytest.raises(UninitialisedNodeId):
        RefVocabulary(v).transform(bc.bits()[None], 0)
    with pytest.raises(ValueError):
        EmuVocabulary(v).transform(bc.bits()[None], 0)


def test_six_identical_descriptors_sum_sequentially():
    """The value of a word hit c times is w; += w; ... (BowVector::addWeight), not c * w: for
    w = 0.1 the two differ from 6 features on."""
    r = RefVocabulary(bc.tiny_vocabulary())
    t = r.transform(np.repeat(bc.bits()[None], 6, 0), 1, normalize=False)
    s = 0.1
    for _ in range(5):
        s += 0.1
    assert t["word_id"].tolist() == [0] and t["word_value"][0] == s
    assert t["word_value"][0] != 6 * 0.1
    for w in (0.1, math.log(10 / 3), math.log(1000 / 7), math.log(10)):
        s, first = 0.0, None
        for c in range(1, 20):
            s += w
            if s != c * w and first is None:
                first = c
        assert first == 6, (w, first)


def test_normalisation_is_one_ordered_sum():
    voc, desc = bc.golden_case()
    t = RefVocabulary(voc).transform(desc, 1, normalize=False)
    n = RefVocabulary(voc).transform(desc, 1)
    norm = 0.0
    for x in t["word_value"]:
        norm += abs(float(x))
    assert norm == n["norm"] and [float(x) / norm for x in t["word_value"]] == n["word_value"].tolist()


def test_golden_fixture_reproduces():
    z = np.load(os.path.join(ROOT, "tests", "golden", "bowvoc_traces.npz"))
    voc, desc = bc.golden_case()
    for k, a in (("parent", voc.parent), ("is_leaf", voc.is_leaf), ("vdesc", voc.desc), ("desc", desc)):
        assert np.array_equal(z[k], a), k
    assert np.array_equal(z["weight"].view(np.uint64), voc.weight.view(np.uint64))
    assert len(voc.parent) == 40 and len(desc) == 64
    for impl in IMPLS:
        v = impl(voc)
        for lu in z["levelsups"]:
            want = {k: z[f"l{lu}_{k}"] for k in ("word_id", "word_value", "node_id", "node_begin", "feat")}
            assert_same(v.transform(desc, int(lu)), want, (impl.__name__, int(lu)))
    # the fixture has stopped features, several features per word and shared nodes
    assert z["l1_f_stopped"].sum() > 0 and len(z["l1_word_id"]) < 64 - z["l1_f_stopped"].sum()


@pytest.mark.parametrize("case", ["irregular", "deep", "quirk", "duplicates"])
def test_emulation_agrees_with_the_restatement(case):
    rng = np.random.default_rng(31)
    if case == "irregular":
        voc, lu = bc.irregular_vocabulary(), 3
    elif case == "deep":
        voc, lu = synth.make_vocabulary(rng, 4, 6, zero_weight_frac=0.05, nonword_leaf_frac=0.05), 4
    elif case == "quirk":
        voc, lu = bc.with_loader_quirk(synth.make_vocabulary(rng, 3, 2))[0], 1
    else:
        voc, lu = synth.make_vocabulary(rng, 4, 3, duplicate_frac=0.5), 1
    desc = synth.sample_descriptors(rng, voc, 300, mean_flips=8.0)
    if case == "quirk":
        desc[::4] = voc.desc[-1]
    if case == "duplicates":
        desc[:64] = voc.desc[-64:]
    ref = RefVocabulary(voc).transform(desc, lu)
    assert_same(EmuVocabulary(voc).transform(desc, lu), ref, case)
    if case == "quirk":
        assert ref["f_stopped"][::4].all() and not np.isin(np.arange(0, 300, 4), ref["feat"]).any()


def test_make_vocabulary_shapes():
    rng = np.random.default_rng(32)
    v = synth.make_vocabulary(rng, 10, 3)
    assert v.n_nodes == 1111 and (v.parent[1:] < np.arange(1, 1111)).all() and (np.diff(v.parent) >= 0).all()
    assert RefVocabulary(v).size() == 1000
    # a child is its parent with bit flips: closer to its parent than a random descriptor is
    x = np.unpackbits(v.desc[1:] ^ v.desc[v.parent[1:]], axis=1).sum(1)
    assert 10 < x.mean() < 60
    v = bc.irregular_vocabulary()
    nch = np.bincount(v.parent[1:], minlength=v.n_nodes)
    assert {1, 2, 16, 17, 32} <= set(nch.tolist()) and nch.max() == 32
    assert set(bc.depths(v)[nch == 0].tolist()) == {2, 3, 4, 5}
    v = synth.make_vocabulary(rng, 4, 3, zero_weight_frac=0.3, duplicate_frac=0.5)
    leaves = np.bincount(v.parent[1:], minlength=v.n_nodes) == 0
    assert 0 < (v.weight[leaves] == 0).sum() < leaves.sum()
    assert ((v.desc[2:] == v.desc[1:-1]).all(1) & (v.parent[2:] == v.parent[1:-1])).sum() > 5


def test_emulation_program_under_sanitizers():
    emu_lib()
    for exe in ("bowvoc_emu_main", "bowvoc_emu_main_san"):
        out = subprocess.run([os.path.join(EMU_DIR, "build", exe)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        assert out.stdout.count("levelsup") == 5


@pytest.mark.parametrize("trailing_newline", [True, False])
def test_facade_loader_parses_the_text_format(tmp_path, trailing_newline):
    """csrc/facade/ORBVocabulary.hpp parseTextFile on a file written here: every node as written, and
    no extra node for the trailing newline (the reference loader's quirk is not reproduced)."""
    exe = os.path.join(ROOT, "orb-slam2-optimized_amd", "lib", "facade_voc_test")
    assert os.path.exists(exe), "facade_voc_test not built (make)"
    voc, _ = bc.golden_case()
    path = tmp_path / "voc.txt"
    bc.write_text_vocabulary(voc, path, trailing_newline)
    if trailing_newline:
        assert open(path).read().endswith("\n")
    out = subprocess.run([exe, "parse", str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[0] == f"{voc.k} {voc.L} 0 0 {voc.n_nodes}"
    assert len(lines) == voc.n_nodes
    for i in range(1, voc.n_nodes):
        f = lines[i].split()
        assert int(f[0]) == voc.parent[i] and int(f[1]) == voc.is_leaf[i], i
        assert [int(x) for x in f[2:34]] == voc.desc[i].tolist(), i
        assert int(f[34], 16) == int(voc.weight[i:i + 1].view(np.uint64)[0]), i


def test_facade_loader_rejects_malformed_files(tmp_path):
    exe = os.path.join(ROOT, "orb-slam2-optimized_amd", "lib", "facade_voc_test")
    for k, text in enumerate(["", "3 3 0\n", "3 3 0 0\n5 1 " + "0 " * 32 + "1.0\n", "3 3 0 0\n0 1 1 2 3 1.0\n"]):
        p = tmp_path / f"bad{k}.txt"
        p.write_text(text)
        out = subprocess.run([exe, "parse", str(p)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2, (k, out.stdout)
