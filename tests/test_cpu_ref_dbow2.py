"""This project's restatements against the BUILT REFERENCE DBoW2, bit for bit, through the committed
fixture tests/golden/ref_dbow2.npz (tests/golden/make_ref_dbow2_golden.py records what
oracle/_ref/ref_dbow2, the reference's own sources around oracle/ref_dbow2_driver.cpp, returns):

* the vocabulary transform of tests/bowvoc_ref.py and tests/bowvoc_emu, and their word numbering;
* the facade loader's node and word numbering (csrc/facade/ORBVocabulary.hpp, facade_voc_test parse);
* the L1 score of oracle/kfdb_oracle and of the pure-Python PyKFDB, alone and through the database;
* BowVector::normalize as tests/bowvoc_ref.py restates it;
* RandomInt of the oracle and of the host RngStream, and the kernels' host-compiled samplers;
* live: the reference binary, where it is built, still returns what the fixture holds.

No tolerance anywhere: integers equal, doubles equal as uint64, floats as uint32."""
import json
import os
import subprocess

import numpy as np
import pytest

import bowvoc_cases as bc
import hostemu_lib as he
import oracle_lib as ol
import ref_dbow2_io as rio
from bowvoc_emu_lib import EmuVocabulary
from bowvoc_ref import RefVocabulary, assert_same, normalize_l1
from rsc import synth
from test_cpu_kfdb import PyKFDB
from test_gpu_ref_dbow2 import sample_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(rio.FIXTURE)
VOCS, CASES = rio.names(Z, "vocs"), rio.names(Z, "tcases")
PAIRS = list(zip(rio.names(Z, "spair_a"), rio.names(Z, "spair_b"), rio.names(Z, "spair_kind")))


def f64_bits(x):
    return int(np.float64(x).view(np.uint64))


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def parent_chains(parent, nodes, nl):
    """getParentNode(w, l) for l = 0..nl-1 of the words at `nodes` (TemplatedVocabulary.h:1264-1274)."""
    chain = np.zeros((len(nodes), nl), np.uint32)
    cur = np.asarray(nodes, np.int64)
    for l in range(nl):
        chain[:, l] = cur
        cur = parent[cur]  # the root's parent is the root
    return chain


@pytest.mark.parametrize("v", VOCS)
def test_word_numbering_equals_the_reference(v):
    voc = bc.fixture_vocabulary(Z, v)
    r = RefVocabulary(voc)
    chain = Z[f"voc.{v}.chain"]
    assert r.size() == int(Z[f"voc.{v}.size"]) == len(chain)
    assert [r.word_id[n] for n in chain[:, 0]] == list(range(r.size()))
    assert np.array_equal(parent_chains(voc.parent, chain[:, 0], chain.shape[1]), chain)
    assert np.array_equal(np.array([r.weight[n] for n in chain[:, 0]]).view(np.uint64),
                          rio.fixture_word_weights(Z, v).view(np.uint64))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("impl", [RefVocabulary, EmuVocabulary], ids=["restatement", "emu"])
def test_transform_equals_the_reference(impl, case):
    voc = impl(bc.fixture_vocabulary(Z, str(Z[f"t.{case}.voc"])))
    for lu in Z[f"t.{case}.levelsups"]:
        want = {k: Z[f"t.{case}.l{int(lu)}.{k}"] for k in rio.TRANSFORM_KEYS}
        assert_same(voc.transform(Z[f"t.{case}.desc"], int(lu)), want, (case, int(lu)))


@pytest.mark.parametrize("v", VOCS)
def test_facade_loader_numbering_equals_the_reference(tmp_path, v):
    """parseTextFile on the very text the reference loaded: words numbered in the reference's order with
    its node ids, parent chains and weights.  The facade skips the empty last line (Q21), so for a
    file with a trailing newline its size() is one less than the reference's: the zero-weight word."""
    exe = os.path.join(ROOT, "orb-slam2-optimized_amd", "lib", "facade_voc_test")
    assert os.path.exists(exe), "facade_voc_test not built (make)"
    path = tmp_path / "voc.txt"
    path.write_text(rio.fixture_vocabulary_text(Z, v))
    out = subprocess.run([exe, "parse", str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    rows = [l.split() for l in lines[1:]]
    parent = np.array([0] + [int(f[0]) for f in rows], np.int64)
    weight = np.array([0] + [int(f[34], 16) for f in rows], np.uint64)
    nodes = np.array([i + 1 for i, f in enumerate(rows) if int(f[1]) > 0], np.int64)
    chain, extra = Z[f"voc.{v}.chain"], int(bool(Z[f"voc.{v}.newline"]))
    assert len(nodes) == int(Z[f"voc.{v}.size"]) - extra and len(parent) == len(Z[f"voc.{v}.parent"])
    n = len(nodes)
    assert np.array_equal(parent_chains(parent, nodes, chain.shape[1]), chain[:n])
    assert np.array_equal(weight[nodes], rio.fixture_word_weights(Z, v)[:n].view(np.uint64))
    if extra:
        assert chain[n, 0] == len(parent) and Z[f"voc.{v}.wweight_tail"].view(np.uint64).tolist() == [0]


def test_trailing_newline_shape_as_recorded():
    """what the built reference made of the empty last line."""
    plain, nl = Z["voc.q21_plain.chain"], Z["voc.q21_newline.chain"]
    n_nodes = len(Z["voc.q21_plain.parent"])
    assert int(Z["voc.q21_newline.size"]) == int(Z["voc.q21_plain.size"]) + 1 == 10
    assert np.array_equal(nl[:-1], plain)
    assert nl[-1].tolist() == [n_nodes, int(Z["voc.q21_plain.parent"][-1]), 0, 0]  # a word under the last line's parent
    assert Z["voc.q21_newline.wweight_tail"].view(np.uint64).tolist() == [0]
    hit = Z["q21.hit"]
    assert np.isin(hit, Z["t.q21_plain.l1.feat"]).all() and not np.isin(hit, Z["t.q21_newline.l1.feat"]).any()


@pytest.mark.parametrize("a,b,kind", PAIRS, ids=[f"{a}-{b}" for a, b, _ in PAIRS])
def test_l1_score_equals_the_reference(a, b, kind):
    i = PAIRS.index((a, b, kind))
    (ia, va), (ib, vb) = rio.fixture_vector(Z, a), rio.fixture_vector(Z, b)
    want64, want32 = int(Z["spair_bits64"][i]), int(Z["spair_bits32"][i])
    s = ol.l1_score(ia, va, ib, vb)
    assert f64_bits(s) == want64 and f32_bits(np.float32(s)) == want32
    p = PyKFDB.score(dict(zip(ia.tolist(), va.tolist())), dict(zip(ib.tolist(), vb.tolist())))
    assert f64_bits(p) == want64
    common = len(np.intersect1d(ia, ib))
    if kind == "none":
        assert common == 0 and want64 == 0x8000000000000000 and want32 == 0x80000000  # -0.0, the sign recorded
    for cls in (PyKFDB, ol.OracleKFDB):  # through the database, as the device test reads it
        db = cls(1)
        db.add(0, ib, vb)
        cand = db.detect_relocalization(5, ia, va)
        (_, rq), (_, rw), (_, rs) = db.state(0)
        if common:
            assert rq == 5 and rw == common and list(cand) == [0] and f32_bits(rs) == want32, cls.__name__
        else:
            assert rq == 0 and len(cand) == 0, cls.__name__


@pytest.mark.parametrize("n", rio.names(Z, "vecs"))
def test_normalize_equals_the_reference(n):
    norm, vals = normalize_l1(Z[f"vec.{n}.raw"].tolist())
    assert np.array_equal(np.array(vals, np.float64).view(np.uint64), Z[f"vec.{n}.val"].view(np.uint64))
    if n in ("zeros", "empty"):
        assert norm == 0.0


def test_chain_equals_the_reference():
    name, lu = str(Z["chain.voc"]), int(Z["chain.levelsup"])
    for impl in (RefVocabulary, EmuVocabulary):
        voc = impl(bc.fixture_vocabulary(Z, name))
        q, kf = voc.transform(Z["chain.q_desc"], lu), voc.transform(Z["chain.kf_desc"], lu)
        s = ol.l1_score(q["word_id"], q["word_value"], kf["word_id"], kf["word_value"])
        assert f64_bits(s) == int(Z["chain.bits64"]) and f32_bits(np.float32(s)) == int(Z["chain.bits32"])


def random_int_of(raw, maxes):
    """RandomInt(0, max) of a raw rand() value (Random.cpp:47-50): rand() / 2^31 is exact in double and
    so is its product with d <= 2^11, so the truncation is an integer shift."""
    return ((raw.astype(np.int64) * (np.asarray(maxes, np.int64) + 1)) >> 31).astype(np.int32)


@pytest.mark.parametrize("i", range(len(Z["rand_cases"])))
def test_random_int_equals_the_reference(i):
    seed, N, minset, count = (int(x) for x in Z["rand_cases"][i])
    want = Z[f"rand.{i}"]
    maxes = (N - 1 - np.arange(count) % minset).astype(np.int32)
    assert np.array_equal(ol.random_int(seed, maxes), want)  # the oracle's RandomInt
    assert np.array_equal(random_int_of(he.rand_stream(seed, count), maxes), want)  # the host RngStream
    with open(os.path.join(ROOT, "tests", "golden", "glibc_rand.json")) as f:
        raw = json.load(f)["rand"]
    if str(seed) in raw:  # the committed raw glibc stream of the same seed
        assert np.array_equal(random_int_of(np.array(raw[str(seed)][:count], np.int64), maxes), want)
    else:
        assert seed != 1


@pytest.mark.parametrize("i", range(len(Z["rand_cases"])))
def test_host_compiled_samplers_follow_the_reference(i):
    """The kernels' sampling code compiled for the host (tests/hostemu: the seed window's closed form,
    the draws and the swap-remove) against the sets built from the reference's RandomInt draws."""
    seed, N, minset, count = (int(x) for x in Z["rand_cases"][i])
    want = sample_sets(Z[f"rand.{i}"], N, minset)
    scene = synth.make_pnp_scene(np.random.default_rng(900 + i), N, 0.4)
    draw = he.pnp_hypothesis if minset == 4 else he.mlpnp_hypothesis
    assert len(want) == count // minset
    for h in list(range(0, len(want), 7)) + [len(want) - 1]:
        assert draw(scene, seed, h, minset)[0].tolist() == want[h].tolist(), (seed, N, h)


def test_fixture_is_what_the_built_reference_returns():
    """Live: where build() produced oracle/_ref/ref_dbow2 (a reference tree was present), run it on
    the fixture's inputs and compare every recorded output bit for bit: a stale fixture fails here."""
    if not rio.have_binary():
        pytest.skip("oracle/_ref/ref_dbow2 is not built: no reference tree on this machine")
    out = rio.reference_outputs(Z)
    for v in VOCS:
        out[f"voc.{v}.wweight_tail"] = out[f"voc.{v}.wweight"][int((Z[f"voc.{v}.is_leaf"] > 0).sum()):]
        assert np.array_equal(out.pop(f"voc.{v}.wweight").view(np.uint64), rio.fixture_word_weights(Z, v).view(np.uint64))
    recorded = set(Z.keys())
    assert set(out) <= recorded and len(out) > 300
    for k, a in out.items():
        a, b = np.asarray(a), Z[k]
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    inputs = recorded - set(out)  # everything else in the fixture is an input the outputs were computed from
    assert all(k.split(".")[-1] in ("k", "L", "newline", "parent", "is_leaf", "desc", "weight", "voc", "levelsups",
                                    "id", "raw", "hit", "q_desc", "kf_desc", "levelsup") or "." not in k for k in inputs), inputs
