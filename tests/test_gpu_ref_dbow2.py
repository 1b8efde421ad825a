"""Device stages against the BUILT REFERENCE DBoW2, through the committed fixture
tests/golden/ref_dbow2.npz (tests/golden/make_ref_dbow2_golden.py: outputs of the reference's own
loadFromTextFile / transform / L1Scoring::score / RandomInt, compiled unmodified).  No tolerance: word
and node ids, feature lists, doubles as uint64 and the float score as uint32 equal the reference's.

* bowvoc.hip: Vocabulary.transform on every transform case of the fixture;
* kfdb.hip: the L1 score as the database computes it, read back through state();
* the chain descriptors -> transform -> add / detect_relocalization -> score;
* the PnP sampler's on-device seed window against the reference's Random.cpp draws.

Only the fixture is read here; nothing needs the reference tree or the reference binary."""
import numpy as np
import pytest

import bowvoc_cases as bc
import ref_dbow2_io as rio
from bowvoc_ref import assert_same
from gpu_common import ctx
from rsc import engine, synth
from rsc import workloads as wl

pytestmark = pytest.mark.gpu
Z = np.load(rio.FIXTURE)
CASES = rio.names(Z, "tcases")


def want(case, lu):
    return {k: Z[f"t.{case}.l{int(lu)}.{k}"] for k in rio.TRANSFORM_KEYS}


def sample_sets(draws, N, minset):
    """The minimal sets PnPsolver::iterate builds from consecutive RandomInt draws by swap-remove
    (src/PnPsolver.cpp:125-137), mvAllIndices being 0..N-1."""
    sets = np.zeros((len(draws) // minset, minset), np.int32)
    for h in range(len(sets)):
        avail = list(range(N))                      # :125  vAvailableIndices = mvAllIndices
        for i in range(minset):                     # :128
            randi = int(draws[h * minset + i])      # :130  RandomInt(0, vAvailableIndices.size()-1)
            sets[h, i] = avail[randi]               # :132
            avail[randi] = avail[-1]                # :136
            avail.pop()                             # :137
    return sets


@pytest.mark.parametrize("case", [c for c in CASES if c != "deep"])
def test_transform_equals_the_reference(case):
    name = str(Z[f"t.{case}.voc"])
    g = engine.Vocabulary(ctx(), bc.fixture_vocabulary(Z, name))
    assert g.size == int(Z[f"voc.{name}.size"])
    for lu in Z[f"t.{case}.levelsups"]:
        assert_same(g.transform(Z[f"t.{case}.desc"], int(lu)), want(case, lu), (case, int(lu)))
    g.close()


@pytest.mark.parametrize("budget,nodes,levels", [(40, 1, 1), (1000, 21, 3), (0, 341, 5)])
def test_deep_tree_equals_the_reference_at_every_lds_cut(budget, nodes, levels):
    """k = 4, L = 6 with the staging cut after the root, after level 2 and at the default budget
    (tests/test_gpu_bowvoc.py test_deep_tree_lds_cut)."""
    g = engine.Vocabulary(ctx(), bc.fixture_vocabulary(Z, "k4l6"), lds_budget_bytes=budget)
    info = g.info()
    assert (info["lds_nodes"], info["lds_levels"]) == (nodes, levels), info
    for lu in Z["t.deep.levelsups"]:
        assert_same(g.transform(Z["t.deep.desc"], int(lu)), want("deep", lu), (budget, int(lu)))
    g.close()


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def test_score_through_the_database():
    """Each score pair: one vector added as a KeyFrame, the other the query; mRelocScore's bits equal
    the reference's `float si = score(...)`.  With one KeyFrame the common-words cut passes every
    pair that shares a word, so only the no-overlap pairs go unscored."""
    ids_max = max(int(Z[f"vec.{n}.id"].max()) for n in rio.names(Z, "vecs") if len(Z[f"vec.{n}.id"]))
    db = engine.KeyFrameDatabase(ctx(), 1, max_words=4096, vocab_words=ids_max + 1)
    scored = []
    kinds, sizes = rio.names(Z, "spair_kind"), Z["spair_n"]
    for i, (a, b) in enumerate(zip(rio.names(Z, "spair_a"), rio.names(Z, "spair_b"))):
        (ia, va), (ib, vb) = rio.fixture_vector(Z, a), rio.fixture_vector(Z, b)
        common = len(np.intersect1d(ia, ib))
        db.add(0, ib, vb)
        cand = db.detect_relocalization(100 + i, ia, va)
        (_, rq), (_, rw), (_, rs) = db.state(0)
        if rq == 100 + i:
            assert rw == common > 0 and list(cand) == [0], (a, b)
            print(f"{a} x {b}: device {f32_bits(rs):08x} reference {int(Z['spair_bits32'][i]):08x}")
            assert f32_bits(rs) == int(Z["spair_bits32"][i]), (a, b, rs)
            scored.append((kinds[i], int(sizes[i])))
        else:
            assert common == 0 and len(cand) == 0, (a, b)
        db.release(0)
    assert len(scored) >= 12
    for kind, n in zip(kinds, sizes):
        if kind.split(".")[0] in ("half", "all", "identical"):
            assert (kind, int(n)) in scored, (kind, n)
    assert {1024, 1025, 4096} <= {n for _, n in scored}  # the count kernel's second batch
    db.close()


def test_descriptors_to_score_chain():
    """descriptors -> device transform -> add / detect_relocalization -> score equals the reference's
    score(transform(q), transform(kf)) on the k = 10, L = 3 vocabulary."""
    name, lu = str(Z["chain.voc"]), int(Z["chain.levelsup"])
    g = engine.Vocabulary(ctx(), bc.fixture_vocabulary(Z, name))
    q, kf = g.transform(Z["chain.q_desc"], lu), g.transform(Z["chain.kf_desc"], lu)
    db = engine.KeyFrameDatabase(ctx(), 1, vocab_words=g.size)
    db.add(0, kf["word_id"], kf["word_value"])
    assert list(db.detect_relocalization(7, q["word_id"], q["word_value"])) == [0]
    (_, rq), _, (_, rs) = db.state(0)
    assert rq == 7 and f32_bits(rs) == int(Z["chain.bits32"]), (rs, hex(int(Z["chain.bits32"])))
    db.close()
    g.close()


def test_pnp_samples_follow_the_reference_random_int():
    """Exhaustive PnP runs (at most 45 % inliers, tests/test_gpu_degenerate.py: no success cuts the
    stream): the 300 sampled sets equal the ones swap-remove builds from the reference's RandomInt
    draws after srand(seed), for the fixture's seeds and N."""
    cases = [(i, int(s), int(N)) for i, (s, N, m, _) in enumerate(Z["rand_cases"]) if m == 4]
    assert len(cases) == 9
    scenes = [synth.make_pnp_scene(np.random.default_rng(900 + i), N, 0.4) for i, _, N in cases]
    gs = [engine.PnPSolver(ctx(), sc, seed) for sc, (_, seed, _) in zip(scenes, cases)]
    b = engine.SolverBatch(gs)
    b.set_ransac_parameters(*wl.RELOC)
    outs = b.iterate(300, with_masks=True)
    for g, o, (i, seed, N) in zip(gs, outs, cases):
        assert not o["ok"] and o["iterations"] == 300, (seed, N, o)
        ref = sample_sets(Z[f"rand.{i}"], N, 4)
        assert len(ref) == 300 and np.array_equal(g.last_samples(400)[:, :4], ref), (seed, N)
