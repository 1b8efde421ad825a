"""Files exchanged with the built reference DBoW2 (oracle/ref_dbow2_driver.cpp, binary
oracle/_ref/ref_dbow2): the one writer of the ORBvoc.txt text form, the binary request writers, the
readers of the driver's raw little-endian outputs, and run_*() wrappers that call the binary in a
scratch directory.  Used by tests/golden/make_ref_dbow2_golden.py and the tests; numpy only."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "oracle", "_ref", "ref_dbow2")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_dbow2.npz")


def vocabulary_text(k, L, parent, is_leaf, desc, weight, trailing_newline=True, scoring=0, weighting=0) -> str:
    """The ORBvoc.txt format: `k L scoring weighting`, then `parent isLeaf b0 .. b31 weight` per node
    (the root has no line).  Weights carry 17 significant digits, which round-trip a double."""
    lines = [f"{int(k)} {int(L)} {int(scoring)} {int(weighting)}"]
    for i in range(1, len(parent)):
        lines.append(f"{int(parent[i])} {int(is_leaf[i])} " + " ".join(str(int(b)) for b in desc[i]) +
                     f" {float(weight[i]):.17g}")
    return "\n".join(lines) + ("\n" if trailing_newline else "")


def write_vocabulary(path, k, L, parent, is_leaf, desc, weight, trailing_newline=True):
    with open(path, "w") as f:
        f.write(vocabulary_text(k, L, parent, is_leaf, desc, weight, trailing_newline))


def bow_bytes(ids, vals) -> bytes:
    ids, vals = np.ascontiguousarray(ids, "<u4"), np.ascontiguousarray(vals, "<f8")
    assert len(ids) == len(vals)
    return np.uint32(len(ids)).astype("<u4").tobytes() + ids.tobytes() + vals.tobytes()


def _take(buf, pos, dtype, n):
    a = np.frombuffer(buf, dtype, n, pos).copy()
    return a, pos + a.nbytes


def parse_bow(buf, pos=0):
    (n,), pos = _take(buf, pos, "<u4", 1)
    ids, pos = _take(buf, pos, "<u4", int(n))
    vals, pos = _take(buf, pos, "<f8", int(n))
    return ids, vals, pos


def parse_load(buf) -> dict:
    """-> size, chain uint32 [size, nl] (getParentNode(w, l)), weight float64 [size]"""
    (size, nl), pos = _take(buf, 0, "<u4", 2)
    chain, pos = _take(buf, pos, "<u4", int(size) * int(nl))
    weight, pos = _take(buf, pos, "<f8", int(size))
    assert pos == len(buf)
    return dict(size=int(size), chain=chain.reshape(int(size), int(nl)), weight=weight)


def parse_transform(buf) -> dict:
    """-> the keys of bowvoc_ref.RefVocabulary.transform that the reference's public API gives"""
    ids, vals, pos = parse_bow(buf)
    (nn,), pos = _take(buf, pos, "<u4", 1)
    node_id, pos = _take(buf, pos, "<u4", int(nn))
    begin, pos = _take(buf, pos, "<u4", int(nn) + 1)
    feat, pos = _take(buf, pos, "<u4", int(begin[-1]))
    assert pos == len(buf)
    return dict(word_id=ids, word_value=vals, node_id=node_id, node_begin=begin.astype(np.int32), feat=feat)


def have_binary() -> bool:
    return os.path.exists(BINARY)


def _run(args, files: dict) -> bytes:
    """Runs the binary with the named request files written first; `@name` in args is a path in the
    scratch directory; the last argument is the output file, whose bytes are returned."""
    with tempfile.TemporaryDirectory() as d:
        for name, data in files.items():
            with open(os.path.join(d, name), "wb") as f:
                f.write(data if isinstance(data, bytes) else data.encode())
        argv = [BINARY] + [os.path.join(d, a[1:]) if str(a).startswith("@") else str(a) for a in args] + [os.path.join(d, "out")]
        p = subprocess.run(argv, capture_output=True, timeout=120)
        assert p.returncode == 0, (args, p.returncode, p.stderr.decode()[-400:])
        with open(os.path.join(d, "out"), "rb") as f:
            return f.read()


def run_load(text: str) -> dict:
    return parse_load(_run(["load", "@voc.txt"], {"voc.txt": text}))


def run_transform(text: str, desc, levelsup: int) -> dict:
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    return parse_transform(_run(["transform", "@voc.txt", "@desc.bin", int(levelsup)],
                                {"voc.txt": text, "desc.bin": d.tobytes()}))


def run_score(ids_a, vals_a, ids_b, vals_b):
    """-> (double bits uint64, float bits uint32) of L1Scoring::score(a, b)"""
    buf = _run(["score", "@a.bin", "@b.bin"], {"a.bin": bow_bytes(ids_a, vals_a), "b.bin": bow_bytes(ids_b, vals_b)})
    assert len(buf) == 12
    return int(np.frombuffer(buf, "<u8", 1, 0)[0]), int(np.frombuffer(buf, "<u4", 1, 8)[0])


def run_normalize(ids, vals):
    i, v, pos = parse_bow(_run(["normalize", "@a.bin"], {"a.bin": bow_bytes(ids, vals)}))
    return i, v


def run_randint(seed: int, N: int, minset: int, count: int) -> np.ndarray:
    return np.frombuffer(_run(["randint", seed, N, minset, count], {}), "<i4").copy()


# ---- the fixture (tests/golden/ref_dbow2.npz): inputs -> the reference's outputs ------------------
TRANSFORM_KEYS = ("word_id", "word_value", "node_id", "node_begin", "feat")


def names(z, key):
    return [str(x) for x in z[key]]


def fixture_vocabulary_text(z, v: str) -> str:
    """The text file of fixture vocabulary v, as the generator gave it to the reference."""
    return vocabulary_text(int(z[f"voc.{v}.k"]), int(z[f"voc.{v}.L"]), z[f"voc.{v}.parent"], z[f"voc.{v}.is_leaf"],
                           z[f"voc.{v}.desc"], z[f"voc.{v}.weight"], bool(z[f"voc.{v}.newline"]))


def fixture_word_weights(z, v: str) -> np.ndarray:
    """getWordWeight of every word of fixture vocabulary v: the generator asserts that the words of
    the file carry the stored weights bit for bit, so the fixture keeps only what follows them (the
    trailing-newline word)."""
    return np.concatenate([z[f"voc.{v}.weight"][z[f"voc.{v}.is_leaf"] > 0], z[f"voc.{v}.wweight_tail"]])


def fixture_vector(z, name: str):
    """(ids, values) of a fixture vector: `x.raw` as drawn, `x` as the reference's normalize left it."""
    raw = name.endswith(".raw")
    base = name[:-4] if raw else name
    return z[f"vec.{base}.id"], z[f"vec.{base}.raw" if raw else f"vec.{base}.val"]


def reference_outputs(z) -> dict:
    """Runs the built reference on the fixture's inputs z (a mapping of arrays) and returns every
    output the fixture records, under the fixture's keys.  The normalised vectors are outputs
    (BowVector::normalize of the raw ones) and, as just computed, the inputs of the scores."""
    out = {}
    for v in names(z, "vocs"):
        r = run_load(fixture_vocabulary_text(z, v))
        out[f"voc.{v}.size"] = np.int64(r["size"])
        out[f"voc.{v}.chain"] = r["chain"]
        out[f"voc.{v}.wweight"] = r["weight"]
    for t in names(z, "tcases"):
        text = fixture_vocabulary_text(z, str(z[f"t.{t}.voc"]))
        for lu in z[f"t.{t}.levelsups"]:
            r = run_transform(text, z[f"t.{t}.desc"], int(lu))
            for k in TRANSFORM_KEYS:
                out[f"t.{t}.l{int(lu)}.{k}"] = r[k]
    for n in names(z, "vecs"):
        ids, vals = run_normalize(z[f"vec.{n}.id"], z[f"vec.{n}.raw"])
        assert np.array_equal(ids, z[f"vec.{n}.id"]), n
        out[f"vec.{n}.val"] = vals
    src = {k: z[k] for k in z.keys() if k.startswith("vec.")}
    src.update({k: out[k] for k in out if k.startswith("vec.")})
    b64, b32 = [], []
    for a, b in zip(names(z, "spair_a"), names(z, "spair_b")):
        s64, s32 = run_score(*fixture_vector(src, a), *fixture_vector(src, b))
        b64.append(s64)
        b32.append(s32)
    out["spair_bits64"] = np.array(b64, np.uint64)
    out["spair_bits32"] = np.array(b32, np.uint32)
    for i, (seed, N, minset, count) in enumerate(z["rand_cases"]):
        out[f"rand.{i}"] = run_randint(int(seed), int(N), int(minset), int(count)).astype(np.int32)
    text = fixture_vocabulary_text(z, str(z["chain.voc"]))
    q = run_transform(text, z["chain.q_desc"], int(z["chain.levelsup"]))
    kf = run_transform(text, z["chain.kf_desc"], int(z["chain.levelsup"]))
    s64, s32 = run_score(q["word_id"], q["word_value"], kf["word_id"], kf["word_value"])
    out["chain.bits64"], out["chain.bits32"] = np.uint64(s64), np.uint32(s32)
    return out
