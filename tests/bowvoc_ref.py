"""TEST-ONLY sequential restatement of DBoW2's vocabulary transform (Frame::ComputeBoW):
TemplatedVocabulary::transform(features, v, fv, levelsup) (TemplatedVocabulary.h:1127-1194), the
per-feature descent (:1218-1259), FORB::distance (FORB.cpp:81-101, a bit count of the XOR),
BowVector::addWeight / normalize(L1) (BowVector.cpp:34-46, :62-84), FeatureVector::addFeature and the
word numbering of loadFromTextFile (:1378-1420).  Python floats are IEEE doubles; every sum is one
add at a time in the reference's order."""
import numpy as np


class UninitialisedNodeId(Exception):
    """The descent reached a leaf above nid_level: the reference leaves *nid unset (:1151, :1251)."""


def _distance(a: int, b: int) -> int:
    """FORB::distance: the number of set bits of a XOR b."""
    return bin(a ^ b).count("1")


def normalize_l1(values):
    """BowVector::normalize(L1) (BowVector.cpp:62-84) on the values in key order -> (norm, values):
    one sum of fabs in std::map order, then one division each, and none when the norm is not > 0."""
    norm = 0.0
    for x in values:
        norm += abs(x)
    return norm, ([x / norm for x in values] if norm > 0.0 else list(values))


class RefVocabulary:
    def __init__(self, voc):
        self.L = int(voc.L)
        n = len(voc.parent)
        self.children = [[] for _ in range(n)]
        for i in range(1, n):  # m_nodes[pid].children.push_back(nid), nid ascending (:1392)
            self.children[int(voc.parent[i])].append(i)
        self.desc = [int.from_bytes(bytes(voc.desc[i]), "little") for i in range(n)]
        self.weight = [float(w) for w in voc.weight]
        self.word_id = [0] * n
        words = 0
        for i in range(1, n):  # nIsLeaf > 0: word_id = m_words.size() (:1408-1415)
            if voc.is_leaf[i] > 0:
                self.word_id[i] = words
                words += 1
        self.words = words

    def size(self):
        return self.words

    def descend(self, feature: int, levelsup: int):
        """transform(feature, word_id, weight, &nid, levelsup) (:1218-1259); nid None = uninitialised."""
        nid_level = self.L - levelsup
        nid = 0 if nid_level <= 0 else None
        final_id, level = 0, 0
        while True:
            level += 1
            nodes = self.children[final_id]
            final_id = nodes[0]
            best = _distance(feature, self.desc[final_id])
            for c in nodes[1:]:
                d = _distance(feature, self.desc[c])
                if d < best:
                    best, final_id = d, c
            if level == nid_level:
                nid = final_id
            if not self.children[final_id]:
                break
        return self.word_id[final_id], self.weight[final_id], nid

    def transform(self, desc, levelsup: int = 4, normalize: bool = True):
        """-> dict: word_id uint32[], word_value float64[] (BowVector in key order), node_id uint32[],
        node_begin int32[], feat uint32[] (FeatureVector as CSR), f_word / f_node uint32[n],
        f_stopped uint8[n] (per feature), norm.  normalize=False leaves out BowVector::normalize (the
        word sums as accumulated; not a reference mode, a window for the tests)."""
        desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        v, fv = {}, {}
        f_word, f_node, f_stop = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        for i in range(n):
            wid, w, nid = self.descend(int.from_bytes(bytes(desc[i]), "little"), levelsup)
            if nid is None:
                raise UninitialisedNodeId(i)
            f_word[i], f_node[i] = wid, nid
            if w > 0:  # not stopped (:1157)
                if wid in v:
                    v[wid] += w  # addWeight: vit->second += v
                else:
                    v[wid] = w
                fv.setdefault(nid, []).append(i)
            else:
                f_stop[i] = 1
        keys = sorted(v)
        norm, normed = normalize_l1([v[k] for k in keys])
        if normalize:
            v = dict(zip(keys, normed))
        nodes = sorted(fv)
        begin = np.zeros(len(nodes) + 1, np.int32)
        feat = []
        for j, k in enumerate(nodes):
            feat += fv[k]
            begin[j + 1] = len(feat)
        return dict(word_id=np.array(keys, np.uint32), word_value=np.array([v[k] for k in keys], np.float64),
                    node_id=np.array(nodes, np.uint32), node_begin=begin, feat=np.array(feat, np.uint32),
                    f_word=f_word, f_node=f_node, f_stopped=f_stop, norm=norm)


def assert_same(got: dict, ref: dict, where=""):
    """Bit-for-bit: integers equal, doubles equal as uint64."""
    for k in ("word_id", "node_id", "node_begin", "feat"):
        assert np.array_equal(np.asarray(got[k]), ref[k]), (where, k, got[k], ref[k])
    assert np.array_equal(np.ascontiguousarray(got["word_value"], np.float64).view(np.uint64),
                          ref["word_value"].view(np.uint64)), (where, "word_value")
    for k in ("f_word", "f_node", "f_stopped"):
        if k in got and k in ref:
            # the word id and node id of a stopped feature are still the descent's
            assert np.array_equal(np.asarray(got[k]), ref[k]), (where, k)
