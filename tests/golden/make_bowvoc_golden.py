"""Writes tests/golden/bowvoc_traces.npz: the sequential restatement's (tests/bowvoc_ref.py) outputs
on a 40-node vocabulary (k = 3, L = 3) and 64 descriptors, for levelsup 0..4, with the inputs.
Run from the repository root: python tests/golden/make_bowvoc_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import bowvoc_cases as bc  # noqa: E402
from bowvoc_ref import RefVocabulary  # noqa: E402


def main():
    voc, desc = bc.golden_case()
    assert voc.n_nodes == 40 and len(desc) == 64
    r = RefVocabulary(voc)
    out = dict(k=voc.k, L=voc.L, parent=voc.parent, is_leaf=voc.is_leaf, vdesc=voc.desc, weight=voc.weight, desc=desc,
               words=r.size(), levelsups=np.arange(5))
    for lu in range(5):
        t = r.transform(desc, lu)
        for k in ("word_id", "word_value", "node_id", "node_begin", "feat", "f_word", "f_node", "f_stopped"):
            out[f"l{lu}_{k}"] = t[k]
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "bowvoc_traces.npz"), **out)


if __name__ == "__main__":
    main()
