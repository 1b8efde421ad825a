"""Writes tests/golden/triang_traces.npz from the sequential restatement (tests/triang_ref.py): for every problem of
triang_cases.fixture_problems() the matcher's outputs and trace and the status / x3D of its matched pairs; for every
pair case its status and x3D; for every driver case the literal neighbour loop's outputs.  The problems themselves
are rebuilt by triang_cases (seeded); tests/test_cpu_triang.py checks that they still give these outputs.

    python tests/golden/make_triang_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import triang_cases as tc  # noqa: E402
import triang_ref as tr  # noqa: E402


def build():
    out = {}
    names = []
    for n, (k1, k2, F, only_stereo, check_ori) in tc.fixture_problems().items():
        r = tr.search_for_triangulation(k1, k2, F, only_stereo, check_ori, all_den_zero=True)
        names.append(n)
        out[f"{n}/matches12"] = r["matches12"]
        out[f"{n}/counts"] = np.array([r["nmatches"], r["den_zero"]], np.int32)
        out[f"{n}/den_zero_slot"] = r["den_zero_slot"]
        out[f"{n}/code"], out[f"{n}/bin"] = r["code"].astype(np.int8), r["bin"].astype(np.int8)
        pairs = np.array(tr.matched_pairs(r["matches12"]), np.int32).reshape(-1, 2)
        res = [tr.triangulate_pair(k1, k2, a, b)[:2] for a, b in pairs]
        out[f"{n}/pairs"] = pairs
        out[f"{n}/status"] = np.array([s for s, _ in res], np.int32)
        out[f"{n}/x3d"] = np.array([x for _, x in res], np.float32).reshape(-1, 3)
    out["names"] = np.array(names)
    for n, (k1, k2, i1, i2, *_rest) in tc.pair_cases().items():
        s, x, _ = tr.triangulate_pair(k1, k2, i1, i2)
        out[f"pair/{n}/status"], out[f"pair/{n}/x3d"] = np.int32(s), x
    for n, (cur, neigh, _exp) in tc.driver_cases().items():
        r = tr.create_new_map_points(cur, neigh)
        for k in ("new_neighbour", "new_idx2", "new_pos"):
            out[f"driver/{n}/{k}"] = r[k]
        out[f"driver/{n}/nnew"] = np.int32(r["nnew"])
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "triang_traces.npz")
    np.savez_compressed(path, **build())
    print(path, os.path.getsize(path), "bytes")
