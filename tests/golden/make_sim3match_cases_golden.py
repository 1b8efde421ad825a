"""Writes tests/golden/sim3match_cases.npz: the hand-built SearchBySim3 cases of tests/sim3match_cases.py
(every distinct KeyFrame once, then per case its two KeyFrame numbers, R12, t12, matched12 and th) with the
answers vnMatch1, vnMatch2, out12 and nFound.  The answers are written only where the Python restatement
(tests/sim3match_ref.py), the oracle's trace and the hand-written expectations agree.

    python tests/golden/make_sim3match_cases_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle_lib as ol  # noqa: E402
import sim3match_cases as sc  # noqa: E402
import sim3match_ref as sr  # noqa: E402


def build() -> dict:
    """Few large arrays instead of many small ones (an .npz entry costs more than a small case): KeyFrame k
    owns rows kf_off[k] : kf_off[k + 1] of every per-slot array, cell_feat rows feat_off[k] : feat_off[k + 1],
    scale factors sf_off[k] : sf_off[k + 1]; case c owns rows c1_off[c] : c1_off[c + 1] of m12 / m1 / out and
    c2_off[c] : c2_off[c + 1] of m2."""
    kfs, kf_no, names, rows = [], {}, [], []

    def number(kf):
        if id(kf) not in kf_no:
            kf_no[id(kf)] = len(kfs)
            kfs.append(kf)
        return kf_no[id(kf)]

    for group, (th, cases) in sc.groups().items():
        for name, c in cases:
            names.append(f"{group}:{name}")
            nf, out, m1, m2, r1, r2 = ol.search_by_sim3_trace(c.kf1, c.kf2, c.R12, c.t12, c.m12, th)
            t = sr.py_trace(c.kf1, c.kf2, c.R12, c.t12, c.m12, th)
            assert nf == t.nfound and np.array_equal(out, t.out), names[-1]
            assert np.array_equal(m1, t.m1) and np.array_equal(m2, t.m2), names[-1]
            for want, got in ((c.m1, m1), (c.m2, m2), (c.out, out)):
                pinned = want != sc.UNPINNED
                assert np.array_equal(want[pinned], got[pinned]), names[-1]
            rows.append((number(c.kf1), number(c.kf2), th, c, nf, out, m1, m2))

    def cat(arrays, dtype, tail=()):
        return np.concatenate([np.asarray(a, dtype).reshape((-1,) + tail) for a in arrays] or
                              [np.zeros((0,) + tail, dtype)])

    def offsets(sizes):
        return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)

    d = {"names": np.array(names), "kf_off": offsets([k.n for k in kfs]),
         "feat_off": offsets([len(k.cell_feat) for k in kfs]), "sf_off": offsets([len(k.scale_factors) for k in kfs]),
         "kp": cat([k.kp for k in kfs], np.float32, (2,)), "octave": cat([k.octave for k in kfs], np.int32),
         "desc": cat([k.desc for k in kfs], np.uint8, (32,)), "mp_desc": cat([k.mp_desc for k in kfs], np.uint8, (32,)),
         "cell_begin": np.stack([np.asarray(k.cell_begin, np.int32) for k in kfs]),
         "cell_feat": cat([k.cell_feat for k in kfs], np.int32),
         "scale_factors": cat([k.scale_factors for k in kfs], np.float32),
         "Rcw": np.stack([np.asarray(k.Rcw, np.float32).reshape(3, 3) for k in kfs]),
         "tcw": np.stack([np.asarray(k.tcw, np.float32).reshape(3) for k in kfs]),
         "mp_state": cat([k.mp_state for k in kfs], np.uint8), "mp_pos": cat([k.mp_pos for k in kfs], np.float32, (3,)),
         "mp_dmax": cat([k.mp_dmax for k in kfs], np.float32), "mp_dmin": cat([k.mp_dmin for k in kfs], np.float32),
         "geom": np.array([[k.fx, k.fy, k.cx, k.cy, k.min_x, k.max_x, k.min_y, k.max_y, k.log_scale_factor,
                            k.grid_w_inv, k.grid_h_inv] for k in kfs], np.float32),
         "case_kf": np.array([[r[0], r[1]] for r in rows], np.int32), "case_th": np.array([r[2] for r in rows], np.float32),
         "case_R12": np.stack([r[3].R12 for r in rows]), "case_t12": np.stack([r[3].t12 for r in rows]),
         "case_n": np.array([r[4] for r in rows], np.int32),
         "c1_off": offsets([r[3].kf1.n for r in rows]), "c2_off": offsets([r[3].kf2.n for r in rows]),
         "m12": cat([r[3].m12 for r in rows], np.int32), "out": cat([r[5] for r in rows], np.int32),
         "m1": cat([r[6] for r in rows], np.int32), "m2": cat([r[7] for r in rows], np.int32)}
    return d


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "sim3match_cases.npz")
    np.savez_compressed(out, **build())
    print(out, os.path.getsize(out), "bytes")
