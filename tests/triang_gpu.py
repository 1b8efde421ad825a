"""Device views of the KeyFrame namespaces of tests/triang_cases.py (shared by the triangulation GPU tests)."""
import numpy as np

from gpu_common import ctx

INPUTS = ("kp", "kp_raw", "octave", "desc", "angle", "u_right", "depth", "cos_parallax_stereo", "mp_state", "node_id",
          "node_begin", "feat", "Rcw", "tcw", "Rwc", "Ow", "Kinv")


def views(k, triangulation=True):
    """(BowView, KFView with set_triangulation) of one KeyFrame."""
    from rsc import engine
    b = engine.BowView(ctx(), k)
    v = engine.KFView(ctx(), k)
    if triangulation:
        v.set_triangulation(k)
    return b, v


def snapshot(kfs):
    return [[np.array(getattr(k, a)).copy() for a in INPUTS] for k in kfs]


def unchanged(kfs, snap):
    return all(np.array_equal(np.array(getattr(k, a)), s, equal_nan=True) for k, ss in zip(kfs, snap)
               for a, s in zip(INPUTS, ss))
