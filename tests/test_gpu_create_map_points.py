"""LocalMapping::CreateNewMapPoints' neighbour loop on the device (rsc_create_new_map_points_many: one matcher launch
and one triangulation launch from the initial slots, the neighbour order replayed on the host) against the literal
loop of the restatement (tests/triang_ref.py create_new_map_points, slots filled as it goes): new_neighbour,
new_idx2, new_pos bits and nnew."""
import os

import numpy as np
import pytest

import triang_cases as tc
import triang_gpu as tg
import triang_ref as tr
from gpu_common import ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(problems):
    from rsc import engine
    cur = [tg.views(p[0]) for p in problems]
    nb = [[tg.views(k) for k in p[1]] for p in problems]
    return engine.create_new_map_points_many(ctx(), [v[0] for v in cur], [v[1] for v in cur],
                                             [[v[0] for v in vs] for vs in nb], [[v[1] for v in vs] for vs in nb])


def same(r, c, ref):
    assert np.array_equal(r["new_neighbour"][c], ref["new_neighbour"]), (r["new_neighbour"][c], ref["new_neighbour"])
    assert np.array_equal(r["new_idx2"][c], ref["new_idx2"])
    assert np.array_equal(r["new_pos"][c].view(np.uint32), ref["new_pos"].view(np.uint32))
    assert int(r["nnew"][c]) == ref["nnew"]


def test_driver_cases():
    """The hand-built driver cases in one call: a slot matched by two neighbours where the first succeeds / fails
    triangulation, a neighbour below the baseline, a neighbour voided by a den == 0 slot and the same neighbour not
    voided because an earlier one filled that slot."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "triang_traces.npz"))
    cs = tc.driver_cases()
    names = list(cs)
    r = run([cs[n] for n in names])
    for c, n in enumerate(names):
        ref = {k: g[f"driver/{n}/{k}"] for k in ("new_neighbour", "new_idx2", "new_pos")}
        ref["nnew"] = int(g[f"driver/{n}/nnew"])
        same(r, c, ref)
        for slot, want in enumerate(cs[n][2]):  # the worked answer
            assert want is None or int(r["new_neighbour"][c][slot]) == want, (n, slot)
    assert int(r["nnew"][names.index("den_zero_voids")]) == 0
    assert int(r["nnew"][names.index("den_zero_filled")]) >= 3


def test_batch_of_three():
    """Three current KeyFrames with 1, 4 and 10 neighbours in one call (and a KeyFrame with none)."""
    rng = np.random.default_rng(31)
    problems = []
    for nn in (1, 4, 10, 0):
        poses = [(tc.I3, (0, 0, 0))] + [(tc.I3, (rng.uniform(-0.8, 0.8), rng.uniform(-0.2, 0.2), rng.uniform(-0.5, 0.5)))
                                        for _ in range(nn)]
        kfs, _ = tc.scene(rng, poses, 60, mp_frac=0.3, node_groups=7, stereo_frac=0.3, noise=0.4, flips=20)
        problems.append((kfs[0], kfs[1:]))
    r = run(problems)
    total = 0
    for c, (cur, nb) in enumerate(problems):
        ref = tr.create_new_map_points(cur, nb)
        same(r, c, ref)
        total += ref["nnew"]
    assert total >= 30 and int(r["nnew"][3]) == 0
    assert len({int(v) for v in r["new_neighbour"][2] if v >= 0}) >= 3  # later neighbours still contribute
