"""GPU parity of the EPnP eigen stage at the edges of its work units, bit for bit against the oracle's
trace (every hypothesis' sample, inlier count and float pose).

The split form (pnp_eig_split_kernel) packs 20 hypotheses into a unit (a chase wave and a row wave)
and four units into a workgroup; the pair form (pnp_eig_group_kernel) 20 hypotheses into a
single-wave workgroup.  H in {1, 19, 20, 21, 79, 80, 81} at N = 64 puts the last hypothesis one
short of, on and one past a unit's and a workgroup's end: a last unit with one lane pair, a workgroup
with three idle units, a second workgroup holding one hypothesis.  Both forms are forced onto these
small launches (set_eig_rows(0): the rows form, their default, is switched off).
tests/test_gpu_chase_bookkeeping.py covers the chase inside full units."""
import numpy as np
import pytest

from gpu_common import assert_pnp_equal, bits
import oracle_lib as ol
from rsc import synth

pytestmark = pytest.mark.gpu

EDGES = (1, 19, 20, 21, 79, 80, 81)
# max iterations 1: the budget alone sets the hypothesis count; 40 % inliers against epsilon 0.5:
# no hypothesis qualifies, every one is evaluated
PARAMS = (0.99, 10, 1, 4, 0.5, 5.991)
SEED = 6100

_REF = {}


def _reference(h):
    """The scene (shared by all cases) and the oracle's trace of iterate(h), computed once per h."""
    if "scene" not in _REF:
        _REF["scene"] = synth.make_pnp_scene(np.random.default_rng(SEED), 64, 0.4)
    if h not in _REF:
        o = ol.OraclePnP(_REF["scene"], SEED + h)
        o.set_ransac_parameters(*PARAMS)
        o.enable_trace()
        ro = o.iterate(h)
        ints, fl = o.trace()
        assert not ro["ok"] and len(ints) == h
        _REF[h] = (ro, ints, fl)
    return (_REF["scene"],) + _REF[h]


@pytest.fixture(scope="module", params=["split", "pairs"])
def form_ctx(request):
    from rsc import engine
    c = engine.Context(0)
    c.set_eig_rows(0)
    c.set_eig_split(request.param == "split")
    yield c
    c.close()


@pytest.mark.parametrize("h", EDGES)
def test_unit_and_workgroup_edges(form_ctx, h):
    from rsc import engine
    sc, ro, ints, fl = _reference(h)
    g = engine.PnPSolver(form_ctx, sc, SEED + h)
    g.set_ransac_parameters(*PARAMS)
    rg = g.iterate(h)
    assert_pnp_equal(rg, ro, f"H={h}")
    assert rg["iterations"] == ro["iterations"] == h
    cnt, pos = g.last_hypotheses(128)
    smp = g.last_samples(128)
    assert len(cnt) == len(smp) == h
    assert np.array_equal(smp[:, :4], ints[:, :4]), f"H={h} samples"
    assert np.array_equal(cnt, ints[:, 8]), f"H={h} counts"
    assert np.array_equal(bits(pos), bits(fl)), f"H={h} poses"
    g.close()
