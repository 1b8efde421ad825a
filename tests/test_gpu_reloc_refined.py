"""Tracking::Relocalization's SearchByProjection refinement on the device (Tracking.cpp:1294-1335):

* rsc_reloc_refine_many on the three branches of the chain in one launch, against reloc_refine_ref;
* rsc_reloc_events_refined on three events in one call — the chain lifts the first success to a match,
  the chain fails and a later candidate matches, no candidate reaches 50 — against run_reloc_refined;
* rsc_reloc_events_gated on the same solvers still hands the first event off, unchanged;
* the C++ facade's ORBmatcher::SearchByProjection on mock Frame / KeyFrame types.
Counts, poses (bit for bit) and the final mvpMapPoints are compared."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import events_oracle as eo
import frameproj_cases as fc
import frameproj_ref as fr
import reloc_refine_cases as rc
from gpu_common import bits, ctx
from rsc import events as rev
from rsc import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "orb-slam2-optimized_amd", "lib", "facade_proj_test")


def kf_view(kf):
    from rsc import engine
    v = engine.KFView(ctx(), kf)
    v.set_angles(kf.angle)
    return v


def test_refine_many_three_branches_one_launch():
    from rsc import engine
    st = rc.chain_states()
    names = ["stage1_short", "stage1_only", "both_stages"]
    want = [fr.reloc_refine_ref(st[n].frame, st[n].kf, dict(u_right=None, bf=0.0), st[n].frame_mp, st[n].found,
                                st[n].n_good_in, st[n].Tcw_in) for n in names]
    assert [w["pose_opts"] for w in want] == [0, 1, 2]  # the branches this launch is meant to cover
    fv = engine.FrameView(ctx(), st[names[0]].frame)
    res, mps = engine.reloc_refine_many(ctx(), [fv] * 3, [kf_view(st[n].kf) for n in names], [(None, 0.0)] * 3,
                                        [st[n].frame_mp for n in names], [st[n].found for n in names],
                                        [st[n].n_good_in for n in names], [st[n].Tcw_in for n in names])
    for k, (n, w) in enumerate(zip(names, want)):
        g = res[k]
        assert (int(g["n_good"]), [int(x) for x in g["n_additional"]], int(g["pose_opts"])) == \
            (w["n_good"], list(w["n_additional"]), w["pose_opts"]), n
        assert np.array_equal(bits(np.asarray(g["Tcw"])), bits(w["Tcw"]).ravel()), n
        assert np.array_equal(mps[k], w["frame_mp"]), n


def _solvers(evs):
    from rsc import engine
    eb = engine.EventBatch([[engine.PnPSolver(ctx(), sc, s) for (_, _, sc), s in zip(cs, sds)] for cs, sds in evs])
    eb.batch.reset(np.array([s for _, sds in evs for s in sds], np.uint32))
    eb.batch.set_ransac_parameters(*rev.RELOC_PARAMS)
    return eb


def test_events_refined_match_reference_and_gated_unchanged():
    from rsc import engine
    p, evs = rc.events()
    want = [fr.run_reloc_refined(p.frame, cs, sds, None, 0.0) for cs, sds in evs]
    # the branches, on the reference's own record
    w0, w1, w2 = want
    assert w0["status"] == eo.GATE_MATCH and w0["winner"] == 0 and 10 <= w0["n_good_first"] < 50 and w0["chains"] == 1
    assert w1["status"] == eo.GATE_MATCH and w1["winner"] == 1 and w1["chains"] >= 2 and w1["rejected"] >= 1
    assert w1["trace"][0][1] == 0 and w1["trace"][0][3] is not None and w1["trace"][0][3]["n_good"] < 50
    assert w2["status"] == eo.GATE_NONE and w2["chains"] >= 1
    eb = _solvers(evs)
    fv = engine.FrameView(ctx(), p.frame)
    kvs = {}
    cands = [[(kvs.setdefault(id(kf), kf_view(kf)), m) for kf, m, _ in cs] for cs, _ in evs]
    res, mps = eb.run_reloc_refined([fv] * len(evs), [(None, 0.0)] * len(evs), cands)
    keys = ("status", "winner", "round", "hypothesis", "n_inliers", "n_good", "rejected", "gates", "n_good_first",
            "chains")
    for e, w in enumerate(want):
        g = res[e]
        assert tuple(int(g[k]) for k in keys) == tuple(int(w[k]) for k in keys), f"event {e}"
        assert [int(x) for x in g["n_additional"]] == list(w["n_additional"]), f"event {e}"
        if w["status"] == eo.GATE_MATCH:
            assert np.array_equal(bits(np.asarray(g["Tcw"])), bits(w["Tcw"])), f"event {e} Tcw"
            assert np.array_equal(mps[e], w["frame_mp"]), f"event {e} mvpMapPoints"
        else:
            assert (mps[e] == -1).all()
    # the gated driver on the same solvers (reset): event 0 is still handed off
    eb.batch.reset(np.array([s for _, sds in evs for s in sds], np.uint32))
    gres, _, _ = eb.run_reloc_gated([(None, 0.0)] * len(evs))
    o = eo.run_reloc_gated([sc for _, _, sc in evs[0][0]], evs[0][1], None, 0.0)
    assert o["status"] == eo.GATE_HANDOFF and int(gres["status"][0]) == eo.GATE_HANDOFF
    assert int(gres["n_good"][0]) == o["n_good"] == w0["n_good_first"]
    assert np.array_equal(bits(np.asarray(gres["Tcw"][0])), bits(o["Tcw"]))


def _proj_bytes(p):
    """facade_proj_test input record of one problem (see tests/cpp/facade_proj_test.cpp)."""
    F, K = p.frame, p.kf
    sf = synth.scale_factors()
    b = struct.pack("<ii", F.n, K.n)
    b += struct.pack("<8f", F.fx, F.fy, F.cx, F.cy, F.min_x, F.max_x, F.min_y, F.max_y)
    b += struct.pack("<2f", synth.GRID_W_INV, synth.GRID_H_INV)
    b += struct.pack("<i", len(sf)) + sf.astype("<f4").tobytes() + struct.pack("<f", synth.LOG_SCALE_FACTOR)
    b += np.asarray(p.Tcw, "<f4").tobytes()
    b += np.ascontiguousarray(F.kp, "<f4").tobytes() + np.ascontiguousarray(F.octave, "<i4").tobytes()
    b += np.ascontiguousarray(F.angle, "<f4").tobytes() + np.ascontiguousarray(F.desc, np.uint8).tobytes()
    b += np.ascontiguousarray(F.cell_begin, "<i4").tobytes() + np.ascontiguousarray(F.cell_feat, "<i4").tobytes()
    b += np.ascontiguousarray(p.frame_mp, "<i4").tobytes()
    b += np.ascontiguousarray(K.angle, "<f4").tobytes() + np.ascontiguousarray(K.mp_state, np.uint8).tobytes()
    b += np.ascontiguousarray(K.mp_pos, "<f4").tobytes() + np.ascontiguousarray(K.mp_dmax, "<f4").tobytes()
    b += np.ascontiguousarray(K.mp_dmin, "<f4").tobytes() + np.ascontiguousarray(K.mp_desc, np.uint8).tobytes()
    b += np.ascontiguousarray(p.already, np.uint8).tobytes()
    b += struct.pack("<fii", p.th, p.orb_dist, int(p.check_orientation))
    return b


def test_facade_search_by_projection():
    """rsc_orb::ORBmatcher::SearchByProjection(Frame&, KeyFrame, sAlreadyFound, th, ORBdist) on mock types:
    the return value and CurrentFrame.mvpMapPoints after the call equal the reference, per call and in
    the Many form."""
    ps = [fc.random_problem(61, 300, 500, 10, 100, n_clusters=6), fc.random_problem(62, 300, 500, 3, 64, n_clusters=6),
          fc.random_problem(63, 200, 400, 10, 100, n_clusters=4)]
    ps[1].check_orientation = False
    buf = struct.pack("<i", len(ps)) + b"".join(_proj_bytes(p) for p in ps)
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        open(a, "wb").write(buf)
        subprocess.run([BIN, a, b], check=True, timeout=120)
        out = np.frombuffer(open(b, "rb").read(), "<i4")
    pos = 0
    for form in range(2):  # single calls, then one SearchByProjectionMany over the checked problems
        for p in ps:
            if form == 1 and not p.check_orientation:
                continue  # the Many form runs the problems that share the matcher's setting
            n, o = fr.search_by_projection(p.frame, p.kf, p.Tcw, p.already, p.frame_mp, p.th, p.orb_dist,
                                           p.check_orientation)
            assert n > 20
            assert out[pos] == n
            # mvpMapPoints as KeyFrame slots: entry value where set, else the new match
            exp = np.where(p.frame_mp >= 0, p.frame_mp, o)
            assert np.array_equal(out[pos + 1:pos + 1 + p.frame.n], exp)
            pos += 1 + p.frame.n
    assert pos == len(out)
