"""rsc_orb::ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) and ::Fuse(pKF, Scw, vpPoints, th,
vpReplacePoint) on mock KeyFrame / MapPoint types (tests/cpp/facade_loopproj_test.cpp): vpMatched, the return
values, vpReplacePoint and the KeyFrame's slots after the calls equal the restatement (tests/kfproj_ref.py),
per call and in the Many forms."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import kfproj_cases as kc
import kfproj_ref as kr
from rsc import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "orb-slam2-optimized_amd", "lib", "facade_loopproj_test")
OTHER = 1000000  # id of a MapPoint that is not in the list: OTHER + slot


def _points(pts) -> bytes:
    return struct.pack("<i", pts.n) + b"".join(np.ascontiguousarray(a, dt).tobytes() for a, dt in (
        (pts.state, np.uint8), (pts.pos, np.float32), (pts.normal, np.float32), (pts.dmax, np.float32),
        (pts.dmin, np.float32), (pts.desc, np.uint8)))


def _problem(kf, Scw, slots, th) -> bytes:
    sf = synth.scale_factors()
    b = struct.pack("<i4f4i2fi", kf.n, kf.fx, kf.fy, kf.cx, kf.cy, int(kf.min_x), int(kf.max_x), int(kf.min_y),
                    int(kf.max_y), float(synth.GRID_W_INV), float(synth.GRID_H_INV), len(sf))
    b += sf.tobytes() + struct.pack("<f", float(synth.LOG_SCALE_FACTOR))
    b += np.ascontiguousarray(Scw, np.float32).tobytes()
    b += b"".join(np.ascontiguousarray(a, dt).tobytes() for a, dt in (
        (kf.kp, np.float32), (kf.octave, np.int32), (kf.desc, np.uint8), (kf.cell_begin, np.int32),
        (kf.cell_feat, np.int32), (slots, np.int32)))
    return b + struct.pack("<f", float(th))


def _search_slots(p):
    """vpMatched on entry as slot codes: occupied slots hold the `already` points first, then other MapPoints."""
    occ = np.nonzero(p.occupied)[0]
    al = np.nonzero(p.already)[0]
    assert len(al) <= len(occ)
    slots = np.full(p.kf.n, -1, np.int32)
    slots[occ] = -2
    slots[occ[:len(al)]] = al
    return slots


def _fuse_slots(kf, in_kf, pts):
    """The KeyFrame's own slots: the list's points that are in the KeyFrame sit on slots of their state."""
    slots = np.where(kf.mp_state == 1, -2, np.where(kf.mp_state == 2, -3, -1)).astype(np.int32)
    s = np.nonzero(kf.mp_state == 1)[0]
    q = np.nonzero(in_kf == 1)[0]
    assert len(q) <= len(s) and (pts.state[q] == 1).all()
    slots[s[:len(q)]] = q
    return slots


def test_facade_loop_projection_and_fuse():
    z = np.load(os.path.join(ROOT, "tests", "golden", "kfproj_traces.npz"))
    cs = kc.cases()
    search = [cs[n][0] for n in ("greedy_order", "occupied_on_entry", "z_zero", "level_above")]
    big = kc.from_arrays(z, "random_a")
    big.already = big.already.copy()
    big.already[np.nonzero(big.already)[0][int(big.occupied.sum()):]] = 0  # every such point needs a slot to sit on
    search.append(big)
    blob = struct.pack("<i", len(search))
    for p in search:
        blob += _points(p.pts) + _problem(p.kf, p.Scw, _search_slots(p), p.th)
    fuse = []
    for k in range(len(z["fuse/Scw"])):
        kf = kc.make_kf(big.kf.kp, big.kf.octave, big.kf.desc, z["fuse/mp_state"][k])
        # a bad point is skipped whether or not the KeyFrame holds it, and GetMapPoints() lists no bad ones
        fuse.append((kf, z["fuse/Scw"][k], np.where(big.pts.state == 1, z["fuse/in_kf"][k], 0).astype(np.uint8)))
    th = float(z["fuse/th"][0])
    blob += struct.pack("<i", len(fuse)) + _points(big.pts)
    fslots = [_fuse_slots(kf, ik, big.pts) for kf, _, ik in fuse]
    for (kf, S, ik), sl in zip(fuse, fslots):
        blob += _problem(kf, S, sl, th)
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        open(a, "wb").write(blob)
        subprocess.run([BIN, a, b], check=True, timeout=120)
        out = np.frombuffer(open(b, "rb").read(), "<i4")
    pos = 0
    want = []
    for p in search:
        n, o = kr.search_by_projection_kf(p.kf, p.pts, p.Scw, p.already, p.occupied, p.th)
        ids = _search_slots(p)
        ids = np.where(ids == -2, OTHER + np.arange(p.kf.n), ids)
        want.append((n, np.where(o >= 0, o, ids)))
    assert want[-1][0] >= 100
    for form in range(2):  # single calls, then one SearchByProjectionMany
        for n, ids in want:
            assert int(out[pos]) == n, form
            assert np.array_equal(out[pos + 1:pos + 1 + len(ids)], ids), form
            pos += 1 + len(ids)
    fwant = []
    for (kf, S, ik), sl in zip(fuse, fslots):
        r = kr.fuse(kf, big.pts, S, ik, th)
        assert np.array_equal(r["best_idx"], z["fuse/best_idx"][len(fwant)])
        before = np.where(sl <= -2, OTHER + np.arange(kf.n), sl)
        rep = np.where(r["replace"] >= 0, before[np.maximum(r["replace"], 0)], -1)
        rep = np.where(r["holder"] >= 0, r["holder"], rep)  # the slot was filled by an earlier point of this call
        assert (r["holder"] >= 0).sum() >= 1
        after = before.copy()
        for i in np.nonzero(r["added"] >= 0)[0]:  # :938-939 in list order: the last point added to a slot stays
            after[r["added"][i]] = i
        fwant.append((r["nfused"], rep, after, int((r["added"] >= 0).sum())))
    assert sum(w[3] for w in fwant) >= 50 and all((w[1] >= 0).sum() >= 10 for w in fwant)
    for form in range(2):  # single calls, then one FuseMany
        for n, rep, after, _ in fwant:
            assert int(out[pos]) == n, form
            assert np.array_equal(out[pos + 1:pos + 1 + len(rep)], rep), form
            pos += 1 + len(rep)
            if form == 1:  # AddObservation ran once per added point over the whole batch
                assert int(out[pos]) == sum(w[3] for w in fwant)
            assert np.array_equal(out[pos + 1:pos + 1 + len(after)], after), form
            pos += 1 + len(after)
    assert pos == len(out)
