"""rsc_orb::ORBmatcher::Fuse(pKF, vpMapPoints, th) / FuseMany(vpTargetKFs, vpMapPoints, th) (facade/ORBmatcher.hpp)
through the C++ driver tests/cpp/facade_fusekf_test.cpp with mock KeyFrame / MapPoint types, against the map model
of tests/fusekf_ref.py run sequentially (every point matched from the map as it stands when the loop reaches it):
return values, final slots, bad flags, observations and descriptors.

All KeyFrames share the hand geometry of tests/fusekf_cases.py (identity pose, a point (x, 0, 1) projects to
u = 100 x + 300, v = 200); what differs between them is which keypoints they have, the descriptors and the slots."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import fusekf_cases as fc
import fusekf_ref as fr
from rsc import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "orb-slam2-optimized_amd", "lib", "facade_fusekf_test")
ZERO = np.zeros(32, np.uint8)


class Scene:
    """KeyFrames (id = index), MapPoints (id = index) and the initial slots, kept as a recipe so that the model and
    the driver's input are built from the same data."""

    def __init__(self):
        self.kfs, self.pts, self.obs = [], [], []

    def kf(self, kps):
        """kps: [(u, v, descriptor, u_right)]"""
        view = fc.make_kf([k[:2] for k in kps], [0] * len(kps), [k[2] for k in kps], [k[3] for k in kps],
                          fx=fc.FX, fy=fc.FY, cx=fc.CX, cy=fc.CY, max_x=fc.MAX_X)
        self.kfs.append(view)
        return len(self.kfs) - 1

    def point(self, x, desc=ZERO, bad=False, y=0.0):
        self.pts.append(dict(pos=(x, y, 1.0), desc=np.array(desc, np.uint8), bad=bad))
        return len(self.pts) - 1

    def put(self, p, kf, idx):
        self.obs.append((p, kf, idx))

    def model(self):
        kfs = [fr.KeyFrame(i, v) for i, v in enumerate(self.kfs)]
        pts = []
        for i, p in enumerate(self.pts):
            pos = np.array(p["pos"], np.float32)
            m = fr.MapPoint(i, pos, np.array((0.0, 0.0, 10.0), np.float32), np.float32(np.sqrt(np.float32(pos @ pos))),
                            np.float32(0.01), p["desc"])
            m.bad = p["bad"]
            pts.append(m)
        for p, k, idx in self.obs:
            kfs[k].slots[idx] = pts[p]
            if not pts[p].bad:
                pts[p].add_observation(kfs[k], idx)
        return kfs, pts

    def pack(self, mode, th, cur, targets, lst):
        kfs, pts = self.model()
        sf = synth.scale_factors()
        b = [struct.pack("<i", len(sf)), sf.tobytes(), struct.pack("<f", float(synth.LOG_SCALE_FACTOR)),
             struct.pack("<i", len(self.kfs))]
        for i, v in enumerate(self.kfs):
            b.append(struct.pack("<ii4f4i3f", i, v.n, v.fx, v.fy, v.cx, v.cy, int(v.min_x), int(v.max_x), int(v.min_y),
                                 int(v.max_y), float(synth.GRID_W_INV), float(synth.GRID_H_INV), v.mbf))
            for a, dt in ((v.Rcw, np.float32), (v.tcw, np.float32), (v.Rwc, np.float32), (v.Ow, np.float32),
                          (v.kp, np.float32), (v.octave, np.int32), (v.desc, np.uint8), (v.u_right, np.float32),
                          (v.cell_begin, np.int32), (v.cell_feat, np.int32)):
                b.append(np.ascontiguousarray(a, dt).tobytes())
        b.append(struct.pack("<i", len(pts)))
        b.append(np.array([p.bad for p in pts], np.uint8).tobytes())
        for key, dt in (("pos", np.float32), ("normal", np.float32), ("dmax", np.float32), ("dmin", np.float32),
                        ("desc", np.uint8)):
            b.append(np.ascontiguousarray([getattr(p, key) for p in pts], dt).tobytes())
        b.append(struct.pack("<i", len(self.obs)))
        for o in self.obs:
            b.append(struct.pack("<3i", *o))
        b.append(struct.pack("<ifii", mode, th, cur, len(targets)) + struct.pack(f"<{len(targets)}i", *targets))
        b.append(struct.pack("<i", len(lst)) + struct.pack(f"<{len(lst)}i", *[-1 if p is None else p for p in lst]))
        return b"".join(b)

    def run(self, mode, targets, lst=(), cur=0, th=fc.TH):
        """(driver's return values, driver's final map) and (the model's, the model's), after the same calls."""
        with tempfile.TemporaryDirectory() as d:
            a, b = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(a, "wb") as f:
                f.write(self.pack(mode, th, cur, targets, lst))
            subprocess.run([BIN, a, b], check=True, timeout=120)
            out = np.fromfile(b, np.int32).tolist()
        it = iter(out)
        ret = [next(it) for _ in range(next(it))]
        got = dict(slots=[[next(it) for _ in range(v.n)] for v in self.kfs], bad=[], nobs=[], obs=[], desc=[])
        for _ in self.pts:
            got["bad"].append(next(it))
            got["nobs"].append(next(it))
            got["obs"].append([(next(it), next(it)) for _ in range(next(it))])
            got["desc"].append([next(it) for _ in range(32)])
        kfs, pts = self.model()
        mlist = [None if p is None else pts[p] for p in lst]
        if mode == 2:
            fwd, cand, back = fr.search_in_neighbors(kfs[cur], [kfs[k] for k in targets], th)
            want_ret = fwd + [len(cand), back]
        else:
            want_ret = [fr.fuse(kfs[k], mlist, th) for k in targets]
        return ret, got, want_ret, fr.snapshot(kfs, pts), (kfs, pts)


def check(scene, mode, targets, lst=(), cur=0):
    ret, got, want_ret, want, model = scene.run(mode, targets, lst, cur)
    assert ret == want_ret
    for key in ("slots", "bad", "nobs", "obs", "desc"):
        assert got[key] == want[key], key
    return ret, got, model


def elsewhere(s, p, n):
    """n monocular observations of point p in KeyFrames of their own (not targets), on a keypoint far from
    everything with the point's descriptor."""
    for _ in range(n):
        k = s.kf([(600.0, 400.0, s.pts[p]["desc"], -1.0)])
        s.put(p, k, 0)


@pytest.mark.parametrize("b_obs, survivor", [(0, "a"), (1, "b"), (3, "b")])
@pytest.mark.parametrize("mode", [0, 1])
def test_fill_then_claim(b_obs, survivor, mode):
    """Point A fills the empty slot (:811-815) and point B of the same call finds it there (:801-809).  A then has
    one observation: with B at 0 the occupant has more and B->Replace(A); at 1 (the tie) and at 3 the else branch
    runs, A->Replace(B)."""
    s = Scene()
    k = s.kf([(301.0, 200.0, fc.desc_bits(2), -1.0), (302.0, 200.0, fc.desc_bits(30), -1.0)])
    a, b = s.point(0.0), s.point(0.0)
    elsewhere(s, b, b_obs)
    ret, got, _ = check(s, mode, [k], [a, b])
    assert ret == [2]
    win, lose = (a, b) if survivor == "a" else (b, a)
    assert got["slots"][k][0] == win and got["bad"][lose] == 1 and got["bad"][win] == 0
    assert got["nobs"][win] == 1 + b_obs * (survivor == "b")


def test_bad_occupant_counts():
    s = Scene()
    k = s.kf([(301.0, 200.0, fc.desc_bits(2), -1.0)])
    a, z = s.point(0.0), s.point(0.0, bad=True)
    s.put(z, k, 0)
    ret, got, _ = check(s, 0, [k], [a])
    assert ret == [1] and got["slots"][k] == [z] and got["obs"][a] == []


def test_joins_a_later_keyframe_through_replace():
    """A (three observations elsewhere) meets Q in KeyFrame 1; Q has two (KeyFrames 1 and 2), so Q->Replace(A) puts A
    into KeyFrame 2's slot 0.  When the replay reaches KeyFrame 2, A is in it and is skipped (:695), although at
    launch it was not and its bestIdx there is keypoint 1 (the nearer descriptor), an empty slot."""
    s = Scene()
    k1 = s.kf([(301.0, 200.0, fc.desc_bits(2), -1.0)])
    k2 = s.kf([(301.0, 200.0, fc.desc_bits(9), -1.0), (299.0, 200.0, fc.desc_bits(1), -1.0)])
    a, q = s.point(0.0), s.point(0.0, desc=fc.desc_bits(2))
    elsewhere(s, a, 3)
    s.put(q, k1, 0)
    s.put(q, k2, 0)
    kfs, pts = s.model()
    assert int(fr.fuse_kf(kfs[k2].view, fr.points_view([pts[a]]), [0], fc.TH)[0]) == 1  # the launch's answer
    ret, got, _ = check(s, 0, [k1, k2], [a])
    assert ret == [1, 0] and got["slots"][k2] == [a, -1] and got["bad"][q] == 1
    assert (k2, 0) in got["obs"][a] and got["nobs"][a] == 5


def test_a_point_that_turns_bad():
    """A (no observations) meets Q (one) in KeyFrame 1: A->Replace(Q), A is bad from then on and KeyFrame 2, where
    its launch-time bestIdx is an empty slot, must not receive it."""
    s = Scene()
    k1 = s.kf([(301.0, 200.0, fc.desc_bits(2), -1.0)])
    k2 = s.kf([(301.0, 200.0, fc.desc_bits(2), -1.0)])
    a, q = s.point(0.0), s.point(0.0, desc=fc.desc_bits(2))
    s.put(q, k1, 0)
    ret, got, _ = check(s, 0, [k1, k2], [a])
    assert ret == [1, 0] and got["bad"][a] == 1 and got["slots"][k2] == [-1] and got["slots"][k1] == [q]


@pytest.mark.parametrize("mode", [0, 1])
def test_survivor_descriptor_moves_best_idx(mode):
    """A's descriptor is all zeros (two observations elsewhere on all-zero keypoints).  In KeyFrame 1 it meets Q on a
    keypoint with descriptor D (30 bits set); Q has two observations too, both on D keypoints, so the tie runs
    Q->Replace(A) and A takes them over.  A's observations are then D, D, 0, 0 in KeyFrame-id order and
    ComputeDistinctiveDescriptors picks D.  KeyFrame 2 has keypoint 0 at distance 5 from zeros and 35 from D, and
    keypoint 1 at distance 33 from zeros and 3 from D: the launch-time bestIdx is 0, the reference's (and the
    redo's) is 1."""
    D = fc.desc_bits(30, 100)
    near_d = D.copy()
    near_d[0] |= 7  # D plus bits 0..2
    s = Scene()
    k1 = s.kf([(301.0, 200.0, D, -1.0)])
    k2 = s.kf([(301.0, 200.0, fc.desc_bits(5), -1.0), (299.0, 200.0, near_d, -1.0)])
    k3 = s.kf([(600.0, 400.0, D, -1.0)])
    a, q = s.point(0.0), s.point(0.0, desc=D)
    s.put(q, k1, 0)
    s.put(q, k3, 0)
    elsewhere(s, a, 2)  # KeyFrames 3 and 4 by index: after k1 and k3 in id order
    kfs, pts = s.model()
    stale = int(fr.fuse_kf(kfs[k2].view, fr.points_view([pts[a]]), [0], fc.TH)[0])
    ret, got, (mk, mp) = check(s, mode, [k1, k2], [a])
    assert stale == 0 and got["slots"][k2] == [-1, a]  # a facade without the redo fills slot 0
    assert got["desc"][a] == D.tolist() and ret == [1, 1] and got["bad"][q] == 1


def test_null_and_duplicate_entries():
    s = Scene()
    k = s.kf([(301.0, 200.0, fc.desc_bits(2), -1.0), (401.0, 200.0, fc.desc_bits(2), 360.0)])
    a, b = s.point(0.0), s.point(1.0)
    ret, got, _ = check(s, 0, [k], [None, a, a, None, b, None])
    assert ret == [2] and got["slots"][k] == [a, b] and got["nobs"] == [1, 2]  # keypoint 1 is stereo: +2
    ret, got, _ = check(s, 0, [k, k], [])
    assert ret == [0, 0]
    ret, got, _ = check(s, 0, [], [a])
    assert ret == []


def test_search_in_neighbors_sequence():
    """LocalMapping.cpp:458-490 on four target KeyFrames: the current KeyFrame's slots (nulls included) forward in one
    FuseMany, then the targets' points backward into the current KeyFrame.  Six locations 50 px apart; every
    KeyFrame has a keypoint near each (descriptor: the location's base with a few bits flipped, 30 % stereo with a
    consistent right coordinate), the current KeyFrame holds a point on four of them, the targets hold points of
    their own with one to three observations elsewhere on some, and nothing on others."""
    rng = np.random.default_rng(5)
    s = Scene()
    xs = [-1.0, -0.5, 0.0, 0.5, 1.0, 1.5]
    base = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in xs]

    def flip(d, n):
        d = d.copy()
        for bit in rng.choice(256, n, replace=False):
            d[bit // 8] ^= 1 << (bit % 8)
        return d

    def keyframe():
        kps = []
        for x, d in zip(xs, base):
            u = 100.0 * x + 300.0 + float(rng.uniform(-1.2, 1.2))
            kps.append((u, 200.0 + float(rng.uniform(-1.2, 1.2)), flip(d, int(rng.integers(0, 12))),
                        u - fc.MBF + float(rng.uniform(-0.5, 0.5)) if rng.random() < 0.3 else -1.0))
        return s.kf(kps)

    cur = keyframe()
    targets = [keyframe() for _ in range(4)]
    for j in (0, 1, 3, 4):  # the current KeyFrame's own points; slots 2 and 5 stay null
        p = s.point(xs[j], desc=flip(base[j], 3))
        s.put(p, cur, j)
        elsewhere(s, p, int(rng.integers(0, 3)))
    for k in targets:
        for j in range(len(xs)):
            if rng.random() < 0.5:
                q = s.point(xs[j], desc=flip(base[j], 3), bad=bool(rng.random() < 0.15))
                s.put(q, k, j)
                if not s.pts[q]["bad"]:
                    elsewhere(s, q, int(rng.integers(0, 4)))
    ret, got, _ = check(s, 2, targets, cur=cur)
    assert sum(ret[:4]) >= 8 and ret[4] >= 4 and ret[5] >= 2  # forward matches, backward candidates and matches
    assert sum(got["bad"]) > sum(p["bad"] for p in s.pts)     # some Replace ran
