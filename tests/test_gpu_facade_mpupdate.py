"""rsc_orb::UpdateMapPoints(vpMapPoints, what) / UpdateMapPointsOf(pKF) (facade/MapPoint.hpp) through the C++ driver
tests/cpp/facade_mpupdate_test.cpp.  Its mock MapPoint keeps a std::map<std::shared_ptr<KeyFrame>, size_t> and has
the reference's two functions restated sequentially; the driver runs them on a copy of the MapPoints (same KeyFrame
pointers, so the same iteration order) and the facade on the originals, and reports how many points differ in
descriptor, normal or distances.  What does not depend on the pointer order (the distances, the descriptor of a
point whose kept descriptors are all equal, untouched points) is checked here as well against
tests/mpupdate_ref.py."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import fusekf_cases as fc
import fusekf_ref as fr
import mpupdate_ref as mr
from rsc import synth
from test_gpu_facade_fusekf import Scene as FuseScene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "orb-slam2-optimized_amd", "lib", "facade_mpupdate_test")
f32 = np.float32
INIT_NORMAL, INIT_DMIN = (0.0, 0.0, 10.0), 0.01  # as the map model of tests/fusekf_ref.py starts its points


class Scene(FuseScene):
    """KeyFrames (fusekf_cases.make_kf views), MapPoints and observations as in the Fuse facade test, plus bad
    KeyFrames and a reference KeyFrame per point (default: its first observation's)."""

    def __init__(self):
        super().__init__()
        self.kf_bad, self.ref = set(), {}

    def kf_at(self, kps, Ow=(0.0, 0.0, 0.0), octaves=None):
        view = fc.make_kf([k[:2] for k in kps], [0] * len(kps) if octaves is None else octaves, [k[2] for k in kps],
                          [k[3] for k in kps], Ow=Ow, fx=fc.FX, fy=fc.FY, cx=fc.CX, cy=fc.CY, max_x=fc.MAX_X)
        self.kfs.append(view)
        return len(self.kfs) - 1

    def pack(self, mode, what, th, cur, targets, lst):
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
        b.append(np.array([k in self.kf_bad for k in range(len(self.kfs))], np.uint8).tobytes())
        n = len(self.pts)
        b.append(struct.pack("<i", n))
        b.append(np.array([p["bad"] for p in self.pts], np.uint8).tobytes())
        b.append(np.array([p["pos"] for p in self.pts], f32).tobytes())
        b.append(np.array([INIT_NORMAL] * n, f32).tobytes())
        b.append(np.array([init_dmax(p) for p in self.pts], f32).tobytes())
        b.append(np.full(n, INIT_DMIN, f32).tobytes())
        b.append(np.array([p["desc"] for p in self.pts], np.uint8).tobytes())
        first = {}
        for p, k, _ in self.obs:
            first.setdefault(p, k)
        b.append(np.array([self.ref.get(p, first.get(p, -1)) for p in range(n)], np.int32).tobytes())
        b.append(struct.pack("<i", len(self.obs)))
        for o in self.obs:
            b.append(struct.pack("<3i", *o))
        b.append(struct.pack("<iifii", mode, what, th, cur, len(targets)) + struct.pack(f"<{len(targets)}i", *targets))
        b.append(struct.pack("<i", len(lst)) + struct.pack(f"<{len(lst)}i", *[-1 if p is None else p for p in lst]))
        return b"".join(b)

    def run(self, lst=(), what=3, mode=0, cur=0, targets=(), th=fc.TH):
        with tempfile.TemporaryDirectory() as d:
            a, b = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(a, "wb") as f:
                f.write(self.pack(mode, what, th, cur, list(targets), list(lst)))
            subprocess.run([BIN, a, b], check=True, timeout=120)
            out = np.fromfile(b, np.int32)
        head, body = out[:3].tolist(), out[3:].reshape(len(self.pts), 39)
        pts = [dict(bad=int(r[0]), nobs=int(r[1]), desc=r[2:34].astype(np.uint8),
                    normal=r[34:37].copy().view(f32), dmax=r[37:38].copy().view(f32)[0],
                    dmin=r[38:39].copy().view(f32)[0]) for r in body]
        return dict(mismatches=head[0], updated=head[1], fused=head[2], pts=pts)


def init_dmax(p):
    pos = np.array(p["pos"], f32)
    return f32(np.sqrt(f32(pos @ pos)))


def untouched(p, init, what=3):
    ok = True
    if what & 1:
        ok = ok and np.array_equal(p["desc"], init["desc"])
    if what & 2:
        ok = ok and p["normal"].tolist() == list(INIT_NORMAL) and p["dmax"] == init_dmax(init) and p["dmin"] == f32(INIT_DMIN)
    return ok


@pytest.fixture(scope="module")
def scene():
    """Five KeyFrames with camera centres of their own (KeyFrame 3 is bad), eight points:
    0  five observations, the reference KeyFrame among them
    1  its reference KeyFrame (4) is not among its observations: index 0 of that KeyFrame is read (octave 6)
    2  a bad point (it sits in a slot, unobserved)
    3  observed by the bad KeyFrame only: no descriptor, the normal and depth are written
    4  no observations
    5  two observations with one descriptor
    6  three observations, one of them in the bad KeyFrame
    7  one observation"""
    rng = np.random.default_rng(12)
    s = Scene()
    base = rng.integers(0, 256, 32, dtype=np.uint8)

    def flip(n):
        d = base.copy()
        for bit in rng.choice(256, n, replace=False):
            d[bit // 8] ^= 1 << (bit % 8)
        return d

    same = flip(9)
    for k in range(5):
        kps = [(100.0 + 40 * j, 100.0 + 30 * j, same if j == 5 else flip(int(rng.integers(0, 25))), -1.0)
               for j in range(8)]
        s.kf_at(kps, Ow=rng.uniform(-2, 2, 3), octaves=[6, 1, 2, 3, 4, 5, 0, 7])
    s.kf_bad = {3}
    for i in range(8):
        s.point(float(rng.uniform(-1, 1)), desc=flip(60), bad=(i == 2), y=float(rng.uniform(-1, 1)))
        s.pts[-1]["pos"] = (s.pts[-1]["pos"][0], s.pts[-1]["pos"][1], 6.0)
    for k in (4, 0, 2, 1, 3):
        s.put(0, k, 0 if k != 2 else 3)
    s.ref[0] = 2
    for k in (1, 0, 2):
        s.put(1, k, 1)
    s.ref[1] = 4
    s.put(2, 0, 2)
    s.put(3, 3, 4)
    s.put(5, 0, 5)
    s.put(5, 1, 5)
    for k in (0, 3, 4):
        s.put(6, k, 6)
    s.put(7, 2, 7)
    return s


def depth_of(s, p, ref_kf, ref_idx):
    """mfMaxDistance, mfMinDistance of the restatement: they do not depend on the list order."""
    sf = synth.scale_factors()
    pos = np.array(s.pts[p]["pos"], f32)
    _, dmax, dmin = mr.normal_and_depth(pos, [s.kfs[ref_kf].Ow], s.kfs[ref_kf].Ow, sf[int(s.kfs[ref_kf].octave[ref_idx])],
                                        sf[len(sf) - 1])
    return dmax, dmin


@pytest.mark.parametrize("what", [3, 1, 2])
def test_update_map_points(scene, what):
    s = scene
    lst = [0, None, 1, 2, 0, 3, 4, None, 5, 6, 7, 5]  # nulls and repeated pointers
    r = s.run(lst, what)
    assert r["mismatches"] == 0
    assert r["updated"] == (6 if what & 2 else 5)  # points 0, 1, 5, 6, 7, and 3 through its normal only
    p = r["pts"]
    init = s.pts
    assert untouched(p[2], init[2]) and untouched(p[4], init[4])  # the bad point, the point without observations
    assert np.array_equal(p[3]["desc"], init[3]["desc"])          # every KeyFrame bad: no descriptor
    if what & 1:
        for i in (0, 1, 5, 6, 7):
            assert not np.array_equal(p[i]["desc"], init[i]["desc"]), i
        assert np.array_equal(p[5]["desc"], s.kfs[0].desc[5])     # both observations carry this descriptor
        assert np.array_equal(p[7]["desc"], s.kfs[2].desc[7])
        kept6 = [s.kfs[0].desc[6].tolist(), s.kfs[4].desc[6].tolist()]
        assert p[6]["desc"].tolist() in kept6                     # N = 2 of the good KeyFrames: never the bad one's
    else:
        assert all(untouched(p[i], init[i], 1) for i in range(8))
    if what & 2:
        for i, (rk, ri) in {0: (2, 3), 1: (4, 0), 3: (3, 4), 5: (0, 5), 6: (0, 6), 7: (2, 7)}.items():
            dmax, dmin = depth_of(s, i, rk, ri)
            assert mr.same_floats([p[i]["dmax"], p[i]["dmin"]], [dmax, dmin]), i
            assert p[i]["normal"].tolist() != list(INIT_NORMAL) and abs(np.linalg.norm(p[i]["normal"]) - 1) < 0.2
        # one observation: the normal does not depend on any order
        n7, _, _ = mr.normal_and_depth(np.array(s.pts[7]["pos"], f32), [s.kfs[2].Ow], s.kfs[2].Ow, 1.0, 1.0)
        assert mr.same_floats(p[7]["normal"], n7)
    else:
        assert all(untouched(p[i], init[i], 2) for i in range(8))


def test_empty_and_null_lists(scene):
    assert scene.run([], 3)["updated"] == 0
    assert scene.run([None, None], 3)["updated"] == 0
    r = scene.run([2, 4], 3)  # nothing to update: no launch
    assert r["updated"] == 0 and r["mismatches"] == 0


def chain_scene():
    """The scene of the Fuse facade's SearchInNeighbors test (six locations 50 px apart, a current KeyFrame with
    points on four of them, four targets with points of their own and observations elsewhere)."""
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
            kps.append((u, 200.0 + float(rng.uniform(-1.2, 1.2)), flip(d, int(rng.integers(0, 12))), -1.0))
        return s.kf(kps)

    def elsewhere(p, n):
        for _ in range(n):
            k = s.kf([(600.0, 400.0, flip(s.pts[p]["desc"], 4), -1.0)])
            s.put(p, k, 0)

    cur = keyframe()
    targets = [keyframe() for _ in range(4)]
    for j in (0, 1, 3, 4):
        p = s.point(xs[j], desc=flip(base[j], 3))
        s.put(p, cur, j)
        elsewhere(p, int(rng.integers(0, 3)))
    for k in targets:
        for j in range(len(xs)):
            if rng.random() < 0.5:
                q = s.point(xs[j], desc=flip(base[j], 3), bad=bool(rng.random() < 0.15))
                s.put(q, k, j)
                if not s.pts[q]["bad"]:
                    elsewhere(q, int(rng.integers(0, 4)))
    return s, cur, targets


def test_fuse_then_update_of_current_keyframe():
    """LocalMapping.cpp:458-506: FuseMany over the targets, the backward Fuse, then the update loop over the current
    KeyFrame's points, compared in the driver with the sequential loop on a copy of the map.  The map model of
    tests/fusekf_ref.py says how many pairs fuse and which points the current KeyFrame holds afterwards."""
    s, cur, targets = chain_scene()
    kfs, pts = s.model()
    fwd, cand, back = fr.search_in_neighbors(kfs[cur], [kfs[k] for k in targets], fc.TH)
    held = {m.id for m in kfs[cur].slots if m is not None and not m.bad}
    assert sum(fwd) + back >= 6 and len(held) >= 4
    r = s.run(mode=2, cur=cur, targets=targets)
    assert r["mismatches"] == 0
    assert r["fused"] == sum(fwd) + back and r["updated"] == len(held)
    for i, p in enumerate(r["pts"]):
        assert (p["normal"].tolist() != list(INIT_NORMAL)) == (i in held), i
        assert p["bad"] == int(pts[i].bad) and p["nobs"] == len(pts[i].obs)
    assert any(r["pts"][i]["nobs"] >= 3 for i in held)  # points that gained observations and were then updated
