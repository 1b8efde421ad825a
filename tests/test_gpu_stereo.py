"""Frame::ComputeStereoMatches on the device (stereo.hip, rsc_compute_stereo_matches_many) against the answers
worked out by hand (tests/stereo_cases.py), the golden fixture of the sequential restatement
(tests/golden/stereo_traces.npz) and the restatement itself, bit for bit: all hand-built cases in one call, all
random frames in one call (sizes mixed, empties included), with and without set_stereo and the diagnostics; every
refusal with the outputs' fill bytes kept; and the write-through of mvuRight into the resident view."""
import os

import numpy as np
import pytest

import localproj_cases as lc
import stereo_cases as sc
import stereo_ref as sr
from gpu_common import ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("u_right", "depth", "best_right", "best_dist")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "stereo_traces.npz"))


@pytest.fixture(scope="module")
def randoms():
    """name -> (frame, the restatement's result), computed once."""
    return {name: (fr, sr.compute(fr)) for name, fr in sc.random_frames().items()}


def from_golden(golden, name):
    r = {k: golden[f"{name}/{k}"] for k in ARRAYS}
    rec = golden[f"{name}/result"]
    r.update(n_candidates=int(rec[0]), n_removed=int(rec[1]), median=int(rec[2]), th_dist=np.float32(rec[3]))
    return r


def view(fr, c=None):
    """The resident left Frame of a stereo_ref frame (the grid and the angles are not read by the stereo call)."""
    from rsc import engine, synth
    assert np.array_equal(fr.scale, synth.scale_factors())
    pf = synth.make_proj_frame(fr.kp, fr.octave, np.zeros(len(fr.kp), np.float32), fr.desc)
    return engine.FrameView(c or ctx(), pf)


def run(frames, **kw):
    from rsc import engine
    views = [view(fr) for fr in frames]
    r = engine.compute_stereo_matches_many(ctx(), views, frames, [fr.mbf for fr in frames], [fr.mb for fr in frames],
                                           **kw)
    return views, r


def test_hand_built_cases_one_call(golden):
    cases = sc.cases()
    _, res = run([fr for _, fr, _ in cases])
    for (name, fr, exp), r in zip(cases, res):
        assert sr.same(r, exp) == [], (name, r, exp)
        assert sr.same(r, from_golden(golden, name)) == [], name


@pytest.mark.parametrize("set_stereo", [False, True])
def test_random_frames_one_call(golden, randoms, set_stereo):
    """Sizes 1 to 1,200 on the left and 63 to 4,097 on the right in one batch, with two empties in the middle."""
    names = list(randoms)
    frames = [randoms[n][0] for n in names]
    empties = {name: (fr, exp) for name, fr, exp in sc.cases() if name in ("empty_left", "empty_right")}
    frames[3:3] = [empties["empty_left"][0], empties["empty_right"][0]]
    names[3:3] = ["empty_left", "empty_right"]
    _, res = run(frames, set_stereo=set_stereo)
    for name, r in zip(names, res):
        want = empties[name][1] if name in empties else randoms[name][1]
        assert sr.same(r, want) == [], name
        assert sr.same(r, from_golden(golden, name)) == [], name


def test_null_diagnostics(randoms):
    from rsc import engine
    frames = [randoms[n][0] for n in ("r_65x257", "r_200x2049")]
    views, res = run(frames, diagnostics=False)
    for fr, r in zip(frames, res):
        want = sr.compute(fr)
        assert r["best_right"] is None and r["best_dist"] is None
        assert np.array_equal(r["u_right"].view(np.uint32), want["u_right"].view(np.uint32))
        assert np.array_equal(r["depth"].view(np.uint32), want["depth"].view(np.uint32))
        assert (r["n_candidates"], r["n_removed"], r["median"]) == (want["n_candidates"], want["n_removed"], want["median"])
    # NULL entries inside a diagnostics array: one frame with, one without
    F = engine.STEREO_FILL
    out = [dict(u_right=np.full(len(fr.kp), F["u_right"], np.float32), depth=np.full(len(fr.kp), F["depth"], np.float32),
                best_right=None, best_dist=None) for fr in frames]
    out[1]["best_right"] = np.full(len(frames[1].kp), F["best_right"], np.int32)
    res = engine.compute_stereo_matches_many(ctx(), views, frames, [fr.mbf for fr in frames], [fr.mb for fr in frames],
                                             False, True, out)
    want = sr.compute(frames[1])
    assert np.array_equal(res[1]["best_right"], want["best_right"]) and res[1]["best_dist"] is None
    assert np.array_equal(res[0]["u_right"].view(np.uint32), sr.compute(frames[0])["u_right"].view(np.uint32))


def test_count_zero():
    from rsc import engine
    assert engine.compute_stereo_matches_many(ctx(), [], [], [], []) == []


def test_argument_errors(randoms):
    """Every refusal comes before any launch: the outputs keep their fill, and the call works afterwards."""
    import copy

    from rsc import engine
    fr = randoms["r_63x64"][0]
    v = view(fr)
    F = engine.STEREO_FILL

    def refused(views, frames, mbf, mb, set_stereo=False, c=None):
        out = [dict(u_right=np.full(max(x.n, 1), F["u_right"], np.float32), depth=np.full(max(x.n, 1), F["depth"], np.float32),
                    best_right=np.full(max(x.n, 1), F["best_right"], np.int32),
                    best_dist=np.full(max(x.n, 1), F["best_dist"], np.int32)) for x in views]
        with pytest.raises(RuntimeError):
            engine.compute_stereo_matches_many(c or ctx(), views, frames, mbf, mb, set_stereo, True, out)
        for o in out:
            for k in ARRAYS:
                assert (o[k] == F[k]).all(), k

    # one right keypoint too many
    big = copy.copy(fr)
    m = engine.STEREO_MAX_RIGHT + 1
    big.r_kp, big.r_octave, big.r_desc = np.zeros((m, 2), np.float32), np.zeros(m, np.int32), np.zeros((m, 32), np.uint8)
    refused([v], [big], [fr.mbf], [fr.mb])
    # mbf / mb: zero, negative, infinite, NaN
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused([v], [fr], [bad], [fr.mb])
        refused([v], [fr], [fr.mbf], [bad])
    # a non-finite right keypoint coordinate, either one
    for col, bad in ((0, np.nan), (1, np.inf), (1, np.nan)):
        nf = copy.copy(fr)
        nf.r_kp = fr.r_kp.copy()
        nf.r_kp[5, col] = bad
        refused([v], [nf], [fr.mbf], [fr.mb])
    # the same view twice with set_stereo (without it the two entries are independent and legal), also in a later slot
    other = view(randoms["r_64x65"][0])
    refused([v, other, v], [fr, randoms["r_64x65"][0], fr], [fr.mbf] * 3, [fr.mb] * 3, set_stereo=True)
    twice = engine.compute_stereo_matches_many(ctx(), [v, v], [fr, fr], [fr.mbf] * 2, [fr.mb] * 2, False)
    assert sr.same(twice[0], randoms["r_63x64"][1]) == [] and sr.same(twice[1], randoms["r_63x64"][1]) == []
    # a view of another context, called on this one and on its own with a foreign neighbour
    c2 = engine.Context(0)
    foreign = view(fr, c2)
    refused([foreign], [fr], [fr.mbf], [fr.mb])
    refused([foreign, v], [fr, fr], [fr.mbf] * 2, [fr.mb] * 2, c=c2)
    foreign.close()
    c2.close()
    # a left octave outside [0, n_levels) cannot reach the call: the view itself is refused
    from rsc import synth
    for bad in (-1, 8):
        octv = fr.octave.copy()
        octv[7] = bad
        with pytest.raises(RuntimeError):
            engine.FrameView(ctx(), synth.make_proj_frame(fr.kp, octv, np.zeros(len(fr.kp), np.float32), fr.desc))
    # right octaves are only compared: any int32 is legal
    wide = copy.copy(fr)
    wide.r_octave = fr.r_octave.copy()
    wide.r_octave[::7] = np.iinfo(np.int32).min
    wide.r_octave[3::7] = np.iinfo(np.int32).max
    r = engine.compute_stereo_matches_many(ctx(), [v], [wide], [fr.mbf], [fr.mb], False)[0]
    assert sr.same(r, sr.compute(wide)) == []
    # and the call still works afterwards
    r = v.compute_stereo(fr, fr.mbf, fr.mb, set_stereo=False)
    assert sr.same(r, randoms["r_63x64"][1]) == []


def test_set_stereo_writes_through():
    """After set_stereo = 1 the local-map matcher reads the view as after rsc_frameview_set_stereo with the same
    mvuRight; a view that got neither is refused."""
    from rsc import engine, synth
    p = lc.random_problem(22, 1.0, n_frame=300, n_points=600)
    f = p.frame
    rng = np.random.default_rng(5)
    n = f.n
    r_kp = f.kp.copy()
    r_kp[:, 0] = np.maximum(f.kp[:, 0] - rng.uniform(1.0, 60.0, n).astype(np.float32), 0.0)
    r_desc = f.desc.copy()
    r_desc[:, 0] ^= rng.integers(0, 256, n, dtype=np.uint8)  # up to 8 flipped bits
    r_desc[::3, 1] ^= 0xFF                                     # 8 more on every third: the cut has something to remove
    order = rng.permutation(n)
    fr = sr.frame(f.kp, f.octave, f.desc, synth.scale_factors(), r_kp[order], f.octave[order], r_desc[order], f.mbf,
                  f.mbf / 100.0)
    want = sr.compute(fr)
    assert want["n_candidates"] > 200 and 0 < want["n_removed"] < want["n_candidates"]
    direct, twin, bare, unset = (engine.FrameView(ctx(), f) for _ in range(4))
    got = direct.compute_stereo(fr, fr.mbf, fr.mb, set_stereo=True)
    assert sr.same(got, want) == []
    twin.set_stereo(got["u_right"], f.mbf)
    assert sr.same(unset.compute_stereo(fr, fr.mbf, fr.mb, set_stereo=False), want) == []
    mv = engine.MPView(ctx(), p.pts)
    args = ([p.Tcw], [p.skip], [p.has_obs], [p.frame_occ], p.cos_limit, p.th, p.nn_ratio)
    a = engine.search_local_points_many(ctx(), [direct], [mv], *args)
    b = engine.search_local_points_many(ctx(), [twin], [mv], *args)
    assert int(a["nmatches"][0]) == int(b["nmatches"][0]) and int(a["nmatches"][0]) > 20
    assert np.array_equal(a["out"][0], b["out"][0])
    assert np.asarray(a["track"][0]).tobytes() == np.asarray(b["track"][0]).tobytes()
    assert int(a["n_to_match"][0]) == int(b["n_to_match"][0]) and int(a["rounds"][0]) == int(b["rounds"][0])
    for v in (bare, unset):
        with pytest.raises(RuntimeError):
            engine.search_local_points_many(ctx(), [v], [mv], *args)


def test_kernel_timing_slots(randoms):
    from rsc import engine
    c = ctx()
    c.enable_timing(True)
    try:
        fr = randoms["r_200x2048"][0]
        view(fr).compute_stereo(fr, fr.mbf, fr.mb, set_stereo=False)
        t = c.last_timing()
    finally:
        c.enable_timing(False)
    assert t["solve_ms"] > 0 and t["scan_ms"] > 0 and t["refine_ms"] >= max(t["solve_ms"], t["scan_ms"])
