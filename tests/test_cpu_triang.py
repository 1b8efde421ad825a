"""SearchForTriangulation, the pair geometry and the CreateNewMapPoints loop off the device: the sequential
restatement (tests/triang_ref.py) gives every hand-worked answer; the host emulation of rsc_triang.h
(tests/triang_emu: the literal loop and the kernels' item / reduction order) equals it bit for bit on every case and
on the fixture; every rule switch changes a named case; the speculative replay equals the literal neighbour loop;
the float 4x4 Jacobi SVD is pinned against a float64 numpy.linalg.svd."""
import os

import numpy as np
import pytest

import triang_cases as tc
import triang_emu_lib as el
import triang_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "triang_traces.npz")
# Largest relative deviation |x3D - x3D_64| / |x3D_64| of the float Jacobi restatement from a float64
# numpy.linalg.svd of the same float32 A, measured on this project's CPU build over the inputs of
# test_svd_against_float64 (noise-free two-view points and the fixture's SVD pairs, all with cosParallaxRays <
# 0.9998): 3.632e-06.  Allowed: four times that, since float Jacobi's error varies with conditioning across inputs.
SVD_MEASURED = 3.632e-06
SVD_ALLOWED = 4 * SVD_MEASURED


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def problems():
    return tc.fixture_problems()


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_matcher_hand_worked_answers():
    for n, (k1, k2, F, os_, co, exp, nm, dz, _) in tc.matcher_cases().items():
        r = tr.search_for_triangulation(k1, k2, F, os_, co)
        assert r["matches12"].tolist() == exp and r["nmatches"] == nm and r["den_zero"] == dz, n
    k1, k2, exp = tc.winner_positions()
    assert tr.search_for_triangulation(k1, k2, tc.F_HORIZ)["matches12"].tolist() == exp
    # den == 0: the flag sits on the planted slot, whichever eligible slot is met first
    k1, k2, F = tc.matcher_cases()["den_zero"][:3]
    assert tr.search_for_triangulation(k1, k2, F)["den_zero_slot"].tolist() == [0, 1]
    # a NaN epipole (C2z = 0 -> 0 * inf) skips nobody
    k1, k2, F = tc.matcher_cases()["epipole_edge"][:3]
    k2.tcw[:] = 0
    ex, ey = tr.epipole(k1, k2)
    assert np.isnan(ex) and np.isnan(ey)
    assert tr.search_for_triangulation(k1, k2, F)["matches12"].tolist() == [0, 1]


def test_pair_hand_worked_answers():
    for n, (k1, k2, i1, i2, status, branch, _) in tc.pair_cases().items():
        s, x, t = tr.triangulate_pair(k1, k2, i1, i2)
        assert s == status and t["branch"] == branch, (n, s, t["branch"])
    s, x, _ = tr.triangulate_pair(*tc.pair_cases()["ok_mono"][:4])
    assert np.allclose(x, [0.25, 0.1, 4.0], atol=1e-4)
    assert sorted({c[4] for c in tc.pair_cases().values()}) == list(range(9))  # every status code has its case


def test_driver_hand_worked_answers():
    for n, (cur, neigh, exp) in tc.driver_cases().items():
        r = tr.create_new_map_points(cur, neigh)
        for slot, want in enumerate(exp):
            assert want is None or int(r["new_neighbour"][slot]) == want, (n, slot, r["new_neighbour"])
        assert r["order"] == sorted(r["order"])  # creation order: (neighbour, idx1) ascending
    cs = tc.driver_cases()
    # the builder's claim: the forward neighbour's matcher takes the den == 0 branch on slot 0 ...
    cur, neigh, _ = cs["den_zero_voids"]
    r = tr.search_for_triangulation(cur, neigh[0], tr.compute_f12(cur, neigh[0]))
    assert r["den_zero"] == 1 and r["den_zero_slot"][0] == 1
    assert tr.create_new_map_points(cur, neigh)["voided"] == [0]
    # ... and is not voided once neighbour 0 has filled that slot, although from the initial slots it would be
    cur, neigh, _ = cs["den_zero_filled"]
    assert tr.search_for_triangulation(cur, neigh[1], tr.compute_f12(cur, neigh[1]))["den_zero"] == 1
    r = tr.create_new_map_points(cur, neigh)
    assert r["voided"] == [] and (r["new_neighbour"] == 1).any()
    assert tr.baseline_short(*[cs["short_baseline"][0], cs["short_baseline"][1][0]])


def test_fixture_is_current(golden, problems):
    """The seeded problems still give the committed golden outputs (so the device tests compare like with like)."""
    assert [str(s) for s in golden["names"]] == list(problems)
    for n, (k1, k2, F, os_, co) in problems.items():
        r = tr.search_for_triangulation(k1, k2, F, os_, co, all_den_zero=True)
        assert np.array_equal(r["matches12"], golden[f"{n}/matches12"]), n
        assert [r["nmatches"], r["den_zero"]] == golden[f"{n}/counts"].tolist(), n
    sizes = set()
    for n in problems:
        k2 = problems[n][1]
        sizes |= set(np.diff(k2.node_begin).tolist())
    assert {1, 2, 63, 64, 65, 255, 256, 257, 700} <= sizes


def test_emulation_equals_restatement(golden, problems):
    """Both forms of the emulation against the restatement on every case and the fixture, bit for bit; the
    stand-alone program (plain and sanitized) over the same problems."""
    cases = []
    for n, (k1, k2, F, os_, co) in problems.items():
        pairs = golden[f"{n}/pairs"]
        for ko in (False, True):
            e = el.search(k1, k2, F, os_, co, kernel_order=ko)
            assert np.array_equal(e["matches12"], golden[f"{n}/matches12"]), (n, ko)
            assert [e["nmatches"], e["den_zero"]] == golden[f"{n}/counts"].tolist(), (n, ko)
        assert np.array_equal(el.search(k1, k2, F, os_, co, kernel_order=True)["den_zero_slot"],
                              golden[f"{n}/den_zero_slot"]), n
        st, x = el.triangulate(k1, k2, pairs)
        assert np.array_equal(st, golden[f"{n}/status"]) and bits_equal(x, golden[f"{n}/x3d"]), n
        cases.append((k1, k2, F, os_, co, pairs))
    for n, (k1, k2, i1, i2, *_r) in tc.pair_cases().items():
        st, x = el.triangulate(k1, k2, [[i1, i2]])
        assert int(st[0]) == int(golden[f"pair/{n}/status"]) and bits_equal(x[0], golden[f"pair/{n}/x3d"]), n
        cases.append((k1, k2, tc.F_HORIZ, 0, 0, [[i1, i2]]))
    for n, (cur, neigh, _) in tc.driver_cases().items():
        e = el.create_new_map_points(cur, neigh)
        assert np.array_equal(e["new_neighbour"], golden[f"driver/{n}/new_neighbour"]), n
        assert np.array_equal(e["new_idx2"], golden[f"driver/{n}/new_idx2"]), n
        assert bits_equal(e["new_pos"], golden[f"driver/{n}/new_pos"]) and e["nnew"] == int(golden[f"driver/{n}/nnew"])
        for k in neigh:
            assert bits_equal(el.compute_f12(cur, k), tr.compute_f12(cur, k)), n
    for sanitized in (False, True):
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            res = el.run_main(cases, os.path.join(d, "cases.bin"), os.path.join(d, "out.bin"), sanitized)
        for (k1, k2, F, os_, co, pairs), (seq, ko, st, x) in zip(cases, res):
            ref = tr.search_for_triangulation(k1, k2, F, os_, co)
            for e in (seq, ko):
                assert np.array_equal(e["matches12"], ref["matches12"]) and e["nmatches"] == ref["nmatches"]
            rr = [tr.triangulate_pair(k1, k2, a, b)[:2] for a, b in np.asarray(pairs).reshape(-1, 2)]
            assert st.tolist() == [s for s, _ in rr] and bits_equal(x, np.array([v for _, v in rr]).reshape(-1, 3))


def test_every_rule_switch_changes_a_named_case():
    seen = set()
    for n, c in tc.matcher_cases().items():
        k1, k2, F, os_, co = c[:5]
        base = tr.search_for_triangulation(k1, k2, F, os_, co)
        for rule in c[8]:
            off = tr.search_for_triangulation(k1, k2, F, os_, co, rules=(rule,))
            assert (not np.array_equal(off["matches12"], base["matches12"])) or off["den_zero"] != base["den_zero"], \
                (n, rule)
            seen.add(rule)
    for n, c in tc.pair_cases().items():
        k1, k2, i1, i2 = c[:4]
        s, x, _ = tr.triangulate_pair(k1, k2, i1, i2)
        for rule in c[6]:
            s2, x2, _ = tr.triangulate_pair(k1, k2, i1, i2, rules=(rule,))
            assert s2 != s or not bits_equal(x, x2), (n, rule)
            seen.add(rule)
    # the third term of the stereo reprojection error: a right-image error of 9 > 7.8 with it, 0 without it
    k1, k2, i1, i2 = tc.pair_cases()["mbf_current"][:4]
    k2.u_right[0] += 3.0
    assert tr.triangulate_pair(k1, k2, i1, i2)[0] == tr.REPROJ2
    assert tr.triangulate_pair(k1, k2, i1, i2, rules=("stereo_reproj_third_term",))[0] == tr.OK
    seen.add("stereo_reproj_third_term")
    assert set(tr.RULES) - seen == {"parallax_double"}, set(tr.RULES) - seen
    # `cosParallaxRays < 0.9998` in float instead of double (:293) cannot change any answer, whatever the inputs:
    # float(0.9998) is the smallest float that is not below 0.9998, so for every float c, c < float(0.9998) holds
    # exactly when c < 0.9998 does
    c = np.float32(0.9998)
    below = np.nextafter(c, np.float32(0))
    assert float(c) >= 0.9998 > float(below)
    for v in (below, c, np.nextafter(c, np.float32(2))):
        assert bool(v < c) == (float(v) < 0.9998)


def test_speculative_replay_equals_literal_loop():
    rng = np.random.default_rng(41)
    sets = [c[:2] for c in tc.driver_cases().values()]
    for nn in (1, 4, 10):
        poses = [(tc.I3, (0, 0, 0))] + [(tc.I3, (rng.uniform(-0.8, 0.8), rng.uniform(-0.2, 0.2), rng.uniform(-0.5, 0.5)))
                                        for _ in range(nn)]
        kfs, _ = tc.scene(rng, poses, 40, mp_frac=0.3, node_groups=5, stereo_frac=0.3, noise=0.4, flips=20)
        sets.append((kfs[0], kfs[1:]))
    for cur, neigh in sets:
        a, b = tr.create_new_map_points(cur, neigh), tr.create_new_map_points_speculative(cur, neigh)
        assert np.array_equal(a["new_neighbour"], b["new_neighbour"]) and np.array_equal(a["new_idx2"], b["new_idx2"])
        assert bits_equal(a["new_pos"], b["new_pos"]) and a["nnew"] == b["nnew"] and a["order"] == b["order"]


def svd_inputs(golden, problems):
    """Triangulation matrices with cosParallaxRays < 0.9998: noise-free two-view points, and the fixture's pairs that
    took the SVD branch."""
    rng = np.random.default_rng(51)
    out = []
    for _ in range(200):
        t2 = (rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.5))
        X = [rng.uniform(-1.5, 1.5), rng.uniform(-1, 1), rng.uniform(2, 10)]
        k1, k2 = tc._two_views(X, t2=t2)
        s, x, t = tr.triangulate_pair(k1, k2, 0, 0)
        if t["branch"] == "svd" and float(t["cos_rays"]) < 0.9998:
            out.append(t["A"])
    for n, (k1, k2, *_r) in problems.items():
        for a, b in golden[f"{n}/pairs"][:40]:
            t = tr.triangulate_pair(k1, k2, int(a), int(b))[2]
            if t["branch"] == "svd" and float(t["cos_rays"]) < 0.9998:
                out.append(t["A"])
    return out


def test_svd_against_float64(golden, problems):
    As = svd_inputs(golden, problems)
    assert len(As) >= 200
    worst = 0.0
    for A in As:
        v = tr.svd_last_v(A).astype(np.float64)
        assert bits_equal(el.svd_last_v(A), v.astype(np.float32))
        v64 = np.linalg.svd(A.astype(np.float64))[2][3]
        if v[3] == 0 or v64[3] == 0:
            continue
        x, x64 = v[:3] / v[3], v64[:3] / v64[3]
        worst = max(worst, float(np.linalg.norm(x - x64) / np.linalg.norm(x64)))
    print(f"float Jacobi SVD: largest relative deviation from float64 {worst:.3e} (allowed {SVD_ALLOWED:.3e})")
    assert worst <= SVD_ALLOWED
