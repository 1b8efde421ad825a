#!/usr/bin/env python3
"""Measurement of the CreateNewMapPoints driver (rsc_create_new_map_points_many) on the MI355X (needs the GPU; it
fails without one).  Writes one JSON file (default profiles/r16/triang_bench.json).

Shapes: one current KeyFrame of 2,000 features against 10 neighbours in one driver call (tests/triang_cases.scene:
2,000 world points seen by all KeyFrames, 30 % of the slots with a MapPoint, 30 % stereo keypoints, 0.4 px keypoint
noise, up to 20 flipped descriptor bits), once with 100 FeatureVector nodes of 20 features ("even") and once with
node sizes drawn from a Zipf law over 300 nodes, from 1 to a few hundred features ("skewed": all three lane-group
widths run).  Baseline: the emulation library's
literal neighbour loop (tests/triang_emu, -O3, one core: slots filled as it goes) over the same inputs.

Timing: medians of `--reps` calls after `--warmup` calls.  The GPU time is a host clock around the synchronous C
entry point with resident views (it includes ComputeF12, the two launches' staging and the host replay); the CPU
time a host clock around the emulation's C call alone.  The outputs of the two are asserted equal bit for bit."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests"), ROOT]
import numpy as np  # noqa: E402
from rsc import engine  # noqa: E402
import triang_cases as tc  # noqa: E402
import triang_emu_lib as el  # noqa: E402


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "triang_bench.json"))
    a = ap.parse_args()
    res = {}
    for shape in ("even", "skewed"):
        res[shape] = run_shape(a, shape)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def run_shape(a, shape):
    rng = np.random.default_rng(61)
    nodes = None
    if shape == "skewed":
        w = 1.0 / np.arange(1, 301) ** 1.2
        nodes = 11 + rng.choice(300, size=a.features, p=w / w.sum())
    poses = [(tc.I3, (0, 0, 0))] + [(tc.I3, (rng.uniform(-0.8, 0.8), rng.uniform(-0.2, 0.2), rng.uniform(-0.5, 0.5)))
                                    for _ in range(a.neighbours)]
    kfs, _ = tc.scene(rng, poses, a.features, mp_frac=0.3, node_groups=100, stereo_frac=0.3, noise=0.4, flips=20,
                      nodes=nodes)
    cur, neigh = kfs[0], kfs[1:]
    ctx = engine.Context(0)

    def views(k):
        v = engine.KFView(ctx, k)
        v.set_triangulation(k)
        return engine.BowView(ctx, k), v
    vc, vn = views(cur), [views(k) for k in neigh]
    call = lambda: engine.create_new_map_points_many(ctx, [vc[0]], [vc[1]], [[v[0] for v in vn]], [[v[1] for v in vn]])
    packed = (el.pack(cur), [el.pack(k) for k in neigh])
    cpu = lambda: el.create_new_map_points(cur, neigh, o3=True, packed=packed)
    g, c = call(), cpu()
    assert np.array_equal(g["new_neighbour"][0], c["new_neighbour"]) and np.array_equal(g["new_idx2"][0], c["new_idx2"])
    assert np.array_equal(g["new_pos"][0].view(np.uint32), c["new_pos"].view(np.uint32))
    assert int(g["nnew"][0]) == c["nnew"]
    times = {}
    for name, fn in (("gpu_call", call), ("cpu_one_core", cpu)):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            t = time.perf_counter()
            fn()
            ms.append(1e3 * (time.perf_counter() - t))
        times[name] = stats(ms)
    sizes = np.diff(cur.node_begin)
    return dict(shape=dict(features=a.features, neighbours=a.neighbours, nnew=int(c["nnew"]),
                          node_sizes=dict(nodes=len(sizes), min=int(sizes.min()), median=int(np.median(sizes)),
                                          max=int(sizes.max())),
                          per_neighbour=np.bincount(c["new_neighbour"][c["new_neighbour"] >= 0],
                                                    minlength=a.neighbours).tolist()),
               outputs_equal=True, **times,
               cpu_over_gpu=round(times["cpu_one_core"]["median_ms"] / times["gpu_call"]["median_ms"], 3))


if __name__ == "__main__":
    main()
