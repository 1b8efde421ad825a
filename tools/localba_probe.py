"""LocalBundleAdjustment on one problem of the workload's own shape — 20 free and 30 fixed KeyFrames, 3,000 points,
about 15,000 edges, 70 % stereo, 1 px noise, 5 % outliers — on the device (rsc_local_bundle_adjustment_many, HIP-event
time of the call and of every stage) and as the sequential host form of tests/localba_emu (built -O3) on one core of
the same machine.  Prints one JSON document; --out writes it to a file as well.

    python tools/localba_probe.py --reps 20 --out profiles/r30/localba_probe.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from rsc import engine, synth  # noqa: E402
import localba_emu_lib as le  # noqa: E402


def stats(v):
    v = np.sort(np.asarray(v, np.float64))
    return dict(median=float(np.median(v)), min=float(v[0]), max=float(v[-1]), n=int(v.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(2030)
    p = synth.make_localba_scene(rng, n_free=20, n_fixed=30, n_points=3000, obs_per_point=(3, 7), stereo_frac=0.7,
                                 noise_px=1.0, pose_perturb=0.005, point_perturb=0.03, outlier_frac=0.05, near=True)
    host = []
    for _ in range(max(3, a.reps // 4)):
        t = time.perf_counter()
        st, ref = le.run(p, 0)
        host.append((time.perf_counter() - t) * 1e3)
        assert st == 0
    ctx = engine.Context(0)
    ctx.enable_timing(True)
    call, wall, stages = [], [], []
    for i in range(a.warmup + a.reps):
        t = time.perf_counter()
        g = engine.local_bundle_adjustment(ctx, p)
        w = (time.perf_counter() - t) * 1e3
        if i >= a.warmup:
            wall.append(w)
            call.append(ctx.last_timing()["refine_ms"])
            stages.append(engine.localba_stage_ms(ctx))
    same = all(np.array_equal(g[k].view(np.uint8), ref[k].view(np.uint8)) for k in ("Tcw", "pos", "edge_flags", "erase"))
    doc = dict(shape=dict(free_kfs=20, fixed_kfs=30, points=3000, edges=int(len(p["obs_kf"])),
                          stereo=float((p["u_right"] >= 0).mean())),
               device_equals_host=bool(same),
               iterations=[q["lm_iterations"] for q in g["phase"]], trials=[q["lm_trials"] for q in g["phase"]],
               host_iterations=[q["lm_iterations"] for q in ref["phase"]], host_trials=[q["lm_trials"] for q in ref["phase"]],
               n_erase=int(g["n_erase"]),
               device_call_ms=stats(call), device_call_wall_ms=stats(wall), host_one_core_ms=stats(host),
               device_stage_ms={k: stats([s[k] for s in stages]) for k in engine.LOCALBA_STAGES})
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
