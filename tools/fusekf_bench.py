#!/usr/bin/env python3
"""Measurement of the KeyFrame Fuse of LocalMapping::SearchInNeighbors on the MI355X (rsc_fuse_kf_many; needs the
GPU, it fails without one).  Writes one JSON file (default profiles/r18/fusekf_bench.json):

(a) forward: the current KeyFrame's ~1,200 MapPoints against 30 target KeyFrames of 2,000 features (30 % stereo),
    th = 3, one launch;
(b) backward: 15,000 candidate points against one KeyFrame, one launch;
both against the emulation library's sequential loop over the same per-pair function on ONE CPU core (-O3), same
inputs, outputs compared, and
(c) the kernel's VGPR / SGPR / scratch / LDS / occupancy lines from -Rpass-analysis=kernel-resource-usage for the
    16-lane and the one-lane form.

The walk form is a build switch.  To compare the two, build the other library first
    make -C tools variant NAME=fusekf1 SRC=fusekf DEFS=-DRSC_FUSEKF_LANES=1
and run this tool once per library (RSC_LIBRSC=tools/bin/librsc_fusekf1.so, --label lanes1), alternating; each run
writes its own file and --merge joins them.

Timing: every figure is the median of `--reps` calls after `--warmup` calls of the same shape, with min and max as
the spread.  GPU call times are a host clock around the C entry point, which returns after the stream is
synchronised and the results are on the host (so they include the upload of the skip flags and the download of
best_idx; the views are resident); kernel_ms is the device-event time around the launch alone.  The CPU time is a
host clock around the emulation's C calls alone (their inputs are packed before)."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests"), ROOT]
import numpy as np  # noqa: E402
from rsc import engine, synth  # noqa: E402
import fusekf_cases as fc  # noqa: E402
import fusekf_emu_lib as fe  # noqa: E402
import kfproj_ref as kr  # noqa: E402


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                reps=len(ms))


def timed(fn, reps, warmup, ctx=None):
    call, kern, res = [], [], None
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        res = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if r >= warmup:
            call.append(dt)
            if ctx is not None:
                kern.append(ctx.last_timing()["refine_ms"])
    return res, call, kern


def scene(seed, n_kf, n_points, n_poses):
    """(pts, KeyFrames, skips): fusekf_cases.random_problem at the bench's sizes.  The generator gives every
    keypoint a point of its own; a KeyFrame with fewer MapPoints than features keeps a random subset of them."""
    n_gen = max(n_points, n_kf + 200)
    pts, kfs, skips = fc.random_problem(seed, n_kf, n_gen, n_poses)
    if n_gen != n_points:
        sel = np.sort(np.random.default_rng(seed).choice(n_gen, n_points, replace=False))
        pts = kr.points_of(state=pts.state[sel], pos=pts.pos[sel], normal=pts.normal[sel], dmax=pts.dmax[sel],
                           dmin=pts.dmin[sel], desc=pts.desc[sel])
        skips = [s[sel] for s in skips]
    return pts, kfs, skips


def bench(ctx, pts, kfs, skips, reps, warmup):
    kvs = []
    for kf in kfs:
        v = engine.KFView(ctx, kf)
        v.set_triangulation(kf)
        kvs.append(v)
    mv = engine.MPView(ctx, pts)
    ctx.enable_timing(True)
    (best, nf), call, kern = timed(lambda: engine.fuse_kf_many(ctx, kvs, [mv] * len(kvs), skips, fc.TH), reps, warmup,
                                   ctx)
    ctx.enable_timing(False)
    packed = [fe.pack(kf, pts, sk, fc.TH) for kf, sk in zip(kfs, skips)]
    cpu_best = [np.full(pts.n, -7, np.int32) for _ in kfs]
    L = fe.lib()
    cn, cpu, _ = timed(lambda: [L.fkfe_fuse(C.byref(pk[0]), o) for pk, o in zip(packed, cpu_best)], reps, warmup)
    g, c = statistics.median(call), statistics.median(cpu)
    same = all(np.array_equal(a, b) for a, b in zip(best, cpu_best)) and [int(x) for x in nf] == cn
    return dict(keyframes=len(kfs), kf_n=kfs[0].n, points=pts.n, pairs=len(kfs) * pts.n, th=fc.TH,
                nfused_total=int(sum(int(x) for x in nf)), outputs_equal=bool(same), gpu_call=stats(call),
                gpu_kernel=stats(kern), cpu_one_core_sequential=stats(cpu), gpu_call_over_cpu=round(g / c, 3),
                synchronised="the C call returns after hipStreamSynchronize")


def resource_usage():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "orb-slam2-optimized_amd", "csrc", "fusekf.hip")
    out = {}
    for lanes in (16, 1):
        cmd = [hipcc, f"-DRSC_FUSEKF_LANES={lanes}", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
               "-fno-fast-math", "-fno-gpu-flush-denormals-to-zero", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
        try:
            err = subprocess.run(cmd, capture_output=True, text=True, timeout=300).stderr
        except (OSError, subprocess.TimeoutExpired) as e:
            out[f"lanes{lanes}"] = dict(error=str(e))
            continue
        part = err.split("Function Name: ")[-1]
        res = {}
        for key in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                    "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", part)
            if m:
                res[key] = int(m.group(1))
        out[f"lanes{lanes}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "fusekf_bench.json"))
    ap.add_argument("--label", default="lanes16", help="the walk form of the library under test")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resources-only", action="store_true", help="print (c) alone; needs no GPU")
    ap.add_argument("--merge", nargs="+", help="join the per-library files into --out and stop")
    a = ap.parse_args()
    if a.resources_only:
        print(json.dumps(resource_usage(), indent=1))
        return
    if a.merge:
        res = {}
        for path in a.merge:
            with open(path) as f:
                res.update(json.load(f))
        res["kernel_resources"] = resource_usage()
    else:
        ctx = engine.Context(0)  # raises without a GPU: no fallback
        pts, kfs, skips = scene(2031, 2000, 1200, 30)
        fwd = bench(ctx, pts, kfs, skips, a.reps, a.warmup)
        pts, kfs, skips = scene(2032, 2000, 15000, 1)
        back = bench(ctx, pts, kfs, skips, a.reps, a.warmup)
        res = {a.label: dict(library=engine.LIB_PATH, forward=fwd, backward=back)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
