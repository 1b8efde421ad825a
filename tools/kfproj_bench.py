#!/usr/bin/env python3
"""Measurement of the loop-closing matchers on the MI355X (needs the GPU; it fails without one).  Writes one
JSON file (default profiles/r08/kfproj_bench.json):

(a) one SearchByProjection(pKF, Scw, vpPoints, vpMatched, 10) problem, KeyFrame n = 2000 against 4,000 loop
    points (rsc_search_by_projection_kf_many, count = 1), with the observed fixed-point rounds;
(b) one Fuse batch, 20 KeyFrames against the same 4,000 points (rsc_fuse_sim3_many, one launch);
both against the emulation library's sequential loop over the same per-point functions on ONE CPU core, same
inputs (tests/kfproj_emu: the CPU baseline), and
(c) the kernels' VGPR / LDS / occupancy lines from -Rpass-analysis=kernel-resource-usage.

Timing: every figure is the median of `--reps` calls after `--warmup` calls of the same shape.  GPU call
times are a host clock around the C entry point, which returns after the stream is synchronised and the
results are on the host (so they include the upload of the call's flags and the download of its outputs; the
views are resident); kernel_ms is the device-event time around the call's launches alone (setup kernel +
rounds kernel for (a), the one kernel for (b)).  The CPU time is a host clock around the emulation's C calls
alone (their inputs are packed before)."""
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
import kfproj_emu_lib as ke  # noqa: E402

KERNELS = ("kfproj_setup_kernel", "kfproj_kernel", "kffuse_kernel")


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


def bench_search(ctx, p, reps, warmup):
    kv, mv = engine.KFView(ctx, p.kf), engine.MPView(ctx, p.pts)
    ctx.enable_timing(True)
    (outs, nm, rounds), call, kern = timed(
        lambda: engine.search_by_projection_kf_many(ctx, [kv], [mv], [p.Scw], [p.already], [p.occupied], p.th),
        reps, warmup, ctx)
    ctx.enable_timing(False)
    pk, keep = ke.pack(p.kf, p.pts, p.Scw, p.already, p.occupied, p.th)
    cpu_out = np.full(p.kf.n, -7, np.int32)
    L = ke.lib()
    cn, cpu, _ = timed(lambda: L.kfpe_search_sequential(C.byref(pk), cpu_out), reps, warmup)
    g, c = statistics.median(call), statistics.median(cpu)
    return dict(kf_n=p.kf.n, points=p.pts.n, th=p.th, nmatches=int(nm[0]), rounds=int(rounds[0]),
                outputs_equal=bool(np.array_equal(outs[0], cpu_out) and int(nm[0]) == cn),
                gpu_call=stats(call), gpu_kernels=stats(kern), cpu_one_core_sequential=stats(cpu),
                gpu_call_over_cpu=round(g / c, 3), synchronised="the C call returns after hipStreamSynchronize")


def bench_fuse(ctx, p, n_kfs, reps, warmup):
    rng = np.random.default_rng(31)
    Scw, in_kf = [], []
    for k in range(n_kfs):
        T = np.asarray(p.Scw, np.float64).copy()
        T[:3, :3] = synth.random_rotation(rng, 0.003) @ T[:3, :3]
        T[:3, 3] += rng.normal(0, 0.003, 3)
        T[:3, :] *= 0.9 + 0.01 * k
        Scw.append(T.astype(np.float32))
        in_kf.append((rng.random(p.pts.n) < 0.1).astype(np.uint8))
    kvs = [engine.KFView(ctx, p.kf) for _ in range(n_kfs)]
    mv = engine.MPView(ctx, p.pts)
    ctx.enable_timing(True)
    (best, nf), call, kern = timed(lambda: engine.fuse_sim3_many(ctx, kvs, mv, Scw, in_kf, 4.0), reps, warmup, ctx)
    ctx.enable_timing(False)
    packed = [ke.pack(p.kf, p.pts, S, ik, None, 4.0) for S, ik in zip(Scw, in_kf)]
    cpu_best = [np.full(p.pts.n, -7, np.int32) for _ in range(n_kfs)]
    L = ke.lib()
    cn, cpu, _ = timed(lambda: [L.kfpe_fuse(C.byref(pk[0]), o) for pk, o in zip(packed, cpu_best)], reps, warmup)
    g, c = statistics.median(call), statistics.median(cpu)
    same = all(np.array_equal(a, b) for a, b in zip(best, cpu_best)) and [int(x) for x in nf] == cn
    return dict(keyframes=n_kfs, kf_n=p.kf.n, points=p.pts.n, th=4.0, nfused=[int(x) for x in nf],
                outputs_equal=bool(same), gpu_call=stats(call), gpu_kernel=stats(kern),
                cpu_one_core_sequential=stats(cpu), gpu_call_over_cpu=round(g / c, 3))


def resource_usage():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "orb-slam2-optimized_amd", "csrc", "kfproj.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
           "-fno-gpu-flush-denormals-to-zero", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", os.devnull]
    try:
        err = subprocess.run(cmd, capture_output=True, text=True, timeout=300).stderr
    except (OSError, subprocess.TimeoutExpired) as e:
        return dict(error=str(e))
    out = {}
    for part in err.split("Function Name: ")[1:]:
        name = next((k for k in KERNELS if k in part.split()[0]), part.split()[0])
        out[name] = {}
        for key in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                    "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", part)
            if m:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "kfproj_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resources-only", action="store_true", help="print (c) alone; needs no GPU")
    a = ap.parse_args()
    if a.resources_only:
        print(json.dumps(resource_usage(), indent=1))
        return
    ctx = engine.Context(0)  # raises without a GPU: no fallback
    p = synth.make_loop_projection_problem(np.random.default_rng(2026), 2000, 4000, n_clusters=40)
    res = dict(search=bench_search(ctx, p, a.reps, a.warmup), fuse=bench_fuse(ctx, p, 20, a.reps, a.warmup),
               kernel_resources=resource_usage())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
