#!/usr/bin/env python3
"""Measurement of the last-frame SearchByProjection (rsc_search_by_projection_last_many) and of the
TrackWithMotionModel driver (rsc_track_motion_model_many) on the MI355X (needs the GPU; it fails without one).
Writes one JSON file (default profiles/r12/lastproj_bench.json).

Shapes: one frame pair of 2,000 current features and 2,000 LastFrame slots (tests/lastproj_cases.random_problem:
clusters that compete for features, 30 % slots without observations, 10 % outliers or empty, 30 % monocular
features, entry occupants of both kinds) at th = 7 and th = 15, one call of 16 such pairs at th = 7, and the
driver on one pair of tests/track_motion_cases.make_pair (2,000 slots, th = 7).  Baseline: the emulation
library's single-core sequential C++ loop (tests/lastproj_emu, -O3: the reference's slot-by-slot matcher
walking every window) over the same inputs, one problem after another.

Timing: every figure is the median of `--reps` calls after `--warmup` calls of the same shape.  GPU call times
are a host clock around the C entry point, which returns after the stream is synchronised and the results are on
the host (they include the upload of the per-call flags and the download of out; the Frame and LastFrame views
are resident); setup_ms / rounds_ms are device-event times around each kernel.  The CPU time is a host clock
around the emulation's C call alone.  The driver has no CPU baseline here (its optimisation is the oracle's)."""
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
from rsc import engine  # noqa: E402
import lastproj_cases as lc  # noqa: E402
import lastproj_emu_lib as le  # noqa: E402
import track_motion_cases as tc  # noqa: E402


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                reps=len(ms))


def _views(ctx, ps):
    fvs = [engine.FrameView(ctx, p.frame) for p in ps]
    for v, p in zip(fvs, ps):
        v.set_stereo(p.frame.u_right, p.frame.mbf)
    return fvs, [engine.LastFrameView(ctx, p.last) for p in ps]


def _poses(ps, key):
    return np.ascontiguousarray(np.stack([np.asarray(getattr(p, key), np.float32).reshape(16) for p in ps]))


def bench_shape(ctx, ps, reps, warmup):
    L = engine.load_library()
    c = len(ps)
    fvs, lvs = _views(ctx, ps)
    occ = [np.ascontiguousarray(p.frame_occ, np.uint8) for p in ps]
    mb = np.array([p.mb for p in ps], np.float32)
    out = [np.full(p.frame.n, -7, np.int32) for p in ps]
    nm, mode, rounds = (np.zeros(c, np.int32) for _ in range(3))
    args = (ctx.h, engine._handles(fvs), engine._handles(lvs), c, _poses(ps, "Tcw_cur"), _poses(ps, "Tcw_last"), mb,
            engine._ptrs(occ), float(ps[0].th), int(ps[0].check_ori), engine._ptrs(out), nm, mode, rounds)
    ctx.enable_timing(True)
    call, setup_ms, rounds_ms = [], [], []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        st = L.rsc_search_by_projection_last_many(*args)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0, st
        if r >= warmup:
            call.append(dt)
            t = ctx.last_timing()
            setup_ms.append(t["solve_ms"])   # slot 0: the setup kernel
            rounds_ms.append(t["scan_ms"])   # slot 1: the rounds kernel
    ctx.enable_timing(False)
    packed = [le.pack(p) for p in ps]
    emu = le.lib(o3=True)
    e_out = [np.full(p.frame.n, -7, np.int32) for p in ps]
    e_cnt = [np.zeros(4, np.int32) for _ in ps]
    cpu = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        for (q, _), o, cn in zip(packed, e_out, e_cnt):
            emu.lse_search_sequential(C.byref(q), o, cn)
        dt = (time.perf_counter() - t0) * 1e3
        if r >= warmup:
            cpu.append(dt)
    same = all(np.array_equal(o, eo) and int(nm[k]) == int(cn[0]) and int(mode[k]) == int(cn[1])
               for k, (o, eo, cn) in enumerate(zip(out, e_out, e_cnt)))
    g, cp = statistics.median(call), statistics.median(cpu)
    return dict(problems=c, features=int(ps[0].frame.n), slots=int(ps[0].last.n), th=float(ps[0].th),
                nmatches=[int(v) for v in nm[:4]], mode=[int(v) for v in mode[:4]],
                rounds=[int(v) for v in rounds[:4]], outputs_equal_bitwise=bool(same), gpu_call=stats(call),
                gpu_setup_kernel=stats(setup_ms), gpu_rounds_kernel=stats(rounds_ms),
                cpu_one_core_sequential=stats(cpu), cpu_over_gpu_call=round(cp / g, 3),
                synchronised="the C call returns after hipStreamSynchronize")


def bench_driver(ctx, p, reps, warmup):
    L = engine.load_library()
    fvs, lvs = _views(ctx, [p])
    out, disc = [np.full(p.frame.n, -7, np.int32)], [np.full(p.frame.n, -7, np.int32)]
    res = (engine.TrackMotionResult * 1)()
    args = (ctx.h, engine._handles(fvs), engine._handles(lvs), 1, _poses([p], "Tcw_cur"), _poses([p], "Tcw_last"),
            np.array([p.mb], np.float32), float(p.th), np.zeros(1, np.int32), res, engine._ptrs(out),
            engine._ptrs(disc))
    call = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        st = L.rsc_track_motion_model_many(*args)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0, st
        if r >= warmup:
            call.append(dt)
    return dict(features=int(p.frame.n), slots=int(p.last.n), th=float(p.th), ok=int(res[0].ok),
                searches=int(res[0].searches), nmatches=int(res[0].nmatches), n_good=int(res[0].n_good),
                gpu_call=stats(call), stages="search, PoseOptimization, discard loop on the host",
                synchronised="the C call returns after hipStreamSynchronize")


def resource_usage():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "orb-slam2-optimized_amd", "csrc", "lastproj.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
           "-fno-gpu-flush-denormals-to-zero", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", os.devnull]
    try:
        err = subprocess.run(cmd, capture_output=True, text=True, timeout=300).stderr
    except (OSError, subprocess.TimeoutExpired) as e:
        return dict(error=str(e))
    out = {}
    for part in err.split("Function Name: ")[1:]:
        sym = part.split()[0]
        name = next((k for k in ("lastproj_setup_kernel", "lastproj_kernel") if k in sym), sym)
        out[name] = {}
        for key in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                    "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", part)
            if m:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "lastproj_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resources-only", action="store_true", help="print the compiler's resource report (no GPU)")
    a = ap.parse_args()
    if a.resources_only:
        print(json.dumps(resource_usage()))
        return
    ctx = engine.Context(0)  # raises without a GPU: no fallback
    make = lambda seed, th: lc.random_problem(seed, th, 0, n_frame=2000, n_last=2000, n_clusters=60)
    one_th7, one_th15 = make(100, 7.0), make(100, 15.0)
    batch = [one_th7] + [make(101 + k, 7.0) for k in range(15)]
    res = dict(one_pair_th7=bench_shape(ctx, [one_th7], a.reps, a.warmup),
               one_pair_th15=bench_shape(ctx, [one_th15], a.reps, a.warmup),
               batch_16_th7=bench_shape(ctx, batch, a.reps, a.warmup),
               driver_one_pair=bench_driver(ctx, tc.make_pair(200, 1940, 0.002, n_wrong=100, no_obs_frac=0.2), a.reps,
                                            a.warmup),
               kernel_resources=resource_usage())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
