#!/usr/bin/env python3
"""Measurement of Tracking::SearchLocalPoints on the device (rsc_search_local_points_many) on the MI355X
(needs the GPU; it fails without one).  Writes one JSON file (default profiles/r10/localproj_bench.json).

Shapes: one Frame of 2,000 features against 4,000 local MapPoints (tests/localproj_cases.random_problem:
clusters that compete for features, 30 % points without observations, 30 % monocular features, entry
occupants of both kinds) at th = 1 and th = 5, and one call of 16 such problems at th = 5.  Baseline: the
emulation library's single-core sequential C++ loop (tests/localproj_emu, -O3: isInFrustum, then the
reference's point-by-point matcher walking every window) over the same inputs, one problem after another.

Timing: every figure is the median of `--reps` calls after `--warmup` calls of the same shape.  GPU call
times are a host clock around the C entry point, which returns after the stream is synchronised and the
results are on the host (they include the upload of the per-call flags and the download of out and track;
the Frame and MapPoint views are resident); setup_ms / rounds_ms are device-event times around each kernel.
The CPU time is a host clock around the emulation's C call alone."""
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
import localproj_cases as lc  # noqa: E402
import localproj_emu_lib as le  # noqa: E402
import localproj_ref as lr  # noqa: E402


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                reps=len(ms))


def bench_shape(ctx, ps, reps, warmup):
    L = engine.load_library()
    c = len(ps)
    fvs = [engine.FrameView(ctx, p.frame) for p in ps]
    for v, p in zip(fvs, ps):
        v.set_stereo(p.frame.u_right, p.frame.mbf)
    mvs = [engine.MPView(ctx, p.pts) for p in ps]
    T = np.ascontiguousarray(np.stack([np.asarray(p.Tcw, np.float32).reshape(16) for p in ps]))
    keep = [[np.ascontiguousarray(a, np.uint8) for a in (p.skip, p.has_obs, p.frame_occ)] for p in ps]
    out = [np.full(p.frame.n, -7, np.int32) for p in ps]
    tr = [np.zeros(p.pts.n, engine.TRACK_RECORD) for p in ps]
    nm, ntm, rounds = (np.zeros(c, np.int32) for _ in range(3))
    args = (ctx.h, engine._handles(fvs), engine._handles(mvs), c, T, engine._ptrs([k[0] for k in keep]),
            engine._ptrs([k[1] for k in keep]), engine._ptrs([k[2] for k in keep]), float(ps[0].cos_limit),
            float(ps[0].th), float(ps[0].nn_ratio), engine._ptrs(out), engine._ptrs(tr), nm, ntm, rounds)
    ctx.enable_timing(True)
    call, setup_ms, rounds_ms = [], [], []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        st = L.rsc_search_local_points_many(*args)
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
    e_tr = [np.zeros(p.pts.n, lr.TRACK) for p in ps]
    e_cnt = [np.zeros(3, np.int32) for _ in ps]
    cpu = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        for (q, _), o, t, cn in zip(packed, e_out, e_tr, e_cnt):
            emu.lpe_search_sequential(C.byref(q), o, t.ctypes.data, cn)
        dt = (time.perf_counter() - t0) * 1e3
        if r >= warmup:
            cpu.append(dt)
    same = all(np.array_equal(o, eo) and t.tobytes() == et.tobytes() and int(nm[k]) == int(cn[0]) and
               int(ntm[k]) == int(cn[1])
               for k, (o, eo, t, et, cn) in enumerate(zip(out, e_out, tr, e_tr, e_cnt)))
    g, cp = statistics.median(call), statistics.median(cpu)
    return dict(problems=c, features=int(ps[0].frame.n), points=int(ps[0].pts.n), th=float(ps[0].th),
                nmatches=[int(v) for v in nm[:4]], n_to_match=[int(v) for v in ntm[:4]],
                rounds=[int(v) for v in rounds[:4]], outputs_equal_bitwise=bool(same), gpu_call=stats(call),
                gpu_setup_kernel=stats(setup_ms), gpu_rounds_kernel=stats(rounds_ms),
                cpu_one_core_sequential=stats(cpu), cpu_over_gpu_call=round(cp / g, 3),
                synchronised="the C call returns after hipStreamSynchronize")


def resource_usage():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "orb-slam2-optimized_amd", "csrc", "localproj.hip")
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
        name = next((k for k in ("localproj_setup_kernel", "localproj_kernel") if k in sym), sym)
        out[name] = {}
        for key in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                    "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", part)
            if m:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "localproj_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = engine.Context(0)  # raises without a GPU: no fallback
    make = lambda seed, th: lc.random_problem(seed, th, n_frame=2000, n_points=4000, n_clusters=60, n_pairs=60)
    one_th1, one_th5 = make(100, 1.0), make(100, 5.0)
    batch = [one_th5] + [make(101 + k, 5.0) for k in range(15)]
    res = dict(one_frame_th1=bench_shape(ctx, [one_th1], a.reps, a.warmup),
               one_frame_th5=bench_shape(ctx, [one_th5], a.reps, a.warmup),
               batch_16_th5=bench_shape(ctx, batch, a.reps, a.warmup),
               kernel_resources=resource_usage())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
