#!/usr/bin/env python3
"""Measurement of the relocalization SearchByProjection matcher on the MI355X (needs the GPU; it fails
without one).  Writes one JSON file (default profiles/r07/frameproj_bench.json):

(a) one launch of 15 problems of relocalization shape (Frame 2000 features, KeyFrame 2000 slots with about
    1500 MapPoints, th = 10, ORBdist = 100) against the emulation library's sequential loop over the same
    per-MapPoint functions on ONE CPU core, same inputs, with the observed fixed-point rounds;
(b) rsc_reloc_events_refined against rsc_reloc_events_gated on one 15-candidate event whose first success
    is refined to a match: what the extra stages cost over the hand-off;
(c) the kernel's VGPR / LDS / occupancy line from -Rpass-analysis=kernel-resource-usage.

Timing: every figure is the median of `--reps` calls after `--warmup` calls of the same shape.  GPU call
times are a host clock around the C entry point, which returns after the stream is synchronised and the
results are on the host (so they include the upload of the call's flags and the download of its
outputs; the views are resident); kernel_ms is the device-event time around the launch alone.  The CPU
time is a host clock around the emulation's C call alone (its inputs are packed before)."""
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
from rsc import engine, events as rev, synth  # noqa: E402
import frameproj_emu_lib as fe  # noqa: E402


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                reps=len(ms))


def bench_search(ctx, reps, warmup):
    rng = np.random.default_rng(2025)
    ps = [synth.make_reloc_projection_problem(rng, 2000, 2000, n_clusters=8) for _ in range(15)]
    fvs = [engine.FrameView(ctx, p.frame) for p in ps]
    kvs = [engine.KFView(ctx, p.kf) for p in ps]
    for kv, p in zip(kvs, ps):
        kv.set_angles(p.kf.angle)
    args = ([p.Tcw for p in ps], [p.already for p in ps], [p.frame_mp for p in ps], 10, 100, True)
    ctx.enable_timing(True)
    call, kern = [], []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        outs, nm, rounds = engine.search_by_projection_many(ctx, fvs, kvs, *args)
        dt = (time.perf_counter() - t0) * 1e3
        if r >= warmup:
            call.append(dt)
            kern.append(ctx.last_timing()["refine_ms"])
    ctx.enable_timing(False)
    packed = [fe.pack(p.frame, p.kf, p.Tcw, p.already, p.frame_mp, 10, 100, True) for p in ps]
    cpu_out = [np.full(p.frame.n, -7, np.int32) for p in ps]
    L = fe.lib()
    cpu = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        cn = [L.fpe_search_sequential(C.byref(pk[0]), o) for pk, o in zip(packed, cpu_out)]
        dt = (time.perf_counter() - t0) * 1e3
        if r >= warmup:
            cpu.append(dt)
    same = all(np.array_equal(a, b) for a, b in zip(outs, cpu_out)) and list(nm) == cn
    g, c = statistics.median(call), statistics.median(cpu)
    return dict(problems=len(ps), frame_n=2000, kf_n=2000,
                map_points=[int((p.kf.mp_state == 1).sum()) for p in ps], th=10, orb_dist=100,
                nmatches=[int(x) for x in nm], rounds=[int(x) for x in rounds], outputs_equal=bool(same),
                gpu_call=stats(call), gpu_kernel=stats(kern), cpu_one_core_sequential=stats(cpu),
                gpu_call_over_cpu=round(g / c, 3), synchronised="the C call returns after hipStreamSynchronize")


def bench_event(ctx, reps, warmup):
    rng = np.random.default_rng(77)
    spec = [(35, 10, None)] + [(12, 30, None)] * 14
    p, cs = synth.make_reloc_refine_event(rng, 2000, 2000, spec)
    seeds = np.arange(1, len(cs) + 1, dtype=np.uint32)
    eb = engine.EventBatch([[engine.PnPSolver(ctx, sc, int(s)) for (_, _, sc), s in zip(cs, seeds)]])
    fv = engine.FrameView(ctx, p.frame)
    kv = engine.KFView(ctx, p.kf)
    kv.set_angles(p.kf.angle)
    cands = [[(kv, m) for _, m, _ in cs]]
    t_ref, t_gate = [], []
    for r in range(warmup + reps):  # alternating
        for which in (0, 1):
            eb.batch.reset(seeds)
            eb.batch.set_ransac_parameters(*rev.RELOC_PARAMS)
            t0 = time.perf_counter()
            if which == 0:
                res, _ = eb.run_reloc_refined([fv], [(None, 0.0)], cands)
            else:
                gres, _, _ = eb.run_reloc_gated([(None, 0.0)])
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                (t_ref if which == 0 else t_gate).append(dt)
    rec = {k: int(res[k][0]) for k in ("status", "winner", "round", "n_good", "n_good_first", "gates", "chains")}
    rec["n_additional"] = [int(x) for x in res["n_additional"][0]]
    return dict(candidates=len(cs), refined_record=rec, gated_status=int(gres["status"][0]),
                refined=stats(t_ref), gated=stats(t_gate),
                extra_ms=round(statistics.median(t_ref) - statistics.median(t_gate), 4))


def resource_usage():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "orb-slam2-optimized_amd", "csrc", "frameproj.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
           "-fno-gpu-flush-denormals-to-zero", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", os.devnull]
    try:
        err = subprocess.run(cmd, capture_output=True, text=True, timeout=300).stderr
    except (OSError, subprocess.TimeoutExpired) as e:
        return dict(error=str(e))
    out = {}
    for part in err.split("Function Name: ")[1:]:
        name = "frameproj_setup_kernel" if "frameproj_setup_kernel" in part.split()[0] else "frameproj_kernel"
        out[name] = {}
        for key in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                    "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", part)
            if m:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "frameproj_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = engine.Context(0)  # raises without a GPU: no fallback
    res = dict(search=bench_search(ctx, a.reps, a.warmup), event=bench_event(ctx, a.reps, a.warmup),
               kernel_resources=resource_usage())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
