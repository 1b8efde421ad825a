#!/usr/bin/env python3
"""Measurement of the batched MapPoint update on the MI355X (rsc_update_map_points_many: ComputeDistinctiveDescriptors
and UpdateNormalAndDepth; needs the GPU, it fails without one).  Writes one JSON file (default
profiles/r21/mpupdate_bench.json) and a short .md beside it.

Workload: 1,200 points over 20 KeyFrames of 1,500 keypoints, what = 3.  List lengths: 92 % uniform in 2..12, 6 %
in 13..40, 2 % in 60..100 (so a few dozen points take the one-point-per-workgroup kernel); observations of a list are
distinct (KeyFrame, keypoint) pairs; descriptors are a few centres with up to 40 flipped bits.

Recorded: the kernels' device-event time (rsc_context_last_kernel_timing; both launches), the call's host time (it
returns after the stream is synchronised and the five arrays are on the host; the KeyFrame views are resident), and
the emulation library's plain sequential restatement (N x N matrix, sorted rows; tests/mpupdate_emu, -O3) on ONE
CPU core over the same input, outputs compared.  Every figure is the median of --reps calls after --warmup calls,
with min and max as the spread; the CPU clock is around the C call alone (its input is packed before).  Also the
kernels' register / LDS / occupancy lines from -Rpass-analysis=kernel-resource-usage (--resources-only: no GPU)."""
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
import fusekf_cases as fc  # noqa: E402
import mpupdate_cases as mc  # noqa: E402
import mpupdate_emu_lib as me  # noqa: E402
import mpupdate_ref as mr  # noqa: E402


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                reps=len(ms))


def workload(seed=2101, n_points=1200, n_kf=20, n_kp=1500):
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    b = mc.Builder()
    for _ in range(n_kf):
        d = centres[rng.integers(0, len(centres), n_kp)].copy()
        flips = rng.integers(0, 41, n_kp)
        for i in range(n_kp):
            for bit in rng.choice(256, int(flips[i]), replace=False):
                d[i, bit // 8] ^= 1 << (bit % 8)
        b.kf(d, octaves=rng.integers(0, 8, n_kp), Ow=rng.uniform(-3, 3, 3))
    for _ in range(n_points):
        r = rng.random()
        n = int(rng.integers(2, 13)) if r < 0.92 else int(rng.integers(13, 41)) if r < 0.98 else int(rng.integers(60, 101))
        pick = rng.choice(n_kf * n_kp, n, replace=False)
        obs = [(int(x) // n_kp, int(x) % n_kp) for x in pick]
        b.point(rng.uniform(-2, 2, 3) + (0, 0, 6), obs, ref=obs[int(rng.integers(0, n))])
    return b.problem()


def resource_usage():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "orb-slam2-optimized_amd", "csrc", "mpupdate.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
           "-fno-gpu-flush-denormals-to-zero", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", os.devnull]
    try:
        err = subprocess.run(cmd, capture_output=True, text=True, timeout=300).stderr
    except (OSError, subprocess.TimeoutExpired) as e:
        return dict(error=str(e))
    out = {}
    for part in err.split("Function Name: ")[1:]:
        name = "wave" if "mpupdate_wave_kernel" in part.split()[0] else "block"
        res = {}
        for key in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                    "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", part)
            if m:
                res[key] = int(m.group(1))
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "mpupdate_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resources-only", action="store_true", help="print the kernels' resources alone; needs no GPU")
    a = ap.parse_args()
    if a.resources_only:
        print(json.dumps(resource_usage(), indent=1))
        return
    ctx = engine.Context(0)  # raises without a GPU: no fallback
    p = workload()
    sizes = np.diff(p.upd.obs_begin)
    rng = np.random.default_rng(3)
    kvs = []
    for v in p.kfs:
        kp = np.stack([rng.uniform(2, 750, v.n), rng.uniform(2, 478, v.n)], 1).astype(np.float32)
        kf = fc.make_kf(kp, v.octave, v.desc, np.full(v.n, -1.0), Ow=v.Ow)
        kv = engine.KFView(ctx, kf)
        kv.set_triangulation(kf)
        kvs.append(kv)
    ctx.enable_timing(True)
    call, kern, got = [], [], None
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        got = engine.update_map_points_many(ctx, kvs, p.upd, 3)
        dt = (time.perf_counter() - t0) * 1e3
        if r >= a.warmup:
            call.append(dt)
            kern.append(ctx.last_timing()["refine_ms"])
    ctx.enable_timing(False)
    pk, keep = me.pack(p)
    n = p.upd.n_points
    F = mr.FILL
    cpu_res = dict(desc=np.full((n, 32), F["desc"], np.uint8), best_obs=np.full(n, F["best_obs"], np.int32),
                   normal=np.full((n, 3), F["normal"], np.float32), dmax=np.full(n, F["dmax"], np.float32),
                   dmin=np.full(n, F["dmin"], np.float32), updated=np.zeros(n, np.uint8))
    o = me.Out()
    for k, arr in cpu_res.items():
        setattr(o, k, arr.ctypes.data)
    L = me.lib()
    cpu = []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        st = L.mpue_update(C.byref(pk), 3, 0, C.byref(o))
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0
        if r >= a.warmup:
            cpu.append(dt)
    res = dict(library=os.path.relpath(engine.LIB_PATH, ROOT), points=int(n), keyframes=len(p.kfs), observations=int(sizes.sum()),
               list_length=dict(median=int(np.median(sizes)), max=int(sizes.max()), over_64=int((sizes > 64).sum()),
                                over_12=int((sizes > 12).sum())),
               outputs_equal=mr.same_result(got, cpu_res) == "", gpu_call=stats(call), gpu_kernels=stats(kern),
               cpu_one_core_sequential=stats(cpu),
               gpu_call_over_cpu=round(statistics.median(call) / statistics.median(cpu), 3),
               synchronised="the C call returns after hipStreamSynchronize", kernel_resources=resource_usage())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.splitext(a.out)[0] + ".md", "w") as f:
        f.write("# Batched MapPoint update (tools/mpupdate_bench.py)\n\n"
                f"{n} points over {len(p.kfs)} KeyFrames, {int(sizes.sum())} observations (list length: median "
                f"{int(np.median(sizes))}, max {int(sizes.max())}, {int((sizes > 64).sum())} lists over 64), what = 3; "
                f"median of {a.reps} calls after {a.warmup}, (min .. max).\n\n"
                "| | median ms | min | max |\n|---|---|---|---|\n")
        for label, key in (("kernels (device events, both launches)", "gpu_kernels"),
                           ("call (host clock, synchronised, results on the host)", "gpu_call"),
                           ("one CPU core, sequential restatement (-O3)", "cpu_one_core_sequential")):
            s = res[key]
            f.write(f"| {label} | {s['median_ms']} | {s['min_ms']} | {s['max_ms']} |\n")
        f.write(f"\nOutputs equal bit for bit: {res['outputs_equal']}.  Numbers: {os.path.basename(a.out)}.\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
