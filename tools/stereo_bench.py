#!/usr/bin/env python3
"""Measurement of the device stereo matcher on the MI355X (rsc_compute_stereo_matches_many:
Frame::ComputeStereoMatches; needs the GPU, it fails without one).  Writes one JSON file (default
profiles/r22/stereo_bench.json) and a short .md beside it.

Workload: the EuRoC shape, 1,200 left and 1,200 right keypoints over 8 levels per frame (tests/stereo_cases.py
random_frame: every left keypoint has a partner within a row, a disparity up to 200 px, 3 to 73 flipped bits), for
count = 1 and count = 64 frames in one call (eight distinct frames, each on eight views of its own).

Recorded per count: the kernels' device-event time (rsc_context_last_kernel_timing: match, cut, both), the call's
host time with set_stereo = 1 (it returns after the stream is synchronised, mvuRight / mvDepth are on the host and
the views hold mvuRight; the left views are resident), the emulation library's sequential path (the reference's sort
and binary searches; tests/stereo_emu, -O3) on ONE CPU core over the same frames, and the per-frame sequence it
replaces: that host path followed by rsc_frameview_set_stereo, frame after frame.  Outputs are compared.  Every
figure is the median of --reps runs after --warmup runs, with min and max as the spread; clocks are not touched.
Also the kernels' register / LDS / occupancy lines from -Rpass-analysis=kernel-resource-usage (--resources-only: no
GPU)."""
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
import stereo_cases as sc  # noqa: E402
import stereo_emu_lib as se  # noqa: E402
import stereo_ref as sr  # noqa: E402

N_LEFT = N_RIGHT = 1200


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                reps=len(ms))


def resource_usage():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "orb-slam2-optimized_amd", "csrc", "stereo.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
           "-fno-gpu-flush-denormals-to-zero", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", os.devnull]
    try:
        err = subprocess.run(cmd, capture_output=True, text=True, timeout=300).stderr
    except (OSError, subprocess.TimeoutExpired) as e:
        return dict(error=str(e))
    out = {}
    for part in err.split("Function Name: ")[1:]:
        name = "match" if "stereo_match_kernel" in part.split()[0] else "cut"
        res = {}
        for key in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                    "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", part)
            if m:
                res[key] = int(m.group(1))
        out[name] = res
    return out


class HostFrame:
    """A frame packed for the emulation library, with output arrays of its own."""

    def __init__(self, fr):
        self.f, self.keep = se.pack(fr)
        n = len(fr.kp)
        self.u, self.z = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.br, self.bd = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.res = se.Result()
        self.o = se.Out(self.u.ctypes.data, self.z.ctypes.data, self.br.ctypes.data, self.bd.ctypes.data,
                        C.pointer(self.res))

    def run(self, L):
        assert L.stme_compute(C.byref(self.f), 0, C.byref(self.o)) == 0


def measure(ctx, frames, reps, warmup):
    count = len(frames)
    views = [engine.FrameView(ctx, synth.make_proj_frame(fr.kp, fr.octave, np.zeros(len(fr.kp), np.float32), fr.desc))
             for fr in frames]
    mbf, mb = [fr.mbf for fr in frames], [fr.mb for fr in frames]
    call, kern, match, cut, got = [], [], [], [], None
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        got = engine.compute_stereo_matches_many(ctx, views, frames, mbf, mb, True, False)
        dt = (time.perf_counter() - t0) * 1e3
        if r >= warmup:
            t = ctx.last_timing()
            call.append(dt)
            kern.append(t["refine_ms"])
            match.append(t["solve_ms"])
            cut.append(t["scan_ms"])
    L = se.lib()
    host = [HostFrame(fr) for fr in frames]
    cpu, seq = [], []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        for h in host:
            h.run(L)
        dt = (time.perf_counter() - t0) * 1e3
        if r >= warmup:
            cpu.append(dt)
    for r in range(warmup + reps):  # the per-frame sequence the call replaces: host stereo, then the upload
        t0 = time.perf_counter()
        for h, v, fr in zip(host, views, frames):
            h.run(L)
            v.set_stereo(h.u, fr.mbf)
        dt = (time.perf_counter() - t0) * 1e3
        if r >= warmup:
            seq.append(dt)
    equal = all(np.array_equal(g["u_right"].view(np.uint32), h.u.view(np.uint32)) and
                np.array_equal(g["depth"].view(np.uint32), h.z.view(np.uint32)) and
                (g["n_candidates"], g["n_removed"], g["median"]) == (h.res.n_candidates, h.res.n_removed, h.res.median)
                for g, h in zip(got, host))
    return dict(count=count, outputs_equal=bool(equal), accepted=int(sum(g["n_candidates"] for g in got)),
                removed=int(sum(g["n_removed"] for g in got)), gpu_call=stats(call), gpu_kernels=stats(kern),
                gpu_match_kernel=stats(match), gpu_cut_kernel=stats(cut), cpu_one_core_sequential=stats(cpu),
                cpu_stereo_then_set_stereo=stats(seq),
                gpu_call_over_cpu=round(statistics.median(call) / statistics.median(cpu), 3),
                gpu_call_over_sequence=round(statistics.median(call) / statistics.median(seq), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "stereo_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resources-only", action="store_true", help="print the kernels' resources alone; needs no GPU")
    a = ap.parse_args()
    if a.resources_only:
        print(json.dumps(resource_usage(), indent=1))
        return
    ctx = engine.Context(0)  # raises without a GPU: no fallback
    distinct = [sc.random_frame(2200 + k, N_LEFT, N_RIGHT, k % 2 == 1) for k in range(8)]
    ctx.enable_timing(True)
    runs = [measure(ctx, distinct[:1], a.reps, a.warmup), measure(ctx, distinct * 8, a.reps, a.warmup)]
    ctx.enable_timing(False)
    res = dict(library=os.path.relpath(engine.LIB_PATH, ROOT), left=N_LEFT, right=N_RIGHT, levels=sc.N_LEVELS, runs=runs,
               synchronised="the C call returns after hipStreamSynchronize", kernel_resources=resource_usage())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.splitext(a.out)[0] + ".md", "w") as f:
        f.write("# Device ComputeStereoMatches (tools/stereo_bench.py)\n\n"
                f"{N_LEFT} left x {N_RIGHT} right keypoints, {sc.N_LEVELS} levels per frame; median of {a.reps} runs after "
                f"{a.warmup}, (min .. max); times are for the whole batch.\n")
        for run in runs:
            f.write(f"\n## count = {run['count']} ({run['accepted']} accepted, {run['removed']} removed by the cut)\n\n"
                    "| | median ms | min | max |\n|---|---|---|---|\n")
            for label, key in (("match kernel (device events)", "gpu_match_kernel"), ("cut kernel", "gpu_cut_kernel"),
                               ("both kernels", "gpu_kernels"),
                               ("call, set_stereo = 1 (host clock, synchronised, results on the host)", "gpu_call"),
                               ("one CPU core, sequential path (-O3)", "cpu_one_core_sequential"),
                               ("one CPU core, then rsc_frameview_set_stereo, frame by frame", "cpu_stereo_then_set_stereo")):
                s = run[key]
                f.write(f"| {label} | {s['median_ms']} | {s['min_ms']} | {s['max_ms']} |\n")
            f.write(f"\nOutputs equal bit for bit: {run['outputs_equal']}.\n")
        f.write(f"\nNumbers: {os.path.basename(a.out)}.\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
