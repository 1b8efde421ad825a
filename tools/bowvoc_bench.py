#!/usr/bin/env python3
"""Measurement of the vocabulary transform (ComputeBoW: rsc_voc_transform_many) on the MI355X (needs the
GPU; it fails without one).  Writes one JSON file (default profiles/r09/bowvoc_bench.json).

Vocabulary: ORBvoc-shaped synthetic tree, k = 10, L = 6 (1 111 111 nodes, 10^6 words), levelsup = 4.
Shapes: (a) one Frame of 2000 descriptors, (b) one call of 16 such views.  Baseline: the emulation
library's single-core sequential C++ loop (tests/bowvoc_emu, -O3: per-feature descent, std::map
BowVector and FeatureVector) over the same inputs, one view after another.

Timing: every figure is the median of `--reps` calls after `--warmup` calls of the same shape.  GPU call
times are a host clock around the C entry point, which returns after the stream is synchronised and the
results are on the host (they include the upload of the descriptors and the download of both vectors;
the vocabulary is resident); descend_ms / build_ms are device-event times around each kernel.  The CPU
time is a host clock around the emulation's C call alone."""
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
import bowvoc_emu_lib as be  # noqa: E402


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                reps=len(ms))


def bench_shape(ctx, voc, emu, descs, levelsup, reps, warmup):
    L = engine.load_library()
    c = len(descs)
    n = np.array([len(d) for d in descs], np.int32)
    ptrs = (C.c_void_p * c)(*[d.ctypes.data for d in descs])
    outs = (engine.VocOutput * c)()
    bufs = [engine._VocBuffers(len(d), per_feature=False) for d in descs]
    for b, o in zip(bufs, outs):
        b.fill(o)
    ctx.enable_timing(True)
    call, desc_ms, build_ms = [], [], []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        st = L.rsc_voc_transform_many(voc.h, c, n, ptrs, levelsup, outs)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0, st
        if r >= warmup:
            call.append(dt)
            a, b = voc.last_kernel_timing()
            desc_ms.append(a)
            build_ms.append(b)
    ctx.enable_timing(False)
    gpu = [b.result(o) for b, o in zip(bufs, outs)]
    cpu = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        for d in descs:
            emu.transform_raw(d, levelsup)
        dt = (time.perf_counter() - t0) * 1e3
        if r >= warmup:
            cpu.append(dt)
    same = True
    for d, g in zip(descs, gpu):
        e = emu.transform(d, levelsup)
        same = same and all(np.array_equal(g[k], e[k]) for k in ("word_id", "node_id", "node_begin", "feat")) and \
            np.array_equal(g["word_value"].view(np.uint64), e["word_value"].view(np.uint64))
    g, cp = statistics.median(call), statistics.median(cpu)
    return dict(views=c, descriptors_per_view=int(n[0]), words=[len(x["word_id"]) for x in gpu][:4],
                nodes=[len(x["node_id"]) for x in gpu][:4], outputs_equal_bitwise=bool(same), gpu_call=stats(call),
                gpu_descend_kernel=stats(desc_ms), gpu_build_kernel=stats(build_ms),
                cpu_one_core_sequential=stats(cpu), cpu_over_gpu_call=round(cp / g, 3),
                synchronised="the C call returns after hipStreamSynchronize")


def resource_usage():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "orb-slam2-optimized_amd", "csrc", "bowvoc.hip")
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
        name = next((k for k in ("voc_descend_kernelILi16", "voc_descend_kernelILi32", "voc_build_kernel",
                                 "voc_gather_kernel") if k in sym), sym)
        out[name] = {}
        for key in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                    "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", part)
            if m:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "bowvoc_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = engine.Context(0)  # raises without a GPU: no fallback
    rng = np.random.default_rng(2026)
    nodes = synth.make_vocabulary(rng, 10, 6, zero_weight_frac=0.001)
    voc = engine.Vocabulary(ctx, nodes)
    emu = be.EmuVocabulary(nodes)
    descs = [synth.sample_descriptors(rng, nodes, 2000, mean_flips=12.0) for _ in range(16)]
    info = voc.info()
    res = dict(vocabulary=dict(k=10, L=6, nodes=nodes.n_nodes, words=voc.size, levelsup=4),
               lds_cut=dict(info, staged_bytes=info["lds_nodes"] * 40, budget_bytes=48 * 1024,
                            note="whole levels within the byte budget: levels 0-3 of a k = 10 tree"),
               one_frame=bench_shape(ctx, voc, emu, descs[:1], 4, a.reps, a.warmup),
               batch_16=bench_shape(ctx, voc, emu, descs, 4, a.reps, a.warmup),
               kernel_resources=resource_usage())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
