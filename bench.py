#!/usr/bin/env python3
"""Headline benchmark: RANSAC hypotheses/s (+ poses/s) of the relocalization EPnP batch.

Workload (BASELINE.json configs[1]): per GPU, 64 relocalization
candidates x 2000 correspondences, SetRansacParameters(0.99,10,300,4,0.5,5.991) (Tracking.cpp:1226)
then iterate(300) on every candidate — 300 hypotheses each (Q1: '||' loop) in exhaustive mode
(40% inliers, minInliers=1000 unreachable), i.e. 19,200 hypotheses per step, all candidates in one
rsc_pnp_iterate_many call.  A "step" = reset every solver with a fresh rand() seed + the call above
(sampling, EPnP solves, inlier scans, selection replay, result records) + the RCCL all-gather of the
per-candidate result records when N > 1.

Multi-GPU: one process per GPU.  Under torchrun the ranks come from the
environment; `python bench.py --gpus N` without WORLD_SIZE starts the N rank processes itself
(before anything touches the GPU) and exits with their status.  Default = weak scaling (64
candidates per GPU); `--strong` splits the one 64-candidate batch across the ranks.

A plain run (`bench.py --gpus 1 --steps K --warmup W`) does only that: set-up, W warm-up steps, the
K timed steps, one JSON line (metric, value, ms_per_step, ...).  `--dump-outputs DIR` also writes what
the last timed step computed (the result records and every hypothesis's pose and inlier count) as
DIR/<name>.npy; the inputs are seeded, so two builds can be compared output for output.

With `--full` the same JSON line carries the rest: the headline's roofline (a second, instrumented
pass of the K steps), sim3 (config 3), mlpnp (config 4 per-GPU share), events (config 5),
single-event latency, the world-1 RCCL check and the SURVEY §8(f) neighbours (PoseOptimization,
SearchByBoW, SearchBySim3, KeyFrameDatabase).  Every RANSAC section carries a cpu_baseline (the oracle
restatement on the host's cores: 1 core and all cores, 3 warm-up batches then the median of >= 10).
The --no-* options and --eig-rows-ab narrow or extend a --full run; they do nothing without it.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "orb-slam2-optimized_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP64_PEAK_TFLOPS = 78.6    # MI355X vector FP64 (spec)
FP32_PEAK_TFLOPS = 157.3   # MI355X vector FP32 (spec)
LDS_PEAK_TBS = 78.6        # 256 CU x 128 B/clk x 2.4 GHz


def _round_dirs():
    """profiles/rNN directories, newest round first (side files come from the newest round that has
    them, so a round that re-measures a file supersedes the older one without a code change)."""
    base = os.path.join(ROOT, "profiles")
    names = [d for d in os.listdir(base) if d[:1] == "r" and d[1:].isdigit()] if os.path.isdir(base) else []
    return tuple(os.path.join("profiles", d) for d in sorted(names, key=lambda d: -int(d[1:])))


PROFILE_DIRS = _round_dirs()


def _profile_json(name):
    """Committed measurement side file (op counts, PMC traffic), from the newest round that has it;
    returns (data, relative path) or (None, None)."""
    for d in PROFILE_DIRS:
        path = os.path.join(ROOT, d, name)
        if os.path.exists(path):
            with open(path) as f:
                return json.load(f), os.path.join(d, name)
    return None, None


def op_count(key):
    """FP64 flops per unit of section `key` from tools/opcount_report.py's opcount.json (None if absent)."""
    opc, _ = _profile_json("opcount.json")
    if not opc:
        return None
    if key in opc and isinstance(opc[key], dict):
        return opc[key].get("fp64_flops_mean")
    return opc.get("fp64_flops_mean") if key == "pnp" else None


def fp64_roofline(kernel, units, flops_per_unit, ms, unit_desc):
    """Roofline object of an FP64-latency-bound solver kernel: algorithmic flops (op-counter build
    of the oracle) per launch / the kernel's HIP-event time, against the FP64 vector peak."""
    if not flops_per_unit or not ms:
        return None
    tf = units * flops_per_unit / (ms * 1e-3) / 1e12
    _, src = _profile_json("opcount.json")
    return {"bound": "fp64-latency", "achieved": round(tf, 4), "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(tf / FP64_PEAK_TFLOPS, 5), "traffic": None, "kernel": kernel,
            "algorithmic_flops_per_launch": round(units * flops_per_unit), "flops_per_unit": flops_per_unit,
            "unit_of_work": unit_desc, "kernel_ms_per_launch": round(ms, 4),
            "sources": {"flops_per_unit": f"{src} (tools/opcount_report.py)", "time": "HIP events, second pass"}}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--candidates", type=int, default=64)
    p.add_argument("--corrs", type=int, default=2000)
    p.add_argument("--iters", type=int, default=300)
    p.add_argument("--strong", action="store_true", help="split one 64-candidate batch across the ranks")
    p.add_argument("--mlpnp-candidates", type=int, default=128, help="config-4 candidates (sharded over the ranks)")
    p.add_argument("--cpu-threads", type=int, default=0, help="threads of the all-cores CPU baseline (0: auto)")
    p.add_argument("--no-cpu", action="store_true")
    for s in ("sim3", "mlpnp", "events", "latency", "poseopt", "bow", "sim3match", "sim3opt", "kfdb", "config1",
              "rccl-check"):
        p.add_argument(f"--no-{s}", action="store_true")
    p.add_argument("--full", action="store_true",
                   help="everything beyond the headline figure: the instrumented second pass and roofline of "
                        "config 2, the CPU baselines, the other sections (narrowed by the --no-* options) and the "
                        "world-1 RCCL check; without it the run warms up, times the steps and prints the line")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the result records and the hypotheses of the last timed config-2 step as DIR/<name>.npy")
    p.add_argument("--only-headline", action="store_true", help="config 2 only (PMC passes)")
    p.add_argument("--eig-rows-ab", action="store_true",
                   help="single-event A/B of the rows-form eigen stage (off-default variant, DESIGN.md §9)")
    p.add_argument("--dist-backend", default="nccl", choices=("nccl", "gloo"),
                   help="nccl (= RCCL over xGMI, the product path) or gloo (host collectives: lets N ranks "
                        "share fewer GPUs to rehearse the launch and gather on a 1-GPU box)")
    a = p.parse_args()
    if not a.full:  # a plain run: the headline's set-up, warm-up and timed steps only
        a.only_headline = a.no_cpu = True
    if a.only_headline:
        for s in ("sim3", "mlpnp", "events", "latency", "poseopt", "bow", "sim3match", "sim3opt", "kfdb", "config1",
                  "rccl_check"):
            setattr(a, f"no_{s}", True)
    return a


# ------------------------------------------------------------------------------------------------
# process launch and distributed setup
# ------------------------------------------------------------------------------------------------
def launch_ranks(args) -> int:
    """`bench.py --gpus N` outside torchrun: start N rank processes (RANK/LOCAL_RANK/WORLD_SIZE,
    rendezvous on 127.0.0.1) and return the worst exit status.  The parent never touches the GPU."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus),
                   LOCAL_WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    for p in procs:
        code = p.wait()
        if code != 0 and rc == 0:
            rc = code
            for q in procs:
                if q.poll() is None:
                    q.terminate()
    return rc


DEFAULT_EIG_ROWS = 64  # the library's default rows-form threshold (rsc_kernels.h kEigRowsDefaultWgs)
COLL_DEV = "cuda"  # device of the collective tensors: cuda for RCCL, cpu for gloo
RESULT_OUT = sys.stdout  # where rank 0 prints the one JSON line
RCCL1 = None  # world-1 RCCL process group (torch.distributed) for rccl_check, or the error text


def dist_setup(args):
    """One process per GPU: rank r drives GPU LOCAL_RANK.  With --dist-backend gloo the ranks may
    share GPUs (device = LOCAL_RANK mod the visible count) and the collectives run on host tensors.
    For world > 1 the process's fd 1 is pointed at stderr (the collective libraries print
    connection banners on stdout) and the JSON line goes to a saved copy of the original stdout."""
    global COLL_DEV, RESULT_OUT, RCCL1
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world == 1 and args.dist_backend == "nccl" and not args.no_rccl_check:
        # A world-1 RCCL process group, created before anything else touches the GPU, so the
        # product's collective (all_gather_into_tensor of the result records on device) executes on
        # a 1-GPU box too (rccl_check section, outside the timed regions: at N = 1 the step has no
        # exchange).  A failure is reported in the JSON line, not fatal.
        sys.stdout.flush()
        RESULT_OUT = os.fdopen(os.dup(1), "w")  # RCCL prints its banner on fd 1
        os.dup2(2, 1)
        try:
            import torch
            import torch.distributed as tdist
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(port))
            torch.cuda.set_device(local)
            tdist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", local))
            RCCL1 = tdist
        except Exception as e:  # noqa: BLE001
            RCCL1 = f"{type(e).__name__}: {e}"
    if world > 1:
        sys.stdout.flush()
        RESULT_OUT = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)
        import torch
        import torch.distributed as dist
        if args.dist_backend == "nccl":
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            local = local % max(1, torch.cuda.device_count())
            COLL_DEV = "cpu"
            dist.init_process_group("gloo")
    return world, rank, local, dist


def barrier(dist):
    if dist is not None:
        dist.barrier()


def reduce_time_and_count(dist, dt, count):
    """max over ranks of the timed region, sum of the work units."""
    if dist is None:
        return dt, count
    import torch
    t = torch.tensor([dt, float(count)], dtype=torch.float64, device=COLL_DEV)
    mx = t.clone()
    dist.all_reduce(mx[:1], op=dist.ReduceOp.MAX)
    dist.all_reduce(t[1:], op=dist.ReduceOp.SUM)
    return float(mx[0]), int(t[1])


def cpu_threads(args) -> int:
    """Threads of the all-cores CPU baseline: every CPU this process may run on
    (os.sched_getaffinity), unless --cpu-threads or OMP_NUM_THREADS (the GPU box's declared CPU
    share) set fewer; host_cpus() reports the counts beside it."""
    if args.cpu_threads > 0:
        return args.cpu_threads
    n = len(os.sched_getaffinity(0))
    env = os.environ.get("OMP_NUM_THREADS")
    if env and env.isdigit() and int(env) > 0:
        n = min(n, int(env))
    return max(1, n)


def host_cpus(threads):
    return {"nproc": os.cpu_count(), "affinity_cpus": len(os.sched_getaffinity(0)),
            "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "all_cores_threads": threads}


def median_batches(fn, warmup=3, reps=10):
    """BASELINE.md §2 timing rule: `warmup` untimed batches, then the median wall time of `reps`
    timed batches."""
    for _ in range(warmup):
        fn()
    times = []
    while len(times) < reps:
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), len(times)


def cpu_section(fn_for_threads, units_per_batch, unit, sample, threads, warmup=3, reps=10):
    """cpu_baseline object: 1 core (the reference's one-thread loop) + all cores (std::thread per
    shard of the same batch)."""
    med1, n1 = median_batches(lambda: fn_for_threads(1), warmup, reps)
    out = dict(value=round(units_per_batch / med1, 2), unit=unit, cores=1, kind="port",
               sample=f"{sample}; {warmup} warm-up + median of {n1} batches, oracle restatement, 1 thread",
               median_batch_s=round(med1, 5))
    if threads > 1:
        medn, nn = median_batches(lambda: fn_for_threads(threads), warmup, reps)
        out["all_cores"] = dict(value=round(units_per_batch / medn, 2), unit=unit, cores=threads,
                                median_batch_s=round(medn, 5),
                                sample=f"same batch, {warmup} warm-up + median of {nn}, std::thread per shard")
    return out


# ------------------------------------------------------------------------------------------------
# config 2 (headline)
# ------------------------------------------------------------------------------------------------
def run_pnp(engine, ctx, scenes, cand_ids, args, dist, rank, world):
    from rsc import workloads as wl
    solvers = [engine.PnPSolver(ctx, sc, 1) for sc in scenes]
    batch = engine.SolverBatch(solvers)
    C = len(solvers)
    gather = None
    if dist is not None:
        import torch
        from rsc import dist as rdist
        maxc = args.candidates  # fixed block per rank (strong-mode shards may differ by one)
        # one int32 payload per rank (rsc.dist.all_gather_records_and_mask's layout): the result
        # records, then the candidate of this rank that can win and its vbInliers as a bitset
        words = (max(sc.n_points for sc in scenes) + 31) // 32
        per = maxc * rdist.RECORD + 1 + words
        rec = torch.zeros(per, dtype=torch.int32, device=COLL_DEV)
        allrec = torch.zeros(world * per, dtype=torch.int32, device=COLL_DEV)
        host = np.full(per, -1, np.int32)
        hrec = host[:maxc * rdist.RECORD].view(np.float32).reshape(maxc, rdist.RECORD)
        gather = (torch, rec, allrec, host, hrec, maxc * rdist.RECORD, rdist)

    def step(s):
        if args.strong:
            seeds = wl.config2_seeds(s, 0, args.candidates)[cand_ids]
        else:
            seeds = wl.config2_seeds(s, rank, args.candidates)
        batch.reset(seeds)
        batch.set_ransac_parameters(*wl.RELOC)
        outs = batch.iterate_raw(args.iters)
        if gather is not None:
            torch, rec, allrec, host, hrec, mo, rdist = gather
            hrec[:C, 0] = cand_ids
            hrec[:C, 1], hrec[:C, 2], hrec[:C, 3], hrec[:C, 4] = (outs["ok"], outs["no_more"], outs["n_inliers"],
                                                                  outs["iterations"])
            hrec[:C, 5:21] = outs["T"].reshape(C, 16)
            ok = np.flatnonzero(outs["ok"])
            host[mo] = cand_ids[ok[0]] if len(ok) else -1  # rsc.dist.local_reloc_candidate
            host[mo + 1:] = 0
            if len(ok):  # the winner's vbInliers (exhaustive mode never has one)
                m = np.zeros((len(host) - mo - 1) * 32, np.uint8)
                v = solvers[ok[0]].last_inliers()
                m[:len(v)] = v
                host[mo + 1:] = np.packbits(m, bitorder="little").view(np.int32)
            rec.copy_(torch.from_numpy(host))
            dist.all_gather_into_tensor(allrec, rec)  # RCCL over xGMI: records + winner mask of all ranks
            if COLL_DEV == "cuda":
                torch.cuda.synchronize()
        return int(outs["iterations"].sum()), outs

    for s in range(args.warmup):
        step(s)
    # Timed region 1 (the metric): K steps, no instrumentation in the queue.
    barrier(dist)
    ctx.synchronize()
    t0 = time.perf_counter()
    hyps = 0
    for s in range(args.steps):
        n, outs = step(args.warmup + s)
        hyps += n
    ctx.synchronize()
    barrier(dist)
    dt = time.perf_counter() - t0
    last = outs.copy()  # iterate_raw returns a view of the batch's reused record buffer
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last, solvers)
    if not args.full:
        return dict(seconds=dt, hyps=hyps, problems=C * args.steps, last=last)
    # Timed region 2 (roofline): the same K steps with HIP events around the kernels on the
    # context stream (eigen stage, betas, scan); events add gaps, so this pass is not the metric.
    ctx.enable_timing(True)
    solve_ms = scan_ms = eig_ms = 0.0
    launches = 0
    t1 = time.perf_counter()
    for s in range(args.steps):
        step(args.warmup + args.steps + s)
        tm = ctx.last_timing()
        solve_ms += tm["solve_ms"]
        scan_ms += tm["scan_ms"]
        eig_ms += tm["eig_ms"]
        launches += tm["solve_launches"]
    ctx.synchronize()
    dt_inst = time.perf_counter() - t1
    ctx.enable_timing(False)
    return dict(seconds=dt, seconds_instrumented=dt_inst, hyps=hyps, problems=C * args.steps,
                solve_ms=solve_ms / max(launches, 1), scan_ms=scan_ms / max(launches, 1),
                eig_ms=eig_ms / max(launches, 1), launches=launches, last=last)


def dump_outputs(path, rec, solvers):
    """--dump-outputs: what the last timed step computed, float32, one row per candidate.  The result
    records its caller received (rsc_pnp_iterate_many): ok, no_more, n_inliers, iterations [C] (counts
    far below 2^24, exact in float32) and T [C, 16] (the record's own float32).  In exhaustive mode no
    candidate succeeds and those records are all alike, so every hypothesis of the step's last launch
    goes with them: hypothesis_inliers [C, H] and hypothesis_poses [C, H, 12] (rsc_pnp_last_hypotheses;
    rows past a candidate's own count are zero).  ~1 MB at the default shapes; with more candidates
    than 60 MB of hypotheses hold, the hypotheses of the first candidates that fit."""
    os.makedirs(path, exist_ok=True)
    out = {name: rec[name] for name in rec.dtype.names}
    per_cand = 13 * 4 * max(1, int(rec["iterations"].max()))
    hyp = [s.last_hypotheses(4096) for s in solvers[:max(1, 60_000_000 // per_cand)]]
    H = max(len(cnt) for cnt, _ in hyp)
    out["hypothesis_inliers"] = np.zeros((len(hyp), H), np.float32)
    out["hypothesis_poses"] = np.zeros((len(hyp), H, 12), np.float32)
    for c, (cnt, pos) in enumerate(hyp):
        out["hypothesis_inliers"][c, :len(cnt)] = cnt
        out["hypothesis_poses"][c, :len(cnt)] = pos
    for name, a in out.items():
        np.save(os.path.join(path, f"{name}.npy"), np.ascontiguousarray(a, np.float32))


def cpu_baseline_pnp(scenes, args, threads):
    """Oracle restatement of the same 64-candidate batch (ora_pnp_run_batch)."""
    import oracle_lib as ol
    from rsc import workloads as wl
    L = ol.lib()
    C = len(scenes)
    n = np.array([sc.n for sc in scenes], np.int32)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    p2d = np.ascontiguousarray(np.concatenate([sc.p2d for sc in scenes]), np.float32)
    p3d = np.ascontiguousarray(np.concatenate([sc.p3dw for sc in scenes]), np.float32)
    s2 = np.ascontiguousarray(np.concatenate([sc.sigma2 for sc in scenes]), np.float32)
    out_i4 = np.zeros(4 * C, np.int32)
    out_T = np.zeros(16 * C, np.float32)
    sc0 = scenes[0]
    seeds = wl.config2_seeds(0, 0, C)

    def batch(nt):
        L.ora_pnp_run_batch(C, n, off, p2d, p3d, s2, sc0.fx, sc0.fy, sc0.cx, sc0.cy, seeds, *wl.RELOC, args.iters,
                            nt, out_i4, out_T, None)
    batch(1)
    hyps = int(out_i4.reshape(C, 4)[:, 3].sum())
    return cpu_section(batch, hyps, "hypotheses/s",
                       f"full batch: {C} candidates x {sc0.n} corrs x iterate({args.iters}) = {hyps} hypotheses",
                       threads)


# ------------------------------------------------------------------------------------------------
# config 3 / 4
# ------------------------------------------------------------------------------------------------
def run_sharded(engine, ctx, batch, lo, hi, total, params, args, dist, world, steps, pack, winner=None,
                mask_len=0):
    """One sharded RANSAC section (configs 3 and 4): every rank runs candidates [lo, hi) of the
    section's `total` (seeds by global candidate index, so any world size gives the same records),
    then ONE all-gather of the fixed-size result records (RCCL over xGMI) when world > 1.  Timed
    like the headline: barrier + sync around K steps, max over ranks, hypotheses summed.

    winner = "loop" / "reloc": the all-gather also carries the vbInliers (mask_len entries) of the
    rank's candidate that can win (rsc.dist.all_gather_records_and_mask: the loop-closure winner by
    (round, candidate), LoopClosing.cpp:271-309; the relocalization winner by index,
    Tracking.cpp:1241-1284), so every rank holds the winner's mask after the step."""
    from rsc import dist as rdist
    from rsc import workloads as wl
    gather = None  # records per rank of the all-gather: the largest shard
    if dist is not None:
        import torch
        counts = torch.tensor([hi - lo], dtype=torch.int64, device=COLL_DEV)
        dist.all_reduce(counts, op=dist.ReduceOp.MAX)
        gather = max(1, int(counts.item()))
    ids = list(range(lo, hi))
    state = {"records": None}

    with_mask = gather is not None and winner is not None

    def local(s):
        batch.reset(wl.step_seeds(s, total)[lo:hi])
        batch.set_ransac_parameters(*params)
        if with_mask:  # result dicts with vbInliers of the successful candidates
            return batch.iterate(args.iters, with_masks=True)
        return batch.iterate_raw(args.iters)

    def step(s):
        h = 0
        rec = np.zeros((0, rdist.RECORD), np.float32)
        outs = None
        if batch is not None:
            outs = local(s)
            h = int(sum(o["iterations"] for o in outs)) if with_mask else int(outs["iterations"].sum())
            if gather is not None:
                rec = pack(ids, outs)
        if with_mask:
            c = rdist.local_loop_candidate(rec) if winner == "loop" else rdist.local_reloc_candidate(rec)
            m = outs[c - lo]["inliers"] if c >= 0 else None
            rec, state["masks"] = rdist.all_gather_records_and_mask(dist, rec, gather, c, m, mask_len,
                                                                    device=COLL_DEV)
        elif gather is not None:
            rec = rdist.all_gather_records(dist, rec, gather, device=COLL_DEV)
        state["records"] = rec
        return h

    for s in range(args.warmup):
        step(s)
    barrier(dist)
    ctx.synchronize()
    t0 = time.perf_counter()
    h = 0
    for s in range(steps):
        h += step(args.warmup + s)
    ctx.synchronize()
    barrier(dist)
    dt = time.perf_counter() - t0
    dt, h = reduce_time_and_count(dist, dt, h)
    # second pass (this rank's launches only, not the metric): HIP events around the solve and scan
    # kernels on the context stream
    kt = dict(solve_ms=0.0, scan_ms=0.0, launches=0, hyps=0)
    if batch is not None:
        ctx.enable_timing(True)
        for s in range(steps):
            batch.reset(wl.step_seeds(args.warmup + steps + s, total)[lo:hi])
            batch.set_ransac_parameters(*params)
            batch.iterate_raw(args.iters)
            tm = ctx.last_timing()
            kt["solve_ms"] += tm["solve_ms"]
            kt["scan_ms"] += tm["scan_ms"]
            kt["launches"] += tm["solve_launches"]
            kt["hyps"] += tm["hypotheses"]
        ctx.enable_timing(False)
    n = max(kt["launches"], 1)
    return dict(hyp_per_s=h / dt, ms_per_step=1e3 * dt / steps, hypotheses_per_step=h // steps, steps=steps,
                kernel_ms_per_launch={"solve": round(kt["solve_ms"] / n, 4), "scan": round(kt["scan_ms"] / n, 4)},
                hypotheses_per_launch=kt["hyps"] // n), state["records"]


def run_sim3(engine, ctx, pairs, args, dist=None, rank=0, world=1):
    """Config 3: 32 loop-closure KeyFrame pairs x 1000 matches, SetRansacParameters(0.99,20,300)
    (LoopClosing.cpp:261) + iterate(300), the pairs (LoopClosing.cpp:238-265's candidates) sharded
    across the ranks by cost."""
    from rsc import dist as rdist
    from rsc import workloads as wl
    C = len(pairs)
    lo, hi = rdist.shard_range(C, world, rank, [p.n1 for p in pairs])
    solvers = [engine.Sim3Solver(ctx, p, 1) for p in pairs[lo:hi]]
    batch = engine.SolverBatch(solvers) if solvers else None
    r, rec = run_sharded(engine, ctx, batch, lo, hi, C, wl.LOOP, args, dist, world, args.steps, rdist.pack_sim3,
                         winner="loop", mask_len=max(p.n1 for p in pairs))
    r.update(pairs=C, pairs_per_rank=hi - lo, correspondences=pairs[0].n1,
             sharding=f"{world} rank(s), contiguous blocks by N, RCCL all-gather of {rdist.RECORD}-float records"
                      + (" + the loop-closure winner's vbInliers (mN1 bits) in the same collective" if world > 1 else ""))
    # config 3 is scan-bound (Horn on 3 points is tiny): FP32 VALU roofline of the scan kernel with
    # SURVEY §8(d)'s F_h = 62 N flops and B_h = 48 N bytes per hypothesis
    scan_ms = r["kernel_ms_per_launch"]["scan"]
    hl = r["hypotheses_per_launch"]
    nc = float(np.mean([p.n1 for p in pairs[lo:hi]])) if hi > lo else 0.0
    if scan_ms and hl:
        tf = hl * 62 * nc / (scan_ms * 1e-3) / 1e12
        r["roofline"] = {"bound": "valu-fp32", "achieved": round(tf, 4), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(tf / FP32_PEAK_TFLOPS, 5), "traffic": None,
                         "kernel": f"sim3_scan_kernel ({hl} hypotheses x {nc:.0f} correspondences per launch)",
                         "algorithmic_flops_per_launch": round(hl * 62 * nc),
                         "effective_scan_bw_frac": round(hl * 48 * nc / (scan_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                         "sources": {"per_unit": "SURVEY.md §8(d): F_h = 62 N, B_h = 48 N", "time": "HIP events"}}
    return r, solvers, rec


def cpu_baseline_sim3(solvers, args, threads):
    """The Sim3 oracle on the solvers' prepared arrays (ctor output: camera-frame points, size_t
    thresholds, projections), SetRansacParameters(0.99,20,300) + iterate(300) per pair."""
    import oracle_lib as ol
    from rsc import workloads as wl
    L = ol.lib()
    preps = [s.prepared() for s in solvers]
    C = len(preps)
    n = np.array([len(p["indices"]) for p in preps], np.int32)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([p[k] for p in preps]), dt)
    X1, X2, P1, P2 = cat("X1c", np.float32), cat("X2c", np.float32), cat("P1im1", np.float32), cat("P2im2", np.float32)
    e1, e2 = cat("maxerr1", np.uint64), cat("maxerr2", np.uint64)
    from rsc import synth
    K = np.array([synth.FX, synth.FY, synth.CX, synth.CY], np.float32)
    seeds = wl.step_seeds(0, C)
    out_i4 = np.zeros(4 * C, np.int32)
    out_Rt = np.zeros(12 * C, np.float32)

    def batch(nt):
        L.ora_sim3_run_prepared_batch(C, n, off, X1, X2, P1, P2, e1, e2, K, K, seeds, *wl.LOOP, args.iters, nt,
                                      out_i4, out_Rt)
    batch(1)
    hyps = int(out_i4.reshape(C, 4)[:, 3].sum())
    return cpu_section(batch, hyps, "hypotheses/s",
                       f"full batch: {C} pairs x {int(n.mean())} matches x iterate({args.iters}) = {hyps} hypotheses",
                       threads)


def mlpnp_covariances(sc):
    from rsc import workloads as wl
    return wl.config4_covariances(sc)


def run_mlpnp(engine, ctx, scenes, args, with_cov=False, dist=None, rank=0, world=1):
    """Config 4: 128 candidates x 4096 correspondences sharded across the ranks (BASELINE: over 4
    MI355X; here over however many ranks run), MLPnP SetRansacParameters(0.99,10,300,6,0.5,5.991)
    (commented call Tracking.cpp:1227-1228), iterate(300), exhaustive; with_cov: computePose's
    bearing-covariance branch (covMats given)."""
    from rsc import dist as rdist
    from rsc import workloads as wl
    C = len(scenes)
    lo, hi = rdist.shard_range(C, world, rank, [sc.n for sc in scenes])
    solvers = [engine.MLPnPSolver(ctx, sc, 1) for sc in scenes[lo:hi]]
    if with_cov:
        for g, sc in zip(solvers, scenes[lo:hi]):
            g.set_covariances(mlpnp_covariances(sc))
    batch = engine.SolverBatch(solvers) if solvers else None
    r, rec = run_sharded(engine, ctx, batch, lo, hi, C, wl.MLPNP, args, dist, world, max(1, args.steps // 4),
                         rdist.pack_pnp)
    r.update(candidates=C, candidates_per_rank=hi - lo, correspondences=scenes[0].n,
             sharding=f"{world} rank(s), contiguous blocks by N, RCCL all-gather of {rdist.RECORD}-float records")
    roof = fp64_roofline("mlpnp_quad_kernel<6>" + ("<MlIndexedCov>" if with_cov else ""), r["hypotheses_per_launch"],
                         op_count("mlpnp"), r["kernel_ms_per_launch"]["solve"],
                         "MLPnP computePose on a 6-point sample")
    if roof:
        r["roofline"] = roof
    return r, rec


def cpu_baseline_mlpnp(scenes, args, threads, sample_cands=4):
    """The MLPnP oracle on a bounded sample: the first `sample_cands` candidates of the batch per
    CPU batch (the full 32 x 4096 x 300 batch is ~1 s per core-batch)."""
    import oracle_lib as ol
    from rsc import workloads as wl
    L = ol.lib()
    sub = scenes[:sample_cands]
    C = len(sub)
    n = np.array([sc.n for sc in sub], np.int32)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    p2d = np.ascontiguousarray(np.concatenate([sc.p2d for sc in sub]), np.float32)
    p3d = np.ascontiguousarray(np.concatenate([sc.p3dw for sc in sub]), np.float32)
    s2 = np.ascontiguousarray(np.concatenate([sc.sigma2 for sc in sub]), np.float32)
    seeds = wl.step_seeds(0, C)
    out_i4 = np.zeros(4 * C, np.int32)
    out_T = np.zeros(16 * C, np.float32)
    sc0 = sub[0]

    def batch(nt):
        L.ora_mlpnp_run_batch(C, n, off, p2d, p3d, s2, sc0.fx, sc0.fy, sc0.cx, sc0.cy, seeds, *wl.MLPNP,
                              args.iters, nt, out_i4, out_T)
    batch(1)
    hyps = int(out_i4.reshape(C, 4)[:, 3].sum())
    return cpu_section(batch, hyps, "hypotheses/s",
                       f"bounded sample: {C} of the {len(scenes)} candidates x {sc0.n} corrs x iterate({args.iters}) "
                       f"= {hyps} hypotheses per batch", min(threads, C))


# ------------------------------------------------------------------------------------------------
# config 5 (event stream) and single-event latency
# ------------------------------------------------------------------------------------------------
def build_event_drivers(engine, ctx, evs, ids):
    from rsc import events as rev
    groups = {"reloc": [], "loop": []}
    for i in ids:
        ev = evs[i]
        cls = engine.PnPSolver if ev.kind == "reloc" else engine.Sim3Solver
        groups[ev.kind].append((ev, [cls(ctx, x, s) for x, s in zip(rev.event_inputs(ev), ev.seeds)]))
    drivers = []
    for kind, params in (("reloc", rev.RELOC_PARAMS), ("loop", rev.LOOP_PARAMS)):
        if groups[kind]:
            eb = engine.EventBatch([g[1] for g in groups[kind]])
            seeds = np.array([s for ev, _ in groups[kind] for s in ev.seeds], np.uint32)
            drivers.append((eb, params, seeds, [ev.eid for ev, _ in groups[kind]]))
    return drivers


def run_events(engine, ctx, args, dist, rank, world):
    """Config 5: the EuRoC-MH01-shaped event stream (150 relocalization + 20 loop events, seed-fixed
    sizes), whole events sharded across ranks by cost (LPT), each event run with the reference's
    iterate(5) round-robin (rsc_reloc_events / rsc_loop_events: all candidates of all local events in
    the same launches), then ONE all-gather of the per-event winner records (RCCL over xGMI).
    A step = reset + SetRansacParameters of every candidate + both drivers + the all-gather."""
    from rsc import events as rev
    evs = rev.make_event_stream()
    shards = rev.shard_events([ev.cost for ev in evs], world)
    drivers = build_event_drivers(engine, ctx, evs, shards[rank])
    max_per_rank = max(len(p) for p in shards)

    def step():
        recs, hyps = [], 0
        for eb, params, seeds, eids in drivers:
            eb.batch.reset(seeds)
            eb.batch.set_ransac_parameters(*params)
            eb.run()
            hyps += int(eb.cand["iterations"].sum())
            recs.append(rev.pack_events(eids, eb.per_event, eb.winner_poses()))
        rec = np.concatenate(recs) if recs else np.zeros((0, rev.EVENT_RECORD), np.float32)
        if dist is not None:
            rec = rev.all_gather_events(dist, rec, max_per_rank, device=COLL_DEV)
        return hyps, rec

    for _ in range(args.warmup):
        step()
    barrier(dist)
    ctx.synchronize()
    t0 = time.perf_counter()
    hyps = 0
    for _ in range(args.steps):
        h, rec = step()
        hyps += h
    ctx.synchronize()
    barrier(dist)
    dt = time.perf_counter() - t0
    dt, hyps = reduce_time_and_count(dist, dt, hyps)
    n_ev = len(evs) * args.steps
    return dict(events_per_s=n_ev / dt, ms_per_stream=1e3 * dt / args.steps, hyp_per_s=hyps / dt,
                events=len(evs), candidates=sum(len(ev.sizes) for ev in evs),
                resolved=int((rec[:, 1] >= 0).sum()),
                sharding=f"{world} rank(s), LPT by N*300, RCCL all-gather of {rev.EVENT_RECORD}-float records"), evs


def cpu_baseline_events(evs, threads):
    """The reference-order event replay of the oracle (ora_reloc/loop_events_batch: per event, the
    solvers are built from the raw inputs, then iterate(5) rounds until a pose) over the whole stream."""
    import events_oracle as eo
    packs = [eo.PackedEvents([ev for ev in evs if ev.kind == k]) for k in ("reloc", "loop")]

    def batch(nt):
        for p in packs:
            p.run(nt)
    return cpu_section(batch, len(evs), "events/s",
                       f"the whole {len(evs)}-event stream per batch", threads, warmup=1, reps=10)


def latency_event(kind: str, seed: int = 4242):
    """One relocalization event as Tracking::Relocalization sees it: C = 15 candidates,
    N ~ U[300, 900] (mean ~600), candidate quality as the config-5 stream; or one loop event, C = 3
    pairs x N ~ U[200, 600]."""
    from rsc import events as rev
    rng = np.random.default_rng(seed)
    if kind == "reloc":
        C = 15
        sizes = [int(x) for x in rng.integers(300, 901, size=C)]
        ratios = [float(x) for x in rng.choice([0.05, 0.2, 0.6, 0.8], size=C, p=[0.5, 0.2, 0.15, 0.15])]
        return rev.Event("reloc", 100000, sizes, ratios, [7 + c for c in range(C)])
    C = 3
    sizes = [int(x) for x in rng.integers(200, 601, size=C)]
    ratios = [float(x) for x in rng.choice([0.02, 0.1, 0.3, 0.6], size=C)]
    return rev.Event("loop", 100001, sizes, ratios, [9 + c for c in range(C)])


def eig_rows_ab(ctx, eb, params, seeds, ref, reps):
    """Interleaved A/B of the eigen-stage form on the single relocalization event: lane pairs vs the
    Refine's rows form (the default for small launches since round 5, rsc_context_set_eig_rows;
    DESIGN.md §9) — same event, alternating calls; the event's outcome must not change.  Then one
    timed pass per form with HIP events (eigen stage, solve pair, Refine).  Reported beside the
    metric, never replaces gpu_ms."""
    keys = ("winner", "round", "hypothesis", "n_inliers")
    forms = {"pairs": 0, "rows": 1 << 20}
    names = list(forms)
    times = {k: [] for k in names}
    kern = {}
    same = True
    try:
        for r in range(len(names) * (reps + 5)):
            name = names[r % len(names)]
            ctx.set_eig_rows(forms[name])
            t0 = time.perf_counter()
            eb.batch.reset(seeds)
            eb.batch.set_ransac_parameters(*params)
            res = eb.run()
            t = time.perf_counter() - t0
            if r >= 5 * len(names):
                times[name].append(t)
            same = same and all(int(res[0][k]) == int(ref[k]) for k in keys)
        for name in names:
            ctx.set_eig_rows(forms[name])
            ctx.enable_timing(True)
            acc = np.zeros(3)
            for _ in range(10):
                eb.batch.reset(seeds)
                eb.batch.set_ransac_parameters(*params)
                eb.run()
                tm = ctx.last_timing()
                acc += [tm["eig_ms"], tm["solve_ms"], tm["refine_ms"]]
            ctx.enable_timing(False)
            kern[name] = {k: round(float(v) / 10, 4) for k, v in zip(("eig_ms", "solve_ms", "refine_ms"), acc)}
    except Exception as e:  # an A/B must never cost the bench line
        return dict(error=str(e)[:200])
    finally:
        ctx.enable_timing(False)
        ctx.set_eig_rows(DEFAULT_EIG_ROWS)
    out = {f"{k}_ms": round(1e3 * float(np.median(v)), 4) for k, v in times.items()}
    out.update(same_result=bool(same), reps=len(times["pairs"]), kernels=kern)
    return out


def run_latency(engine, ctx, args, with_cpu, reps=50):
    """Single-event latency: ONE rsc_reloc_events / rsc_loop_events call on one event (reset +
    SetRansacParameters + the iterate(5) round-robin, result on the host), median over reps calls;
    CPU: the oracle replay of the same event on one core."""
    from rsc import events as rev
    import events_oracle as eo
    out = {}
    for kind in ("reloc", "loop"):
        ev = latency_event(kind)
        (eb, params, seeds, _), = build_event_drivers(engine, ctx, [ev], [0])
        times = []
        for r in range(reps + 5):
            t0 = time.perf_counter()
            eb.batch.reset(seeds)
            eb.batch.set_ransac_parameters(*params)
            res = eb.run()
            t = time.perf_counter() - t0
            if r >= 5:
                times.append(t)
        pe = res[0]
        sec = dict(candidates=len(ev.sizes), mean_corrs=float(np.mean(ev.sizes)), winner=int(pe["winner"]),
                   round=int(pe["round"]), hypotheses=int(eb.cand["iterations"].sum()),
                   gpu_ms=round(1e3 * float(np.median(times)), 4), reps=reps)
        if kind == "reloc" and getattr(args, "eig_rows_ab", False):
            sec["eig_rows_ab"] = eig_rows_ab(ctx, eb, params, seeds, pe, reps)
        if with_cpu:
            pk = eo.PackedEvents([ev])
            med, n = median_batches(lambda: pk.run(1), warmup=3, reps=20)
            assert np.array_equal(pk.records()[0, 1:5], [pe["winner"], pe["round"], pe["hypothesis"], pe["n_inliers"]])
            sec["cpu_ms_1core"] = round(1e3 * med, 4)
            sec["cpu_baseline"] = dict(value=round(1e3 * med, 4), unit="ms/event", cores=1, kind="port",
                                       sample=f"the same event, 3 warm-up + median of {n}, oracle replay, 1 thread")
            sec["speedup_vs_cpu_1core"] = round(med / float(np.median(times)), 2)
        out[kind] = sec
    out.update(run_latency_gated(engine, ctx, with_cpu, reps))
    return out


def run_latency_gated(engine, ctx, with_cpu, reps=50):
    """Single-event latency of the GATED events (rsc_reloc_events_gated / rsc_loop_events_gated): the
    RANSAC round-robin plus the reference's acceptance test on the device — PoseOptimization after
    every success (Tracking.cpp:1268-1331) / SearchBySim3 + OptimizeSim3 with nInliers >= 20
    (LoopClosing.cpp:268-329) — one call per event, result on the host, median over reps calls.  The
    events are built so the first success is rejected by its gate (a candidate with wrong stereo
    matches / keypoints off their MapPoints), as in tests/test_gpu_gated.py.  CPU: the oracle replay
    of the same gated event on one core; both must agree on status, winner, round and rejections."""
    from rsc import events as rev
    from rsc import synth
    import events_oracle as eo
    out = {}
    keys = ("status", "winner", "round", "hypothesis", "rejected")
    # relocalization: C = 15 candidates sized as latency_event("reloc"), the best one poisoned
    rng = np.random.default_rng(4343)
    C = 15
    sizes = [int(x) for x in rng.integers(300, 901, size=C)]
    ratios = [float(x) for x in rng.choice([0.05, 0.2, 0.6, 0.8], size=C, p=[0.5, 0.2, 0.15, 0.15])]
    ratios[0] = 0.9
    scenes, ur, bf = synth.make_reloc_gate_event(rng, 1000, list(zip(sizes, ratios)), (0,), 0.5)
    seeds = [int(x) for x in rng.integers(1, 1 << 30, len(scenes))]
    eb = engine.EventBatch([[engine.PnPSolver(ctx, sc, s) for sc, s in zip(scenes, seeds)]])
    sd = np.array(seeds, np.uint32)
    times = []
    for r in range(reps + 5):
        t0 = time.perf_counter()
        eb.batch.reset(sd)
        eb.batch.set_ransac_parameters(*rev.RELOC_PARAMS)
        res, _, _ = eb.run_reloc_gated([(ur, bf)])
        t = time.perf_counter() - t0
        if r >= 5:
            times.append(t)
    g = res[0]
    sec = dict(candidates=C, mean_corrs=float(np.mean(sizes)), status=int(g["status"]), winner=int(g["winner"]),
               round=int(g["round"]), rejected=int(g["rejected"]), gates=int(g["gates"]),
               gpu_ms=round(1e3 * float(np.median(times)), 4), reps=reps,
               note="RANSAC round-robin + PoseOptimization gate on the device (status 1 match, 2 hand-off)")
    if with_cpu:
        o = None
        ct = []
        for r in range(3 + 10):
            t0 = time.perf_counter()
            o = eo.run_reloc_gated(scenes, seeds, ur, bf)
            if r >= 3:
                ct.append(time.perf_counter() - t0)
        assert all(int(o[k]) == int(g[k]) for k in keys), ({k: int(o[k]) for k in keys}, {k: int(g[k]) for k in keys})
        med = float(np.median(ct))
        sec["cpu_baseline"] = dict(value=round(1e3 * med, 4), unit="ms/event", cores=1, kind="port",
                                   sample=f"the same gated event, 3 warm-up + median of {len(ct)}, oracle replay, 1 thread")
        sec["speedup_vs_cpu_1core"] = round(med / float(np.median(times)), 2)
    out["reloc_gated"] = sec
    # loop closure: 3 candidate KeyFrames, the first poisoned (its Sim3 RANSAC succeeds, OptimizeSim3 fails)
    rng = np.random.default_rng(4444)
    kf1, cands = synth.make_loop_gate_event(rng, [0.9, 0.85, 0.8], poisoned=(0,))
    seeds = [int(x) for x in rng.integers(1, 1 << 30, len(cands))]
    v1 = engine.KFView(ctx, kf1)
    views, solvers, row = [v1], [], []
    for (kf2, m12, pair), s in zip(cands, seeds):
        v2 = engine.KFView(ctx, kf2)
        views.append(v2)
        solvers.append(engine.Sim3Solver(ctx, pair, s))
        row.append((v1, v2, m12))
    eb = engine.EventBatch([solvers])
    sd = np.array(seeds, np.uint32)
    times = []
    for r in range(reps + 5):
        t0 = time.perf_counter()
        eb.batch.reset(sd)
        eb.batch.set_ransac_parameters(*rev.LOOP_PARAMS)
        res, _ = eb.run_loop_gated([row])
        t = time.perf_counter() - t0
        if r >= 5:
            times.append(t)
    g = res[0]
    sec = dict(candidates=len(cands), status=int(g["status"]), winner=int(g["winner"]), round=int(g["round"]),
               rejected=int(g["rejected"]), gpu_ms=round(1e3 * float(np.median(times)), 4), reps=reps,
               note="Sim3 RANSAC round-robin + SearchBySim3(7.5) + OptimizeSim3(10), nInliers >= 20, on the device")
    if with_cpu:
        ct = []
        for r in range(3 + 10):
            t0 = time.perf_counter()
            o = eo.run_loop_gated(kf1, cands, seeds)
            if r >= 3:
                ct.append(time.perf_counter() - t0)
        assert all(int(o[k]) == int(g[k]) for k in keys), ({k: int(o[k]) for k in keys}, {k: int(g[k]) for k in keys})
        med = float(np.median(ct))
        sec["cpu_baseline"] = dict(value=round(1e3 * med, 4), unit="ms/event", cores=1, kind="port",
                                   sample=f"the same gated event, 3 warm-up + median of {len(ct)}, oracle replay, 1 thread")
        sec["speedup_vs_cpu_1core"] = round(med / float(np.median(times)), 2)
    out["loop_gated"] = sec
    return out


def run_config1(engine, ctx, with_cpu, reps=50):
    """BASELINE config 1: ONE PnPsolver::iterate(300) call at N = 500 (Tracking.cpp:1226 parameters,
    exhaustive: 40 % inliers, minInliers 250 unreachable -> 300 hypotheses).  GPU: reset +
    SetRansacParameters + iterate on the resident solver, median of `reps` calls.  CPU: the oracle's
    SetRansacParameters + iterate on a fresh solver (construction outside the clock), median of
    `reps` calls on one core.  Both must return the same result."""
    import oracle_lib as ol
    from rsc import synth
    from rsc import workloads as wl
    sc = synth.make_pnp_scene(np.random.default_rng(500), 500, 0.4)
    b = engine.SolverBatch([engine.PnPSolver(ctx, sc, 1)])
    times = []
    for r in range(reps + 5):
        t0 = time.perf_counter()
        b.reset(np.array([1], np.uint32))
        b.set_ransac_parameters(*wl.RELOC)
        out = b.iterate_raw(300)
        t = time.perf_counter() - t0
        if r >= 5:
            times.append(t)
    g = out[0]
    sec = dict(correspondences=sc.n, hypotheses=int(g["iterations"]), ok=bool(g["ok"]),
               gpu_ms=round(1e3 * float(np.median(times)), 4), reps=reps,
               note="one iterate() call: the latency a single caller sees (CPU plumbing case of BASELINE config 1)")
    if with_cpu:
        ct = []
        res = None
        for r in range(reps + 3):
            o = ol.OraclePnP(sc, 1)
            t0 = time.perf_counter()
            o.set_ransac_parameters(*wl.RELOC)
            res = o.iterate(300)
            t = time.perf_counter() - t0
            if r >= 3:
                ct.append(t)
        assert res["iterations"] == int(g["iterations"]) and bool(res["ok"]) == bool(g["ok"])
        med = float(np.median(ct))
        sec["cpu_baseline"] = dict(value=round(1e3 * med, 4), unit="ms/call", cores=1, kind="port",
                                   sample=f"the same call, 3 warm-up + median of {reps}, oracle restatement, 1 thread")
        sec["cpu_hyp_per_s_1core"] = round(int(g["iterations"]) / med, 1)
        sec["gpu_hyp_per_s"] = round(int(g["iterations"]) / float(np.median(times)), 1)
        sec["speedup_vs_cpu_1core"] = round(med / float(np.median(times)), 2)
    return sec


def rccl_check(engine, ctx, args):
    """The product's collective on THIS box at world 1: the config-2 result records of one step go
    through all_gather_into_tensor on device tensors (RCCL, backend "nccl") and must come back
    bit-equal; reports the collective's time.  Outside every timed region."""
    if args.dist_backend != "nccl" or args.no_rccl_check:
        return None
    if not hasattr(RCCL1, "all_gather_into_tensor"):
        return {"executed": False, "error": RCCL1}
    import torch
    from rsc import dist as rdist
    from rsc import workloads as wl
    scenes = wl.config2_scenes(0, 8, args.corrs)
    b = engine.SolverBatch([engine.PnPSolver(ctx, sc, 1) for sc in scenes])
    b.reset(wl.config2_seeds(0, 0, len(scenes)))
    b.set_ransac_parameters(*wl.RELOC)
    rec = rdist.pack_pnp(list(range(len(scenes))), b.iterate_raw(args.iters))
    t = torch.from_numpy(rec).cuda()
    out = torch.empty_like(t)
    times = []
    for _ in range(25):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        RCCL1.all_gather_into_tensor(out, t)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    got = out.cpu().numpy()
    # the records + winner-mask exchange (rsc.dist.all_gather_records_and_mask) on device, with a
    # parity-mode batch so that a winner exists
    ps = wl.config2_scenes(0, 8, args.corrs, ratio=0.7, seed=4242)
    sol = [engine.PnPSolver(ctx, sc, 1 + i) for i, sc in enumerate(ps)]
    b2 = engine.SolverBatch(sol)
    b2.set_ransac_parameters(*wl.RELOC)
    rec2 = rdist.pack_pnp(list(range(len(ps))), b2.iterate_raw(args.iters))
    c = rdist.local_reloc_candidate(rec2)
    mask = sol[c].last_inliers() if c >= 0 else None
    r2, m2 = rdist.all_gather_records_and_mask(RCCL1, rec2, len(ps), c, mask, ps[0].n_points, device="cuda")
    mask_ok = bool(np.array_equal(r2.view(np.uint32), rec2.view(np.uint32)) and
                   (c < 0 or (c in m2 and np.array_equal(m2[c], mask))))
    return {"executed": True, "backend": RCCL1.get_backend(), "world": RCCL1.get_world_size(),
            "records": int(rec.shape[0]), "bytes": int(rec.nbytes),
            "records_bitequal": bool(np.array_equal(got.view(np.uint32), rec.view(np.uint32))),
            "winner_mask_exchange": {"winner": int(c), "bitequal": mask_ok,
                                     "inliers": int(mask.sum()) if mask is not None else 0},
            "all_gather_us_median": round(1e6 * float(np.median(times[5:])), 2),
            "note": "all_gather_into_tensor of the config-2 result records on device, world 1 (RCCL); "
                    "multi-GPU curves come from the driver's N=2/4/8 runs"}


# ------------------------------------------------------------------------------------------------
# SURVEY §8(f) neighbours
# ------------------------------------------------------------------------------------------------
def poseopt_frames(rng, F=64, N=2000, ratio=0.8, stereo_frac=0.0):
    from rsc import synth
    return [synth.make_poseopt_frame(rng, N, ratio, stereo_frac=stereo_frac) for _ in range(F)]


def run_poseopt(engine, ctx, frames, args):
    """Optimizer::PoseOptimization (Optimizer.cpp:205-424) on a batch of Frames
    (64 x 2000 map-point matches, 80 % inliers, start pose perturbed like a RANSAC estimate), one
    rsc_pose_optimization_many call per step; kernel time from HIP events in a second pass."""
    batch = engine.PoseOptBatch(ctx, frames)

    def step():
        batch.run()

    for _ in range(args.warmup):
        step()
    ctx.synchronize()
    steps = max(1, args.steps // 2)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    ctx.synchronize()
    dt = time.perf_counter() - t0
    res = batch.results()
    ctx.enable_timing(True)
    kms = 0.0
    for _ in range(steps):
        step()
        kms += ctx.last_timing()["refine_ms"]
    ctx.enable_timing(False)
    its = sum(r["lm_iterations"] for r in res)
    trials = sum(r["lm_trials"] for r in res)
    F = len(frames)
    out = dict(poses_per_s=F * steps / dt, ms_per_step=1e3 * dt / steps, kernel_ms=kms / steps, frames=F,
               edges_per_frame=frames[0].n, lm_iterations_per_frame=its / F, lm_trials_per_frame=trials / F,
               steps=steps)
    stereo = any((getattr(f, "u_right", None) is not None and (np.asarray(f.u_right) >= 0).any()) for f in frames)
    roof = fp64_roofline("poseopt_kernel", F, op_count("poseopt" if stereo else "poseopt_mono"), kms / steps,
                         "one PoseOptimization call (one Frame)")
    if roof:
        out["roofline"] = roof
    return out


def bow_views(rng, C=64, N=2000):
    """Relocalization-shaped SearchByBoW input: the current Frame (N features) and C candidate
    KeyFrames sharing 10-70 % of its features (Tracking.cpp:1207-1214)."""
    from rsc import synth
    F = synth.make_bow_view(rng, N)
    kfs = [synth.make_bow_related(rng, F, N, float(rng.uniform(0.1, 0.7)), float(rng.uniform(0, 360)),
                                  mean_flips=float(rng.uniform(8, 30))) for _ in range(C)]
    return F, kfs


def bow_comparisons(F, kfs):
    """Descriptor comparisons the reference's SearchByBoW(pKF, F) walk can make: sum over common
    nodes of (#valid KF features) x (#Frame features) — an upper bound (matched Frame features are
    skipped)."""
    fsz = dict(zip(F.node_id.tolist(), np.diff(F.node_begin).tolist()))
    tot = 0
    for k in kfs:
        for j, nid in enumerate(k.node_id.tolist()):
            if nid in fsz:
                tot += int(k.valid[k.feat[k.node_begin[j]:k.node_begin[j + 1]]].sum()) * fsz[nid]
    return tot


def run_bow(engine, ctx, F, kfs, args):
    """ORBmatcher::SearchByBoW(pKF, F) of 64 candidate KeyFrames against the
    current Frame (2000 features each, ORBmatcher(0.75, true) as in Tracking.cpp:1212), views
    resident in HBM; one rsc_search_by_bow_frame_many per step."""
    gF = engine.BowView(ctx, F)
    gK = [engine.BowView(ctx, k) for k in kfs]
    batch = engine.BowSearch(ctx, gF, gK, True, 0.75, True)
    for _ in range(args.warmup):
        batch.run()
    ctx.synchronize()
    steps = max(1, args.steps)
    t0 = time.perf_counter()
    for _ in range(steps):
        _, nm = batch.run()
    ctx.synchronize()
    dt = time.perf_counter() - t0
    ctx.enable_timing(True)
    kms = 0.0
    for _ in range(steps):
        batch.run()
        kms += ctx.last_timing()["refine_ms"]
    ctx.enable_timing(False)
    kms /= steps
    cmp = bow_comparisons(F, kfs)
    C = len(kfs)
    # algorithmic bytes per launch: every descriptor row of both views once (32 B) + angle (4 B) +
    # FeatureVector index (4 B) + validity (1 B) per feature, + the int32 output vector
    algo = C * (F.n + kfs[0].n) * 41 + C * F.n * 4
    return dict(pairs_per_s=C * steps / dt, ms_per_step=1e3 * dt / steps, kernel_ms=kms, pairs=C,
                features=F.n, comparisons_per_pair=cmp / C, comparisons_per_s=cmp / (kms * 1e-3) if kms else None,
                mean_matches=float(np.mean(nm)), algorithmic_bytes_per_launch=algo,
                hbm_frac=(algo / (kms * 1e-3) / 1e9) / HBM_PEAK_GBS if kms else None, steps=steps)


def cpu_baseline_bow(F, kfs, seconds):
    """The SearchByBoW oracle (std::map FeatureVector walk, as the reference) on ONE host core."""
    import ctypes
    import oracle_lib as ol
    L = ol.lib()
    oF = ol.OracleBow(F)
    oK = [ol.OracleBow(k) for k in kfs]
    C = len(kfs)
    hs = (ctypes.c_void_p * C)(*[o.h for o in oK])
    out = np.zeros((C, F.n), np.int32)
    nm = np.zeros(C, np.int32)
    done = 0
    t0 = time.perf_counter()
    while True:
        L.ora_search_by_bow_many(1, C, hs, oF.h, 0.75, 1, out.reshape(-1), F.n, nm)
        done += C
        if time.perf_counter() - t0 >= seconds:
            break
    dt = time.perf_counter() - t0
    return dict(value=round(done / dt, 2), unit="pairs/s", cores=1, kind="port",
                sample=f"{done // C} batches of {C} KeyFrame x Frame searches ({F.n} features) in {dt:.1f} s, "
                       "oracle restatement, 1 thread")


def run_sim3match(engine, ctx, probs, args):
    """SURVEY §8(f) rank 3 (first half): ORBmatcher::SearchBySim3 (ORBmatcher.cpp:948-1170) on 32
    loop-closure pairs (config-3 shape: ~1000 MapPoints per KeyFrame, 30 % already matched by the
    Sim3 RANSAC), th = 7.5 as LoopClosing.cpp:309; one rsc_search_by_sim3_many per step (inputs
    packed and uploaded in the call)."""
    batch = engine.Sim3Search(ctx, probs, 7.5)
    for _ in range(args.warmup):
        batch.run()
    steps = max(1, args.steps)
    t0 = time.perf_counter()
    for _ in range(steps):
        _, nf = batch.run()
    dt = time.perf_counter() - t0
    ctx.enable_timing(True)
    kms = 0.0
    for _ in range(steps):
        batch.run()
        kms += ctx.last_timing()["refine_ms"]
    ctx.enable_timing(False)
    C = len(probs)
    pts = sum(p[0].n + p[1].n for p in probs)
    return dict(pairs_per_s=C * steps / dt, ms_per_step=1e3 * dt / steps, kernel_ms=kms / steps, pairs=C,
                points_per_pair=pts / C, mean_new_matches=float(np.mean(nf)), steps=steps)


def cpu_baseline_sim3match(probs, seconds):
    """The SearchBySim3 oracle on ONE host core over the same pairs (inputs marshalled once)."""
    import ctypes
    import oracle_lib as ol
    from rsc import engine
    L = ol.lib()
    prepared = []
    for kf1, kf2, R12, t12, m12 in probs:
        k1, keep1 = engine.sim3_kf_struct(kf1)
        k2, keep2 = engine.sim3_kf_struct(kf2)
        prepared.append((k1, k2, keep1, keep2, np.ascontiguousarray(m12, np.int32),
                         np.ascontiguousarray(np.asarray(R12, np.float32).reshape(9)),
                         np.ascontiguousarray(np.asarray(t12, np.float32).reshape(3)),
                         np.zeros(max(kf1.n, 1), np.int32)))
    done = 0
    t0 = time.perf_counter()
    while True:
        for k1, k2, _, _, m12, R, t, out in prepared:
            L.ora_search_by_sim3(ctypes.addressof(k1), ctypes.addressof(k2), m12, R, t, 7.5, out)
        done += len(probs)
        if time.perf_counter() - t0 >= seconds:
            break
    dt = time.perf_counter() - t0
    return dict(value=round(done / dt, 2), unit="pairs/s", cores=1, kind="port",
                sample=f"{done // len(probs)} batches of {len(probs)} KeyFrame pairs in {dt:.1f} s, oracle "
                       "restatement, 1 thread")


def sim3opt_problems(seed=83, pairs=32, n=1000):
    """SURVEY §8(f) rank 3 (second half): Optimizer::OptimizeSim3 on 32 loop-closure pairs (config-3
    shape: ~1000 correspondences after SearchBySim3, 25 % outliers, th2 = 10 as LoopClosing.cpp:311)."""
    from rsc import synth
    rng = np.random.default_rng(seed)
    return [synth.make_sim3opt_problem(rng, n, outlier_frac=0.25) for _ in range(pairs)]


def run_sim3opt(engine, ctx, probs, args):
    """One rsc_optimize_sim3_many per step over the 32 pairs (inputs packed and uploaded in the call,
    as the facade does); kernel time from HIP events in a second pass."""
    batch = engine.Sim3OptBatch(ctx, probs)
    for _ in range(args.warmup):
        batch.run()
    steps = max(1, args.steps // 2)
    t0 = time.perf_counter()
    for _ in range(steps):
        batch.run()
    dt = time.perf_counter() - t0
    res = batch.results()
    ctx.enable_timing(True)
    kms = 0.0
    for _ in range(steps):
        batch.run()
        kms += ctx.last_timing()["refine_ms"]
    ctx.enable_timing(False)
    C = len(probs)
    out = dict(pairs_per_s=C * steps / dt, ms_per_step=1e3 * dt / steps, kernel_ms=kms / steps, pairs=C,
               correspondences_per_pair=float(np.mean([r["n_correspondences"] for r in res])),
               mean_inliers=float(np.mean([r["n_inliers"] for r in res])),
               lm_iterations_per_pair=float(np.mean([r["lm_iterations"] for r in res])), steps=steps)
    roof = fp64_roofline("sim3opt_kernel", C, op_count("optimize_sim3"), kms / steps,
                         "one OptimizeSim3 call (one KeyFrame pair)")
    if roof:
        out["roofline"] = roof
    return out


def cpu_baseline_sim3opt(probs):
    """The OptimizeSim3 oracle on ONE host core over the same pairs."""
    import oracle_lib as ol

    def batch():
        for p in probs:
            ol.optimize_sim3(p)
    med, n = median_batches(batch, warmup=1, reps=5)
    return dict(value=round(len(probs) / med, 2), unit="pairs/s", cores=1, kind="port", median_batch_s=round(med, 5),
                sample=f"{len(probs)} pairs per batch, 1 warm-up + median of {n}, oracle restatement, 1 thread")


def kfdb_scene(seed=82, n_kfs=2000, n_queries=64, revisits=12):
    """a 2000-KeyFrame database (600-word BowVectors) built over 12 passes of
    the same places (a long EuRoC/KITTI-style map with revisits), and 64 relocalization queries
    (Frame BowVectors observed at those places): the reference returns C ~ 3-16 candidates each."""
    from rsc import synth
    rng = np.random.default_rng(seed)
    sc = synth.make_kfdb_scene(rng, n_kfs, words_per_kf=600, revisits=revisits)
    queries = [synth.make_kfdb_query(rng, sc, rng.uniform(0, sc.places - 1)) for _ in range(n_queries)]
    return sc, queries


KFDB_CAPACITY = 65537  # the facade's default (1 << 16 KeyFrames + its never-added slot)


def run_kfdb(engine, ctx, sc, queries, args):
    """KeyFrameDatabase::DetectRelocalizationCandidates (KeyFrameDatabase.cpp:174-283) as the C++
    facade runs it: a database of the facade's default capacity, and per query the covisibility
    refresh of every KeyFrame (rsc_kfdb_set_covisibility_many: unchanged rows are not uploaded)
    followed by rsc_kfdb_detect_relocalization (query upload, four kernels over the slots in use,
    candidates back); fresh Frame ids every step so every query walks the full path."""
    n = len(sc.bows)
    db = engine.KeyFrameDatabase(ctx, KFDB_CAPACITY)
    for k in range(n):
        db.add(k, *sc.bows[k])
    kfs = np.arange(n, dtype=np.int32)
    cnt = np.array([len(c) for c in sc.covis], np.int32)
    tab = np.zeros((n, 10), np.int32)
    for k, c in enumerate(sc.covis):
        tab[k, :len(c)] = c
    db.set_covisibility_table(kfs, cnt, tab)
    fid = [1]

    def step():
        nc = 0
        for ids, vals in queries:
            db.set_covisibility_table(kfs, cnt, tab)
            nc += len(db.detect_relocalization(fid[0], ids, vals))
            fid[0] += 1
        return nc
    for _ in range(args.warmup):
        step()
    steps = max(1, args.steps)
    t0 = time.perf_counter()
    nc = 0
    for _ in range(steps):
        nc += step()
    dt = time.perf_counter() - t0
    ctx.enable_timing(True)
    kms = 0.0
    for ids, vals in queries:
        db.detect_relocalization(fid[0], ids, vals)
        fid[0] += 1
        kms += ctx.last_timing()["refine_ms"]
    ctx.enable_timing(False)
    Q = len(queries)
    words = sum(len(b[0]) for b in sc.bows)
    return dict(queries_per_s=Q * steps / dt, ms_per_query=1e3 * dt / (Q * steps), kernel_ms_per_query=kms / Q,
                keyframes=n, capacity=KFDB_CAPACITY, words_per_keyframe=words / n, mean_candidates=nc / (Q * steps),
                count_kernel_bytes=4 * words, steps=steps,
                path="facade path: covisibility refresh of all KeyFrames + query, per query")


def cpu_baseline_kfdb(sc, queries, seconds):
    """The KeyFrameDatabase oracle on ONE host core, same database and queries."""
    import oracle_lib as ol
    n = len(sc.bows)
    db = ol.OracleKFDB(n)
    for k in range(n):
        db.add(k, *sc.bows[k])
        db.set_covisibility(k, sc.covis[k])
    prepared = [(np.ascontiguousarray(i, np.uint32), np.ascontiguousarray(v, np.float64)) for i, v in queries]
    done, fid = 0, 1
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for ids, vals in prepared:
            db.detect_relocalization(fid, ids, vals)
            fid += 1
        done += len(prepared)
    dt = time.perf_counter() - t0
    return dict(value=round(done / dt, 2), unit="queries/s", cores=1, kind="port",
                sample=f"{done} DetectRelocalizationCandidates queries on a {n}-KeyFrame database in {dt:.1f} s, "
                       "oracle restatement, 1 thread")


def cpu_baseline_poseopt(frames, seconds):
    """The PoseOptimization oracle on ONE host core over the same frames."""
    import oracle_lib as ol
    L = ol.lib()
    F = len(frames)
    n = np.array([f.n for f in frames], np.int64)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    uv = np.ascontiguousarray(np.concatenate([f.uv for f in frames]), np.float32)
    Xw = np.ascontiguousarray(np.concatenate([f.Xw for f in frames]), np.float32)
    inv = np.ascontiguousarray(np.concatenate([f.inv_sigma2 for f in frames]), np.float32)
    ur = (np.ascontiguousarray(np.concatenate([f.u_right for f in frames]), np.float32)
          if frames[0].u_right is not None else None)
    T = np.ascontiguousarray(np.stack([f.Tcw.reshape(16) for f in frames]), np.float32).reshape(-1)
    To = np.zeros(16 * F, np.float32)
    outl = np.zeros(int(off[-1]), np.uint8)
    good = np.zeros(F, np.int32)
    f0 = frames[0]
    done = 0
    t0 = time.perf_counter()
    while True:
        L.ora_pose_optimization_batch(F, off, uv, Xw, inv, f0.fx, f0.fy, f0.cx, f0.cy, T, To, outl, good,
                                      None if ur is None else ur.ctypes.data, float(f0.bf))
        done += F
        if time.perf_counter() - t0 >= seconds:
            break
    dt = time.perf_counter() - t0
    return dict(value=round(done / dt, 2), unit="poses/s", cores=1, kind="port",
                sample=f"{done // F} batches of {F} Frames x {f0.n} edges in {dt:.1f} s, oracle restatement, 1 thread")


def _rounded(d, nd=4):
    return {k: (round(v, nd) if isinstance(v, float) else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------
# main
# ------------------------------------------------------------------------------------------------
def headline_roofline(args, r):
    """the EPnP launch set is bound by FP64 dependency latency (not HBM, not
    MFMA): roofline = the algorithmic FP64 work of the solve kernels (S_h flops per hypothesis from
    the op-counter build of the oracle, profiles/r02/opcount.json) / their HIP-event time, against
    the FP64 vector peak; measured HBM traffic (PMC) and the effective scan bandwidth beside it."""
    per_launch_hyps = r["per_launch_hyps"]
    eig_ms, solve_ms, scan_ms = r["eig_ms"], r["solve_ms"], r["scan_ms"]
    set_ms = solve_ms + scan_ms
    B_h = 24 * args.corrs  # PnP scan bytes per hypothesis (p3D 12 + p2D 8 + maxErr 4)
    scan_bytes = per_launch_hyps * B_h
    _, opc_src = _profile_json("opcount.json")
    traffic, traffic_src = _profile_json("pmc_traffic.json")
    S_h = op_count("pnp")
    tf = per_launch_hyps * S_h / (solve_ms * 1e-3) / 1e12 if (S_h and solve_ms > 0) else None
    meas = traffic["epnp_launch_set_bytes"] if traffic else None
    # the eigen-stage form the library runs on launches of this size (rsc_api.cpp: split form unless
    # RSC_EIG_SPLIT=0; the rows form only for <= 64 workgroups)
    eig_kernel = "pnp_eig_group_kernel" if os.environ.get("RSC_EIG_SPLIT", "1") == "0" else "pnp_eig_split_kernel"
    roof = {"bound": "fp64-latency",
            "achieved": round(tf, 4) if tf else None, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(tf / FP64_PEAK_TFLOPS, 5) if tf else None,
            "traffic": round(meas) if meas else None,
            "kernel": (f"EPnP hypothesis solve: {eig_kernel}<4> + pnp_betas_kernel<4> "
                       f"({per_launch_hyps} hypotheses per launch)"),
            "algorithmic_flops_per_launch": round(per_launch_hyps * S_h) if S_h else None,
            "S_h_fp64_flops_per_hypothesis": S_h,
            "ms_per_launch": {"eig": round(eig_ms, 4), "betas": round(solve_ms - eig_ms, 4),
                              "scan": round(scan_ms, 4), "solve": round(solve_ms, 4), "set": round(set_ms, 4)},
            "launches": r["launches"],
            "hbm": {"measured_bytes_per_launch_set": round(meas) if meas else None,
                    "achieved_GBs": round(meas / (set_ms * 1e-3) / 1e9, 2) if (meas and set_ms) else None,
                    "frac": round(meas / (set_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if (meas and set_ms) else None,
                    "peak_GBs": HBM_PEAK_GBS},
            "effective_scan_bw_frac": round(scan_bytes / (set_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if set_ms else None,
            "scan_algorithmic_bytes_per_launch": scan_bytes,
            "effective_scan_bw_note": ("the scan's algorithmic bytes (every hypothesis re-reads its candidate's "
                                       "N correspondences, 24 B each; served from L2 / registers, not HBM) over "
                                       "the whole launch set's time, as a fraction of HBM peak"),
            "timing": "HIP events on the context stream, second pass of the same K steps "
                      f"({1e3 * r['seconds_instrumented'] / args.steps:.4f} ms/step with events)",
            "sources": {"S_h": f"{opc_src} (tools/opcount_report.py)",
                        "traffic": (f"{traffic_src} (2 x FETCH_SIZE + WRITE_SIZE, commit "
                                    f"{traffic.get('commit')})") if traffic else None}}
    # SURVEY.md section 8(d) "also report": the scan's FP32 fraction (F_h = 31 N FP32-equivalent flops per
    # hypothesis) over the scan kernel's time, and the achieved LDS bandwidth fraction of the launch
    # set (upper estimate: PMC SQ_INSTS_LDS x 64 lanes x 8 B, 256 CU x 128 B/clk x 2.4 GHz peak)
    F_h = 31 * args.corrs
    if scan_ms > 0:
        tf32 = per_launch_hyps * F_h / (scan_ms * 1e-3) / 1e12
        roof["scan_fp32"] = {"kernel": "pnp_scan_kernel", "achieved": round(tf32, 4), "peak": FP32_PEAK_TFLOPS,
                             "unit": "TFLOP/s", "frac": round(tf32 / FP32_PEAK_TFLOPS, 5),
                             "F_h_flops_per_hypothesis": F_h}
    lds, lds_src = _profile_json("pmc_lds.json")
    if lds and set_ms > 0:
        b = lds["lds_bytes_upper_per_launch_set"]
        roof["lds"] = {"bytes_per_launch_set_upper": round(b), "achieved_TBs": round(b / (set_ms * 1e-3) / 1e12, 4),
                       "peak_TBs": LDS_PEAK_TBS, "frac": round(b / (set_ms * 1e-3) / 1e12 / LDS_PEAK_TBS, 5),
                       "source": f"{lds_src} (SQ_INSTS_LDS x 64 lanes x 8 B, commit {lds.get('commit')})"}
    # latency roofline of the chain that bounds the eigen stage: measured clocks
    # per union QR slot of a unit's chase against the dependency-chain bound per slot
    lat, lat_src = _profile_json("latency_model.json")
    if lat:
        p = lat["probe"]
        slots = lat["union_slots_per_unit"]
        bound = lat["bound_clocks_per_unit"] / slots
        probe_clk = p["chase_us_median"] * 1e3 * p["clock_GHz"] / slots
        live_chase_us = eig_ms * 1e3 - (p["phase_A_us"] + p["phase_B_us"] + p["phase_C_us"])
        live_clk = live_chase_us * 1e3 * p["clock_GHz"] / slots
        roof["latency"] = {"kernel": f"{eig_kernel}<4> QR chase", "unit": "clocks per union QR slot",
                           "bound": round(bound, 1), "achieved_probe": round(probe_clk, 1),
                           "frac_probe": round(bound / probe_clk, 4),
                           "achieved_live": round(live_clk, 1) if live_chase_us > 0 else None,
                           "frac_live": round(bound / live_clk, 4) if live_chase_us > 0 else None,
                           "note": ("bound = make_givens chain + 2 mul-add levels per slot + the shift chain per "
                                    "sweep, spread over the slots; achieved_probe = the stamped chase median; "
                                    "achieved_live = this run's eigen-kernel time minus the probe's phases A-C"),
                           "source": lat_src}
    return roof


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    world, rank, local, dist = dist_setup(args)
    from rsc import engine
    from rsc import dist as rdist
    from rsc import workloads as wl
    ctx = engine.Context(local)
    if args.strong:
        all_scenes = wl.config2_scenes(0, args.candidates, args.corrs)
        lo, hi = rdist.shard_range(args.candidates, world, rank, [sc.n * args.iters for sc in all_scenes])
        cand_ids = np.arange(lo, hi)
        scenes = all_scenes[lo:hi]
    else:
        scenes = wl.config2_scenes(rank, args.candidates, args.corrs)
        cand_ids = np.arange(args.candidates)
    r = run_pnp(engine, ctx, scenes, cand_ids, args, dist, rank, world)
    r["per_launch_hyps"] = len(scenes) * args.iters
    dt, hyps_total = reduce_time_and_count(dist, r["seconds"], r["hyps"])
    _, problems_total = reduce_time_and_count(dist, r["seconds"], r["problems"])
    events = evs = None
    if not args.no_events:
        events, evs = run_events(engine, ctx, args, dist, rank, world)
    sections = {}
    threads = cpu_threads(args)
    with_cpu = (not args.no_cpu) and world == 1
    # configs 3 and 4: candidates sharded across the ranks (every rank runs its block)
    s3 = s3_solvers = m4 = None
    if not args.no_sim3:
        s3, s3_solvers, _ = run_sim3(engine, ctx, wl.config3_pairs(), args, dist, rank, world)
    if not args.no_mlpnp:
        sc4 = wl.config4_scenes(candidates=args.mlpnp_candidates)
        m4, _ = run_mlpnp(engine, ctx, sc4, args, False, dist, rank, world)
        m4["with_covariances"] = _rounded(run_mlpnp(engine, ctx, sc4, args, True, dist, rank, world)[0], 3)
    if rank == 0:
        if s3 is not None:
            sections["sim3"] = _rounded(s3, 3)
            if with_cpu:
                cb = cpu_baseline_sim3(s3_solvers, args, threads)
                sections["sim3"]["cpu_baseline"] = cb
                sections["sim3"]["speedup_vs_cpu_1core"] = round(s3["hyp_per_s"] / cb["value"], 1)
        if m4 is not None:
            sections["mlpnp"] = _rounded(m4, 3)
            if with_cpu:
                cb = cpu_baseline_mlpnp(sc4, args, threads)
                sections["mlpnp"]["cpu_baseline"] = cb
                sections["mlpnp"]["speedup_vs_cpu_1core"] = round(m4["hyp_per_s"] / cb["value"], 1)
        if events is not None:
            sections["events"] = _rounded(events, 3)
            if with_cpu:
                cb = cpu_baseline_events(evs, threads)
                sections["events"]["cpu_baseline"] = cb
                sections["events"]["speedup_vs_cpu_1core"] = round(events["events_per_s"] / cb["value"], 1)
        if not args.no_latency:
            sections["single_event_latency"] = run_latency(engine, ctx, args, with_cpu)
        if not args.no_config1:
            sections["config1"] = run_config1(engine, ctx, with_cpu)
        if world == 1:
            rc = rccl_check(engine, ctx, args)
            if rc is not None:
                sections["rccl_check"] = rc
        if not args.no_poseopt:
            # stereo first: the reference builds only stereo_euroc / stereo_kitti, whose Frames carry
            # mvuRight >= 0 on most slots (EdgeStereoSE3ProjectXYZOnlyPose, Optimizer.cpp:290-323)
            for name, sf in (("poseopt", 0.8), ("poseopt_mono", 0.0)):
                po_frames = poseopt_frames(np.random.default_rng(79), stereo_frac=sf)
                po = run_poseopt(engine, ctx, po_frames, args)
                po["stereo_edge_share"] = (float(np.mean([(f.u_right >= 0).mean() for f in po_frames]))
                                           if sf > 0 else 0.0)
                sections[name] = _rounded(po)
                if with_cpu:
                    cb = cpu_baseline_poseopt(po_frames, 3.0)
                    sections[name]["cpu_baseline"] = cb
                    sections[name]["speedup_vs_cpu_1core"] = round(po["poses_per_s"] / cb["value"], 1)
        if not args.no_sim3match:
            from rsc import synth
            r3 = np.random.default_rng(81)
            s3m_probs = [synth.make_sim3match_pair(r3, 1000, 250, 0.3) for _ in range(32)]
            s3m = run_sim3match(engine, ctx, s3m_probs, args)
            sections["search_by_sim3"] = _rounded(s3m, 5)
            if with_cpu:
                cb = cpu_baseline_sim3match(s3m_probs, 2.0)
                sections["search_by_sim3"]["cpu_baseline"] = cb
                sections["search_by_sim3"]["speedup_vs_cpu_1core"] = round(s3m["pairs_per_s"] / cb["value"], 1)
        if not args.no_sim3opt:
            so_probs = sim3opt_problems()
            so = run_sim3opt(engine, ctx, so_probs, args)
            sections["optimize_sim3"] = _rounded(so, 5)
            if with_cpu:
                cb = cpu_baseline_sim3opt(so_probs)
                sections["optimize_sim3"]["cpu_baseline"] = cb
                sections["optimize_sim3"]["speedup_vs_cpu_1core"] = round(so["pairs_per_s"] / cb["value"], 1)
        if not args.no_kfdb:
            kfdb_sc, kfdb_q = kfdb_scene()
            kf = run_kfdb(engine, ctx, kfdb_sc, kfdb_q, args)
            sections["kfdb_relocalization"] = _rounded(kf, 5)
            if with_cpu:
                cb = cpu_baseline_kfdb(kfdb_sc, kfdb_q, 2.0)
                sections["kfdb_relocalization"]["cpu_baseline"] = cb
                sections["kfdb_relocalization"]["speedup_vs_cpu_1core"] = round(kf["queries_per_s"] / cb["value"], 1)
        if not args.no_bow:
            bow_F, bow_K = bow_views(np.random.default_rng(80))
            bw = run_bow(engine, ctx, bow_F, bow_K, args)
            sections["search_by_bow"] = _rounded(bw, 5)
            if with_cpu:
                cb = cpu_baseline_bow(bow_F, bow_K, 3.0)
                sections["search_by_bow"]["cpu_baseline"] = cb
                sections["search_by_bow"]["speedup_vs_cpu_1core"] = round(bw["pairs_per_s"] / cb["value"], 1)
    if rank != 0:
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    value = hyps_total / dt
    if world > 1:
        par = (f"{'strong' if args.strong else 'weak'}: candidates sharded over {world} ranks "
               f"({'64 total' if args.strong else f'{args.candidates} per GPU'}), {args.dist_backend} "
               f"all-gather of {rdist.RECORD}-float result records per step")
    else:
        par = ("single GPU, one rank: no exchange in the step (the all-gather of result records runs "
               "only at N > 1; the world-1 RCCL check is outside the timed region)")
    out = {
        "metric": "RANSAC hypotheses/sec (EPnP relocalization batch, 2k corrs x 64 candidates)",
        "value": round(value, 1),
        "unit": "hypotheses/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1e3 * dt / args.steps, 4),
        "higher_is_better": True,
        "scaling": "strong" if args.strong else "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic (seeded EuRoC-shaped scenes; no dataset)",
        "config": {"workload": "config 2 reloc_pnp: candidates x correspondences, iterate(300), exhaustive "
                               "(40% inliers)",
                   "candidates": args.candidates if args.strong else args.candidates * world,
                   "candidates_per_gpu": len(scenes), "correspondences": args.corrs,
                   "hypotheses_per_candidate": args.iters, "params": "SetRansacParameters(0.99,10,300,4,0.5,5.991)",
                   "parallelism": par},
        "poses_per_s": round(problems_total / dt, 2),
    }
    if args.full:
        out["roofline"] = headline_roofline(args, r)
    if with_cpu:
        cb = cpu_baseline_pnp(scenes, args, threads)
        cb["host"] = host_cpus(threads)
        out["cpu_baseline"] = cb
        out["speedup_vs_cpu_1core"] = round(value / cb["value"], 1)
        if "all_cores" in cb:
            out["speedup_vs_cpu_all_cores"] = round(value / cb["all_cores"]["value"], 1)
        if "sim3" in sections and "cpu_baseline" in sections["sim3"]:
            # north_star: ">= 10x the reference CPU PnP+Sim3 RANSAC throughput" — the combined figure
            g = value + sections["sim3"]["hyp_per_s"]
            c = cb["value"] + sections["sim3"]["cpu_baseline"]["value"]
            out["pnp_plus_sim3"] = {"gpu_hyp_per_s": round(g, 1), "cpu_1core_hyp_per_s": round(c, 1),
                                    "speedup_vs_cpu_1core": round(g / c, 1),
                                    "note": "sum of the config-2 and config-3 rates (same unit, each on its own batch)"}
    out.update(sections)
    print(json.dumps(out), file=RESULT_OUT, flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    elif hasattr(RCCL1, "destroy_process_group"):
        RCCL1.destroy_process_group()


if __name__ == "__main__":
    main()
