#!/usr/bin/env python3
"""Which exits of g2o's Levenberg-Marquardt loop do the GPU parity tests of the two optimisers reach?

Runs every problem that tests/test_gpu_poseopt.py and tests/test_gpu_sim3opt.py build (their check()
is replaced by a recorder, so nothing runs on a GPU) and every case of tests/lm_edge_cases.py through
the oracle with its LM branch record (oracle/lm_branches.h) and prints the totals as the Markdown
table of DESIGN.md §2.3.  CPU only:  python tools/lm_branch_table.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "orb-slam2-optimized_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import lm_edge_cases as lc  # noqa: E402
import oracle_lib as ol  # noqa: E402

FIELDS = ol.LM_BRANCH_FIELDS


class Tally:
    def __init__(self, name):
        self.name, self.problems, self.iterations = name, 0, 0
        self.br = dict.fromkeys(FIELDS, 0)
        self.not_ok2_cases = []

    def add(self, br, iterations, label=None):
        self.problems += 1
        self.iterations += int(iterations)
        for k in FIELDS:
            self.br[k] += br[k]
        if label and br["not_ok2"]:
            self.not_ok2_cases.append(f"{label} ({br['not_ok2']})")


def pose_recorder(tally):
    def check(frames):
        res = []
        for f in frames:
            r, T, out, st, br = ol.pose_optimization_branches(f)
            tally.add(br, st[1])
            res.append({"n_good": r, "Tcw": T, "outlier": out})
        return res
    return check


def sim3_recorder(tally):
    def check(problems, c=None):
        res = []
        for p in problems:
            r, S, keep, st, br = ol.optimize_sim3_branches(p)
            tally.add(br, st[2])
            res.append({"n_inliers": r, "n_bad": int(st[1]), "S": S, "keep": keep})
        return res
    return check


class NoContext:
    def set_sim3opt_helpers(self, helpers):
        pass


def run_module(mod, recorder):
    mod.check = recorder
    for name in sorted(n for n in dir(mod) if n.startswith("test_")):
        fn = getattr(mod, name)
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        args = fn.__code__.co_varnames[:fn.__code__.co_argcount]
        kw = {"form_ctx": NoContext()} if "form_ctx" in args else {}
        if marks:
            for v in marks[0].args[1]:
                fn(**kw, **{marks[0].args[0]: v})
        else:
            fn(**kw)


def main():
    import test_gpu_poseopt
    import test_gpu_sim3opt
    old_p, old_s = Tally("PoseOptimization, test_gpu_poseopt.py"), Tally("OptimizeSim3, test_gpu_sim3opt.py")
    run_module(test_gpu_poseopt, pose_recorder(old_p))
    run_module(test_gpu_sim3opt, sim3_recorder(old_s))
    new_p, new_s = Tally("PoseOptimization, lm_edge_cases.py"), Tally("OptimizeSim3, lm_edge_cases.py")
    for c in lc.pose_cases_c() + lc.pose_cases_d():
        *_, st, br = ol.pose_optimization_branches(c.problem)
        new_p.add(br, st[1], c.name)
    for c in lc.sim3_cases_c() + lc.sim3_cases_d():
        *_, st, br = ol.optimize_sim3_branches(c.problem)
        new_s.add(br, st[2], c.name)
    head = ["inputs", "problems", "LM iterations", "trials", "LDLT not positive", "`tempChi` NaN/Inf", "`rho` NaN",
            "rejected", "`qmax==10`", "`rho==0`", "`nBadLM>=3`", "no active edge", "`currentChi` NaN/Inf",
            "`!ok2` accepted"]
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    for t in (old_p, old_s, new_p, new_s):
        row = [t.name, t.problems, t.iterations] + [t.br[k] for k in FIELDS]
        print("| " + " | ".join(str(v) for v in row) + " |")
    for t in (new_p, new_s):
        print(f"\n`!ok2` trials, {t.name}: " + ", ".join(t.not_ok2_cases))


if __name__ == "__main__":
    main()
