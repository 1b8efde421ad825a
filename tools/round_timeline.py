#!/usr/bin/env python3
"""Per-step timeline of the headline PnP round from a rocprofv3 kernel_trace.csv of
`bench.py --gpus 1 --steps K --warmup W`: the round's kernels in stream order, the idle gap in
front of each (previous kernel's end -> this kernel's start) and the time from the round's last
kernel to the next round's first one (host replay + descriptor build + launch).  A round is
recognised by its scan launch (pnp_scan_kernel) and reaches back to the kernel that follows the
previous round's scan.  Medians over the rounds whose kernel sequence is the most common one.
usage: round_timeline.py kernel_trace.csv [out.md]"""
import csv
import re
import statistics as st
import sys
from collections import Counter


def short(n):
    n = n.replace("(anonymous namespace)::", "").replace("void ", "").replace("rsc::", "")
    return re.sub(r"\(.*", "", n).strip()


rows = []
for r in csv.DictReader(open(sys.argv[1])):
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]),
                 int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))))
rows.sort()
rounds, cur = [], []
for k in rows:
    cur.append(k)
    if k[2].startswith("pnp_scan_kernel"):
        rounds.append(cur)
        cur = []
seqs = Counter(tuple((k[2], k[3]) for k in r) for r in rounds)
seq, n = seqs.most_common(1)[0]
sel = [i for i, r in enumerate(rounds) if tuple((k[2], k[3]) for k in r) == seq]
out = open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout
med = lambda v: round(st.median(v) / 1e3, 2)
print(f"{n} rounds of {len(rounds)} with the sequence below (microseconds, medians)\n", file=out)
print("| kernel | workgroups | gap before | duration |", file=out)
print("|---|---|---|---|", file=out)
tot_k = tot_g = 0.0
for j, (name, wgs) in enumerate(seq):
    dur = med([rounds[i][j][1] - rounds[i][j][0] for i in sel])
    gap = med([rounds[i][j][0] - rounds[i][j - 1][1] for i in sel]) if j else 0.0
    tot_k += dur
    tot_g += gap
    print(f"| {name} | {wgs} | {gap if j else ''} | {dur} |", file=out)
nxt = [rounds[i + 1][0][0] - rounds[i][-1][1] for i in sel if i + 1 < len(rounds) and i + 1 in set(sel)]
per = [rounds[i + 1][0][0] - rounds[i][0][0] for i in sel if i + 1 < len(rounds) and i + 1 in set(sel)]
print(f"\nkernels {round(tot_k, 2)}, gaps inside the round {round(tot_g, 2)}, "
      f"last kernel -> next round's first kernel {med(nxt) if nxt else 'n/a'}, "
      f"round period {med(per) if per else 'n/a'}", file=out)
