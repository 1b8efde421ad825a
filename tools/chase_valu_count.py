#!/usr/bin/env python3
"""Static VALU counts of the QR chase loop of a compiled kernel.

usage: chase_valu_count.py kernels.s [kernel-symbol-substring]

kernels.s is the device assembly of csrc/kernels.hip (the Makefile's HIPFLAGS plus
`--cuda-device-only -S`).  The chase loop of tridiag_qr is recognised as the outermost loop of the
kernel (default: pnp_eig_split_kernel<4>) that holds the most v_rsq_f64: one in the Wilkinson
shift's hypot and one per rotation slot.  A rotation slot is the straight-line code between a
`s_cbranch_execz .L` range guard and its target label that holds exactly one v_rsq_f64.  Printed:
the VALU instructions of a QR step before the first slot (in text order, i.e. the path a wave takes
when it skips the cold blocks), those of the cold blocks placed behind the loop's latch, per slot,
and after the last slot (publish, mirror stores); the LDS instructions of the same parts.
"""
import re
import sys


def function_body(lines, sym):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(sym) + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def main():
    path = sys.argv[1]
    sym = sys.argv[2] if len(sys.argv) > 2 else "pnp_eig_split_kernelILi4"
    body = function_body(open(path).read().splitlines(), sym)
    # depth-1 loops from the assembly printer's block comments
    loops = {}  # header label -> list of line indices of its blocks' lines
    cur = None
    for i, l in enumerate(body):
        m = re.match(r"^\.(LBB\d+_\d+):\s*;\s*(.*)", l)
        if m:
            label, note = m.groups()
            if "This Loop Header: Depth=1" in note:
                cur = label[1:]
            elif "Depth=1" in note and "Header=" in note:
                cur = re.search(r"Header=(BB\d+_\d+)", note).group(1)
            elif "Parent Loop" in note or "Depth=2" in note or "Depth=3" in note:
                pass  # inner loop: stays with the current depth-1 loop
            else:
                cur = None
        elif re.match(r"^\.LBB\d+_\d+:", l):
            cur = None
        if cur:
            loops.setdefault(cur, []).append(i)
    if not loops:
        sys.exit("no loops found")
    chase = max(loops.values(), key=lambda idx: sum("v_rsq_f64" in body[i] for i in idx))
    lo, hi = chase[0], chase[-1]
    text = body[lo:hi + 1]

    def is_valu(l):
        return re.match(r"^\s+v_", l) is not None

    def is_lds(l):
        return re.match(r"^\s+ds_", l) is not None

    # rotation slots
    slots = []  # (branch line, label line)
    for i, l in enumerate(text):
        m = re.match(r"^\s+s_cbranch_execz\s+\.(LBB\d+_\d+)", l)
        if not m:
            continue
        tgt = "." + m.group(1) + ":"
        j = i + 1
        while j < len(text) and not text[j].startswith(".LBB"):
            j += 1
        if j < len(text) and text[j].startswith(tgt) and sum("v_rsq_f64" in x for x in text[i:j]) == 1:
            slots.append((i, j))
    if not slots:
        sys.exit("no rotation slots found")
    first, last = slots[0][0], slots[-1][1]
    # inner (depth-2) loops and cold blocks behind the latch: blocks after the last slot that end in
    # an unconditional branch back into the part before the first slot
    depth2 = [i for i, l in enumerate(text) if re.match(r"^\.LBB\d+_\d+:.*(Depth=2|Parent Loop)", l)]
    labels = {re.match(r"^\.(LBB\d+_\d+):", l).group(1): i for i, l in enumerate(text) if l.startswith(".LBB")}
    cold = []
    starts = sorted(labels.values())
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(text)
        if s < last:
            continue
        br = [re.match(r"^\s+s_branch\s+\.(LBB\d+_\d+)", x) for x in text[s:e]]
        br = [b.group(1) for b in br if b]
        if br and br[-1] in labels and labels[br[-1]] < first:
            cold.append((s, e))
    cold_lines = {i for s, e in cold for i in range(s, e)}

    def is_cmp(l):
        return re.match(r"^\s+v_cmp", l) is not None

    def is_cbranch(l):
        return re.match(r"^\s+s_cbranch", l) is not None

    def count(rng, pred):
        return sum(pred(text[i]) for i in rng)

    top = range(0, first)
    tail = [i for i in range(last, len(text)) if i not in cold_lines]
    per_slot_v = [count(range(a, b), is_valu) for a, b in slots]
    per_slot_l = [count(range(a, b), is_lds) for a, b in slots]
    print(f"kernel {sym}: chase loop of {len(text)} lines, {len(slots)} rotation slots")
    print(f"VALU before the first slot (a QR step's bookkeeping and shift): {count(top, is_valu)}")
    print(f"  of which v_cndmask_b32: {count(top, lambda l: 'v_cndmask_b32' in l)}, v_cmp*: {count(top, is_cmp)}")
    print(f"VALU in cold blocks behind the latch (skipped unless a lane needs them): {count(sorted(cold_lines), is_valu)}")
    print(f"VALU per rotation slot: min {min(per_slot_v)} max {max(per_slot_v)} (slots: {' '.join(map(str, per_slot_v))})")
    print(f"VALU after the last slot (publish, wait, stores): {count(tail, is_valu)}")
    print(f"LDS instructions: before the first slot {count(top, is_lds)}, per slot max {max(per_slot_l)}, after the last slot {count(tail, is_lds)}")
    print(f"branches (s_cbranch*) before the first slot: {count(top, is_cbranch)}")


if __name__ == "__main__":
    main()
