"""The PnP scan's two-segment counting, checked without a GPU.

* The continue rule (rsc_scanbound.h scan_continue / scan_seg_a_points) as the host program
  tests/cpp/scan_bound_test.cpp runs it, built by the Makefile: every N in 1..1100 with PPT = ppt_for(N)
  and its doubles up to 32, every min_inliers in 1..N, every c1 in 0..kA.  The rule rejects exactly when
  c1 + max(0, N - kA) < min_inliers, never continues when kA >= N, and with the bound off continues exactly
  when segment B has points.  Once in the plain build and once under the host sanitizers.
* The compiler's resource remarks of every pnp_scan_kernel instantiation (lib/kernels.resources.txt)
  against the parent commit's (profiles/r31/parent_scan_resources.txt, the same remarks of the parent's
  build): no scratch, and no fewer waves per SIMD."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "orb-slam2-optimized_amd", "lib")
BUILT = os.path.join(LIB, "kernels.resources.txt")
PARENT = os.path.join(ROOT, "profiles", "r31", "parent_scan_resources.txt")


@pytest.mark.parametrize("prog", ["scan_bound_test", "scan_bound_test_san"])
def test_continue_rule_over_every_case(prog):
    path = os.path.join(LIB, prog)
    assert os.path.exists(path), f"{path} not built: run make"
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert r.returncode == 0, (out, r.stderr[-2000:])
    assert out["mismatches"] == 0 and out["empty_b_continued"] == 0 and out["ka_wrong"] == 0 and out["off_wrong"] == 0
    # sum over N and PPT of N (kA + 1) cases, and both outcomes occur
    assert out["cases"] > 10**9 and out["continued"] > 0 and out["rejected"] > 0
    assert out["continued"] + out["rejected"] == out["cases"]


def _remarks(path):
    """{(PPT, form): {remark: value}} of the pnp_scan_kernel instantiations in a remarks file."""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: (.*) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            k = re.search(r"pnp_scan_kernelILi(\d+)ENS_\d+(RoundArgs|NoRoundArgs)E", text)
            cur = out.setdefault((int(k.group(1)), k.group(2)), {}) if k else None
        elif cur is not None and ":" in text:
            k, v = text.rsplit(":", 1)
            cur[k.strip()] = int(v) if v.strip().lstrip("-").isdigit() else v.strip()
    return out


def test_scan_kernel_resources_against_the_parent():
    assert os.path.exists(BUILT), f"{BUILT} not found: run make (the kernels.o rule writes it)"
    built, parent = _remarks(BUILT), _remarks(PARENT)
    want = {(p, f) for p in (1, 2, 4, 8, 16, 32) for f in ("RoundArgs", "NoRoundArgs")}
    assert set(parent) == want and set(built) == want, (sorted(parent), sorted(built))
    for key in sorted(want):
        b, p = built[key], parent[key]
        print(f"pnp_scan_kernel<{key[0]}, {key[1]}>: scratch {b['ScratchSize [bytes/lane]']}, waves/SIMD "
              f"{b['Occupancy [waves/SIMD]']} (parent {p['Occupancy [waves/SIMD]']}), VGPRs {b['VGPRs']} "
              f"(parent {p['VGPRs']}), SGPRs {b['TotalSGPRs']} (parent {p['TotalSGPRs']})")
        assert b["ScratchSize [bytes/lane]"] == 0, key
        assert b["Occupancy [waves/SIMD]"] >= p["Occupancy [waves/SIMD]"], key
