"""Resources of the PnP round's kernels as built (no GPU needed), from the compiler's kernel-resource
remarks the Makefile keeps beside kernels.o (lib/kernels.resources.txt): every instantiation — the blob
path's (records in HBM, `NoRoundArgs`) and the argument path's (records by value, `RoundArgs` /
`SelArgs`) — has no more scratch and no fewer waves per SIMD than the kernel had at the commit before
the argument path (PARENT below, the same remarks of that commit's kernels.hip).  A record read from
the argument block with a wave-uniform index must stay a scalar load from the kernel-argument segment:
a private copy of the 1.5 KB block would show up here as scratch.

The chase of the eigen stage is sensitive to register allocation (a different allocation once made the
unchanged chase 1.5 us slower), so the VGPR / AGPR counts are recorded as well: PARENT holds the parent
commit's, and the test prints the built ones next to them (pytest -s)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REMARKS = os.path.join(ROOT, "orb-slam2-optimized_amd", "lib", "kernels.resources.txt")

# kernel<first template argument> at the parent commit: (scratch bytes/lane, waves/SIMD, VGPRs, AGPRs)
PARENT = {
    "pnp_betas_kernel<4": (0, 1, 248, 0), "pnp_betas_kernel<5": (0, 1, 248, 0), "pnp_betas_kernel<6": (0, 1, 248, 0),
    "pnp_eig_group_kernel<4": (0, 1, 256, 42), "pnp_eig_group_kernel<5": (0, 1, 256, 108),
    "pnp_eig_group_kernel<6": (0, 1, 256, 180),
    "pnp_eig_rows_kernel<4": (0, 1, 256, 42), "pnp_eig_rows_kernel<5": (0, 1, 256, 104),
    "pnp_eig_rows_kernel<6": (0, 1, 256, 180),
    "pnp_eig_split_kernel<4": (40, 2, 256, 0), "pnp_eig_split_kernel<5": (152, 2, 256, 0),
    "pnp_eig_split_kernel<6": (296, 2, 256, 0),
    "pnp_scan_kernel<1": (0, 8, 36, 0), "pnp_scan_kernel<2": (0, 8, 48, 0), "pnp_scan_kernel<4": (0, 8, 64, 0),
    "pnp_scan_kernel<8": (0, 5, 90, 0), "pnp_scan_kernel<16": (0, 3, 136, 0), "pnp_scan_kernel<32": (0, 1, 256, 220),
    "pnp_select_refine_kernel": (0, 1, 256, 2),
    "pnp_refine_kernel": (0, 1, 256, 1),
}
# instantiations each PARENT kernel has now (second template argument; the Refine kernel has none)
FORMS = {"pnp_select_refine_kernel": ("NoRoundArgs", "SelArgs"), "pnp_refine_kernel": (None,)}
ROUND_FORMS = ("NoRoundArgs", "RoundArgs")


def _demangle(names):
    import subprocess
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def _built():
    if not os.path.exists(REMARKS):
        pytest.fail(f"{REMARKS} not found: run make (the kernels.o rule writes it)")
    kernels, cur = {}, None
    for line in open(REMARKS):
        m = re.search(r"remark: (.*) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            cur = kernels.setdefault(text.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in text:
            k, v = text.rsplit(":", 1)
            cur[k.strip()] = v.strip()
    names = _demangle(list(kernels))
    out = {}
    for mangled, d in kernels.items():
        n = names[mangled].replace("void ", "").replace("rsc::", "")
        n = n[:n.index("(")] if "(" in n and not n.startswith("(") else n
        out[n] = (int(d["ScratchSize [bytes/lane]"]), int(d["Occupancy [waves/SIMD]"]), int(d["VGPRs"]), int(d["AGPRs"]))
    return out


def test_no_pnp_kernel_gains_scratch_or_loses_occupancy():
    built = _built()
    seen = 0
    for key, parent in sorted(PARENT.items()):
        forms = FORMS.get(key, ROUND_FORMS)
        for form in forms:
            if form is None:
                name = key
            elif "<" in key:
                name = f"{key}, {form}>"
            else:
                name = f"{key}<{form}>"
            assert name in built, f"{name} not among the built kernels: {sorted(k for k in built if key.split('<')[0] in k)}"
            scratch, occ, vgpr, agpr = built[name]
            print(f"{name}: scratch {scratch} (parent {parent[0]}), waves/SIMD {occ} (parent {parent[1]}), "
                  f"VGPRs {vgpr} + AGPRs {agpr} (parent {parent[2]} + {parent[3]})")
            assert scratch <= parent[0], f"{name}: scratch {scratch} bytes/lane, parent {parent[0]}"
            assert occ >= parent[1], f"{name}: {occ} waves/SIMD, parent {parent[1]}"
            seen += 1
    # 18 round kernels in two forms, the select / refine kernel in two, the Refine kernel
    assert seen == 18 * 2 + 2 + 1
