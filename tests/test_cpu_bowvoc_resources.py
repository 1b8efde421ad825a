"""The vocabulary-transform kernels (bowvoc.hip) run without a private segment: the descent is a chain of
dependent LDS / L2 gathers and the build a chain of LDS sort steps, and a stack round trip inside either
would add to every step.  The build kernel's LDS is the sort keys of one view (8192 x (4 + 2) bytes +
scan words); the descent's staged levels are dynamic LDS, bounded by the host (kVocLdsBudgetMax, 48 KiB),
so its static segment is empty.  Reads the gfx950 code object inside librsc.so as
tests/test_cpu_kernel_resources.py does (no GPU needed)."""
from test_cpu_kernel_resources import _kernels

BUILD_LDS_BUDGET = 8192 * 6 + 256   # the keys + the scan words and the norm
STATIC_LDS = {"voc_descend_kernel": 0, "voc_build_kernel": BUILD_LDS_BUDGET, "voc_gather_kernel": 0}


def test_bowvoc_kernels_have_no_scratch():
    ks = _kernels()
    hits = [n for n in ks if any(f in n for f in STATIC_LDS)]
    assert len(hits) == 4, f"vocabulary kernels in librsc.so: {hits}"  # the descent in two subgroup widths
    for n in hits:
        k = ks[n]
        budget = next(v for f, v in STATIC_LDS.items() if f in n)
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, n
        assert not k.get(".uses_dynamic_stack", False), n
        assert k[".group_segment_fixed_size"] <= budget, (n, k[".group_segment_fixed_size"])


def test_staging_budget_constants():
    """The host bounds the descent's dynamic LDS: default and maximum budget 48 KiB, 40 B per node."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "orb-slam2-optimized_amd", "csrc", "rsc_bowvoc.h")).read()
    consts = {m[0]: eval(m[1]) for m in re.findall(r"constexpr int (kVoc\w+) = ([0-9* ]+);", txt)}
    assert consts["kVocLdsBudgetMax"] <= 64 * 1024 and consts["kVocLdsBudgetDefault"] <= consts["kVocLdsBudgetMax"]
    assert consts["kVocLdsNodeBytes"] == 40 and 1111 * 40 <= consts["kVocLdsBudgetDefault"]
