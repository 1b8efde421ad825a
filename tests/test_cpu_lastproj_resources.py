"""The last-frame SearchByProjection kernels (lastproj.hip) run without a private segment: the rounds of
lastproj_kernel are a chain of dependent LDS / L2 accesses, and a stack round trip inside them, or inside the
window walk of lastproj_setup_kernel, would add to every step.  Reads the gfx950 code object inside
librsc.so as tests/test_cpu_kernel_resources.py does (no GPU needed)."""
from test_cpu_kernel_resources import _kernels


def test_lastproj_kernels_have_no_scratch():
    ks = _kernels()
    hits = [n for n in ks if "lastproj_kernel" in n or "lastproj_setup_kernel" in n]
    assert len(hits) == 2, f"lastproj kernels in librsc.so: {hits}"
    for n in hits:
        k = ks[n]
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, n
        assert k[".group_segment_fixed_size"] <= 64 * 1024, (n, k[".group_segment_fixed_size"])
