"""The loop-closing matcher kernels (kfproj.hip) run without a private segment: the rounds of
kfproj_kernel are a chain of dependent LDS / L2 accesses, and a stack round trip inside them, or inside the
per-pair window walk of kffuse_kernel, would add to every step.  Reads the gfx950 code object inside
librsc.so as tests/test_cpu_kernel_resources.py does (no GPU needed)."""
from test_cpu_kernel_resources import _kernels


def test_kfproj_kernels_have_no_scratch():
    ks = _kernels()
    hits = [n for n in ks if "kfproj_kernel" in n or "kfproj_setup_kernel" in n or "kffuse_kernel" in n]
    assert len(hits) == 3, f"kfproj kernels in librsc.so: {hits}"
    for n in hits:
        k = ks[n]
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, n
        assert k[".group_segment_fixed_size"] <= 64 * 1024, (n, k[".group_segment_fixed_size"])
