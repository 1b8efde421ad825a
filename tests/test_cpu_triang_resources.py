"""The triangulation kernels (triang.hip) run without a private segment and without spills: the candidate loop of
tri_match_kernel and the register-resident 4x4 Jacobi of tri_pairs_kernel would pay a stack round trip per step.
Reads the gfx950 code object inside librsc.so as tests/test_cpu_kernel_resources.py does (no GPU needed)."""
from test_cpu_kernel_resources import _kernels


def test_triang_kernels_have_no_scratch():
    ks = _kernels()
    want = ("tri_join_kernel", "tri_match_kernel", "tri_finish_kernel", "tri_pairs_kernel")
    hits = [n for n in ks if any(w in n for w in want)]
    assert len(hits) == 4, f"triangulation kernels in librsc.so: {hits}"
    for n in hits:
        k = ks[n]
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, n
        assert k[".group_segment_fixed_size"] <= 64 * 1024, (n, k[".group_segment_fixed_size"])
