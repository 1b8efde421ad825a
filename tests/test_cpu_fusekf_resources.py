"""The KeyFrame Fuse kernel (fusekf.hip) runs without a private segment, without spills and without LDS: every
(point, KeyFrame) pair is a chain of dependent L2 reads, and a stack round trip inside the window walk would add to
every feature.  Reads the gfx950 code object inside librsc.so as tests/test_cpu_kernel_resources.py does (no GPU
needed)."""
from test_cpu_kernel_resources import _kernels


def test_fusekf_kernel_has_no_scratch_and_no_lds():
    ks = _kernels()
    hits = [n for n in ks if "fusekf_kernel" in n]
    assert len(hits) == 1, f"fusekf kernels in librsc.so: {hits}"
    k = ks[hits[0]]
    assert k[".private_segment_fixed_size"] == 0, k[".private_segment_fixed_size"]
    assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0
    assert k[".group_segment_fixed_size"] == 0, k[".group_segment_fixed_size"]
