"""The two MapPoint-update kernels (mpupdate.hip) run without a private segment and without spills, and their LDS
stays within the 32 KB that hold the descriptors of the longest list (RSC_MPUPDATE_MAX_OBS = 1,024 of 32 bytes): a
row's median comes from a bisection over the staged descriptors, so a lane keeps no row of distances.  Reads the
gfx950 code object inside librsc.so as tests/test_cpu_kernel_resources.py does (no GPU needed)."""
from test_cpu_kernel_resources import _kernels


def test_mpupdate_kernels_have_no_scratch_and_bounded_lds():
    ks = _kernels()
    hits = [n for frag in ("mpupdate_block_kernel", "mpupdate_wave_kernel") for n in ks if frag in n]
    assert len(hits) == 2 and len([n for n in ks if "mpupdate_" in n]) == 2, f"mpupdate kernels in librsc.so: {hits}"
    for n in hits:
        k = ks[n]
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, n
        assert k[".group_segment_fixed_size"] <= 32 * 1024, (n, k[".group_segment_fixed_size"])
    assert ks[hits[1]][".group_segment_fixed_size"] == 4 * 64 * 32  # four waves of 64 descriptors
    assert ks[hits[0]][".group_segment_fixed_size"] == 1024 * 32
