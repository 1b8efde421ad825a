"""The two stereo kernels (stereo.hip) run without a private segment and without spills, and their LDS stays within
the 24 KB of one staged chunk of the right frame (2,048 keypoints of y, u and octave, 12 bytes each) for the match
kernel, and within the 75-bin histogram, a counter and one result record for the cut kernel.  Reads the gfx950
code object inside librsc.so as tests/test_cpu_kernel_resources.py does (no GPU needed)."""
from test_cpu_kernel_resources import _kernels


def test_stereo_kernels_have_no_scratch_and_bounded_lds():
    ks = _kernels()
    hits = [n for frag in ("stereo_cut_kernel", "stereo_match_kernel") for n in ks if frag in n]
    assert len(hits) == 2 and len([n for n in ks if "stereo_" in n]) == 2, f"stereo kernels in librsc.so: {hits}"
    for n in hits:
        k = ks[n]
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, n
    assert ks[hits[1]][".group_segment_fixed_size"] == 2048 * 12  # one chunk of (y, u, octave)
    assert ks[hits[0]][".group_segment_fixed_size"] <= 75 * 4 + 4 + 16
