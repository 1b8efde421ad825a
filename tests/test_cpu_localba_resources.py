"""The LocalBundleAdjustment stage kernels (localba.hip) that run in every Levenberg trial have no private segment
and no spills, and the reduced solve's LDS is the 6 KiB DESIGN.md §4 states (two vectors of 384 doubles).  Reads the
gfx950 code object inside librsc.so as tests/test_cpu_kernel_resources.py does (no GPU needed)."""
from test_cpu_kernel_resources import _kernels

PER_TRIAL = ("lba_point_prep_kernel", "lba_schur_kernel", "lba_solve_kernel", "lba_update_kernel",
             "lba_edges_kernelILb0", "lba_ctl_trial_kernel", "lba_restore_kernel")
ALL = PER_TRIAL + ("lba_edges_kernelILb1", "lba_fold_kernel", "lba_ctl_begin_kernel", "lba_classify_kernel")


def test_localba_kernels_resources():
    ks = _kernels()
    for frag in ALL:
        hits = [n for n in ks if frag in n]
        assert len(hits) == 1, (frag, hits)
        k = ks[hits[0]]
        assert k[".private_segment_fixed_size"] == 0, (frag, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0, frag
        if frag in PER_TRIAL:
            assert k.get(".sgpr_spill_count", 0) == 0, frag
        lds = k[".group_segment_fixed_size"]
        assert lds == (2 * 384 * 8 if frag == "lba_solve_kernel" else 0), (frag, lds)
    assert len([n for n in ks if "lba_" in n]) == len(ALL)
