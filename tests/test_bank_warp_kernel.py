"""The warp kernel as hipcc compiles it (csrc/k_bank_warp.hip, through tests/kernel_census.py): the file holds exactly its
one kernel -- a file of its own, so that nothing k_ingest.hip, k_bank.hip and k_bank_burst.hip compile to moves
(tests/test_bank_kernel_budgets.py pins those) --, within the 128 VGPRs of four workgroups per compute unit, without a
spilled register and without scratch memory.  hipcc cross-compiles gfx950 without a GPU."""
from kernel_census import kernels

KERNELS = ["k_bank_warp"]


def test_the_source_holds_exactly_its_kernels():
    assert sorted(kernels("k_bank_warp.hip")) == KERNELS


def test_every_kernel_keeps_its_budget():
    for name in KERNELS:
        _, _, vgprs, vgpr_spills, sgpr_spills, scratch = kernels("k_bank_warp.hip")[name]
        assert 0 < vgprs <= 128, (name, vgprs)
        assert (vgpr_spills, sgpr_spills, scratch) == (0, 0, 0), (name, vgpr_spills, sgpr_spills, scratch)


def test_the_library_is_built_from_it():
    import os
    import re
    from kernel_census import tool
    make = open(os.path.join(tool.CSRC, "Makefile")).read()
    assert re.search(r"\bk_bank_warp\.o\b", make) and re.search(r"\baof_warp\.o\b", make)
