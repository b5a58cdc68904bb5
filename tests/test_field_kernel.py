"""The motion-field kernel as hipcc compiles it (csrc/k_field.hip, through tests/kernel_census.py): the file holds exactly its
two forms -- a wave per pair and a workgroup per pair; a file of its own, so that nothing another kernel file compiles to
moves (tests/test_isa_hashes.py and tests/test_bank_kernel_budgets.py pin those) --, each within the 128 VGPRs of four waves
per SIMD, without a spilled register and without scratch memory.  hipcc cross-compiles gfx950 without a GPU."""
from kernel_census import kernels

KERNELS = ["k_field<256, 5>", "k_field<64, 1>"]


def test_the_source_holds_exactly_its_kernels():
    assert sorted(kernels("k_field.hip")) == KERNELS


def test_every_kernel_keeps_its_budget():
    for name in KERNELS:
        _, _, vgprs, vgpr_spills, sgpr_spills, scratch = kernels("k_field.hip")[name]
        assert 0 < vgprs <= 128, (name, vgprs)
        assert (vgpr_spills, sgpr_spills, scratch) == (0, 0, 0), (name, vgpr_spills, sgpr_spills, scratch)


def test_the_library_is_built_from_it_with_contraction_off():
    import os
    import re
    from kernel_census import tool
    make = open(os.path.join(tool.CSRC, "Makefile")).read()
    assert re.search(r"\bk_field\.o\b", make) and re.search(r"\baof_field\.o\b", make)
    for target in ("k_field.o", "aof_field.o"):
        rule = re.search(r"^%s:.*\n\t(.*)$" % re.escape(target), make, re.M)
        assert rule and "-ffp-contract=off" in rule.group(1), target
