"""The stream bank's motion-field kernel as hipcc compiles it (csrc/k_bank_field.hip, through tests/kernel_census.py): the file
holds exactly its two forms -- a wave per stream and a workgroup per stream; a file of its own, so that nothing another kernel
file compiles to moves --, each within the 128 VGPRs of four waves per SIMD, without a spilled register and without scratch
memory; the fit it shares with k_field.hip is written once (csrc/aof_field_fit.hpp).  hipcc cross-compiles gfx950 without a GPU."""
import os
import re

from kernel_census import kernels, tool

KERNELS = ["k_bank_field<256, 5>", "k_bank_field<64, 1>"]


def test_the_source_holds_exactly_its_kernels():
    assert sorted(kernels("k_bank_field.hip")) == KERNELS


def test_every_kernel_keeps_its_budget():
    for name in KERNELS:
        _, _, vgprs, vgpr_spills, sgpr_spills, scratch = kernels("k_bank_field.hip")[name]
        assert 0 < vgprs <= 128, (name, vgprs)
        assert (vgpr_spills, sgpr_spills, scratch) == (0, 0, 0), (name, vgpr_spills, sgpr_spills, scratch)


def test_the_library_is_built_from_it_with_contraction_off():
    make = open(os.path.join(tool.CSRC, "Makefile")).read()
    assert re.search(r"\bk_bank_field\.o\b", make) and re.search(r"\baof_bank_field\.o\b", make)
    objs = re.search(r"^OBJS :=(.*)$", make, re.M).group(1).split()
    assert "k_bank_field.o" in objs and "aof_bank_field.o" in objs
    for target in ("k_bank_field.o", "aof_bank_field.o"):
        rule = re.search(r"^%s:.*\n\t(.*)$" % re.escape(target), make, re.M)
        assert rule and "-ffp-contract=off" in rule.group(1), target


def test_both_kernel_files_compile_one_text_of_the_fit():
    """The record loads with their peeled head and tail, the sweeps, the solve and the gated second pass stand in
    aof_field_fit.hpp; neither kernel file carries a copy."""
    fit = open(os.path.join(tool.CSRC, "aof_field_fit.hpp")).read()
    for marker in ("field_solve(", "field_inlier(", "wave_sum_i64("):
        assert marker in fit, marker
    for name in ("k_field.hip", "k_bank_field.hip"):
        text = open(os.path.join(tool.CSRC, name)).read()
        assert '#include "aof_field_fit.hpp"' in text and "field_fit<GROUP, KEEP>(" in text, name
        assert "field_solve(" not in text and "field_inlier(" not in text and "__shfl" not in text, name
    assert "asm" not in open(os.path.join(tool.CSRC, "k_bank_field.hip")).read()
