"""The one-launch tick with the warp inside it as hipcc compiles it (csrc/k_bank_tick_warp.hip, through
tests/kernel_census.py): a file of its own that holds exactly its two instantiations -- so that nothing k_bank.hip,
k_bank_burst.hip and k_ingest.hip compile to moves (tests/test_bank_kernel_budgets.py pins those) --, each within the 128
VGPRs of four workgroups per compute unit, without a spilled vector register and without scratch memory; the warp launch's
file still holds its one kernel.  hipcc cross-compiles gfx950 without a GPU."""
import os
import re

from kernel_census import kernels, tool

KERNELS = ["k_bank_tick_warped<false>", "k_bank_tick_warped<true>"]


def test_the_source_holds_exactly_its_two_instantiations():
    assert sorted(kernels("k_bank_tick_warp.hip")) == KERNELS


def test_both_keep_the_budget_of_four_workgroups_per_compute_unit():
    for name in KERNELS:
        _, _, vgprs, vgpr_spills, _, scratch = kernels("k_bank_tick_warp.hip")[name]
        assert 0 < vgprs <= 128, (name, vgprs)
        assert (vgpr_spills, scratch) == (0, 0), (name, vgpr_spills, scratch)


def test_the_library_is_built_from_it():
    make = open(os.path.join(tool.CSRC, "Makefile")).read()
    assert re.search(r"\bk_bank_tick_warp\.o\b", make)


def test_the_warp_launch_still_holds_exactly_its_kernel():
    assert sorted(kernels("k_bank_warp.hip")) == ["k_bank_warp"]


def test_the_gather_has_one_home():
    """sample_grey / sample are written in aof_warp_gather.hpp and nowhere else; both kernels include it."""
    for f in ("k_bank_warp.hip", "k_bank_tick_warp.hip"):
        text = open(os.path.join(tool.CSRC, f)).read()
        assert '#include "aof_warp_gather.hpp"' in text and "uint32_t sample_grey(" not in text, f
    assert "uint32_t sample_grey(" in open(os.path.join(tool.CSRC, "aof_warp_gather.hpp")).read()
