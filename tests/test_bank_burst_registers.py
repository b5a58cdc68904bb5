"""The burst kernel's register budget (k_bank_burst.hip): four workgroups of 256 lanes per compute unit need at most 128
VGPRs per lane.  The kernel gets there with an occupancy attribute and a per-round copy of the plan that the compiler
cannot hoist out of the loop over the rounds; a compiler that needs one register more would halve the number of resident
workgroups without a word, and 1 024 streams would take half as long again (LAB_LOG.md, "Stream bank in bursts").  hipcc
cross-compiles gfx950 without a GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_burst_instantiation_keeps_four_waves_per_simd_and_next_to_no_scratch():
    spec = importlib.util.spec_from_file_location("isa_hashes", os.path.join(ROOT, "tools", "isa_hashes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    found = tool.kernels_of(os.path.join(tool.CSRC, "k_bank_burst.hip"))
    burst = [k for k in found if k[0].startswith("k_bank_burst<")]
    assert len(burst) == 4, [k[0] for k in found]           # SUBPIXEL x CAMERA
    for name, _, vgprs, vgpr_spills, _, scratch in burst:
        assert 0 < vgprs <= 128, (name, vgprs)              # 512 VGPRs per SIMD lane / 4 waves
        assert vgpr_spills <= 4 and scratch <= 16, (name, vgpr_spills, scratch)   # (the camera + half-pixel one spills two dwords)
