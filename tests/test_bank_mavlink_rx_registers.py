"""The receive call's kernels (k_bank_mavlink_rx.hip): exactly the two kernels, no scratch memory and no spilled
register in either, and registers for at least four waves per SIMD.  Nothing here looks at which
instructions the kernels are made of.  hipcc cross-compiles gfx950 without a GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_receive_kernels_use_no_scratch_and_spill_nothing():
    spec = importlib.util.spec_from_file_location("isa_hashes", os.path.join(ROOT, "tools", "isa_hashes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    found = tool.kernels_of(os.path.join(tool.CSRC, "k_bank_mavlink_rx.hip"))
    assert sorted(k[0] for k in found) == ["k_bank_mavlink_rx", "k_bank_mavlink_rx_reset"], [k[0] for k in found]
    for name, _, vgprs, vgpr_spills, sgpr_spills, scratch in found:
        assert 0 < vgprs <= 128, (name, vgprs)               # 512 VGPRs per SIMD lane / 4 waves, as every kernel here
        assert vgpr_spills == 0 and sgpr_spills == 0 and scratch == 0, (name, vgpr_spills, sgpr_spills, scratch)
