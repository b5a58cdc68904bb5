"""The kernels of the per-stream sensor records (aof_set_bank_sensors) are instantiations of their own: with nothing
bound, the library launches the kernels without the argument -- those of a build that never had it.  This file holds the
split in place (both forms exist, under the names the launchers pick), and holds the burst with records,
k_bank_burst_sensors, to the budget tests/test_bank_burst_registers.py sets for k_bank_burst: four workgroups of 256
lanes per compute unit need at most 128 VGPRs per lane.  hipcc cross-compiles gfx950 without a GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(tool, name):
    return {k[0]: k for k in tool.kernels_of(os.path.join(tool.CSRC, name))}


def test_bound_and_unbound_forms_are_kernels_of_their_own_and_the_bound_burst_keeps_the_budget():
    spec = importlib.util.spec_from_file_location("isa_hashes", os.path.join(ROOT, "tools", "isa_hashes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    burst = kernels(tool, "k_bank_burst.hip")
    for name in ("k_bank_burst_sensors<true>", "k_bank_burst_sensors<false>"):
        _, _, vgprs, vgpr_spills, _, scratch = burst[name]
        assert 0 < vgprs <= 128, (name, vgprs)              # 512 VGPRs per SIMD lane / 4 waves
        assert vgpr_spills <= 4 and scratch <= 16, (name, vgpr_spills, scratch)
    bank, ingest = kernels(tool, "k_bank.hip"), kernels(tool, "k_ingest.hip")
    for name in ("k_bank_tick<true, true>", "k_bank_tick<false, true>", "k_bank_tick<true, true, BankSensors>",
                 "k_bank_tick<false, true, BankSensors>", "k_bank_commit<true>", "k_bank_commit<true, BankSensors>"):
        assert name in bank, (name, sorted(bank))
    assert not any("false, BankSensors" in n for n in bank), "no plain form takes records"
    assert set(ingest) == {"k_ingest<false>", "k_ingest<false, IngestSensors>", "k_ingest<true>"}, sorted(ingest)
