"""What the packed pixel formats (aof_set_bank_pixel_formats) may cost the kernels: the burst with sensor records,
k_bank_burst_sensors, stays within the budget tests/test_bank_sensors_registers.py pins (four workgroups of 256 lanes per
compute unit: at most 128 VGPRs, at most 4 spilled, at most 16 bytes of scratch), no kernel is added (the format travels
with the sensor instantiations), and every kernel WITHOUT a sensor argument compiles to the instructions it compiled to in
front of the feature (tests/golden/bank_pixels_isa_hashes.txt, recorded from that commit with the hipcc named there; with
another compiler the comparison says nothing and is skipped).  hipcc cross-compiles gfx950 without a GPU."""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bank_pixels_isa_hashes.txt")
FILES = ("k_bank.hip", "k_bank_burst.hip", "k_ingest.hip")

_tool, _kernels = [], {}


def tool():
    if not _tool:
        spec = importlib.util.spec_from_file_location("isa_hashes", os.path.join(ROOT, "tools", "isa_hashes.py"))
        _tool.append(importlib.util.module_from_spec(spec))
        spec.loader.exec_module(_tool[0])
    return _tool[0]


def kernels(name):
    """{kernel: (name, hash, vgprs, vgpr spills, sgpr spills, scratch)} of one source file, compiled once."""
    if name not in _kernels:
        _kernels[name] = {k[0]: k for k in tool().kernels_of(os.path.join(tool().CSRC, name))}
    return _kernels[name]


def test_the_burst_with_records_keeps_its_budget_and_no_kernel_is_added():
    burst = kernels("k_bank_burst.hip")
    for name in ("k_bank_burst_sensors<true>", "k_bank_burst_sensors<false>"):
        _, _, vgprs, vgpr_spills, _, scratch = burst[name]
        assert 0 < vgprs <= 128, (name, vgprs)
        assert vgpr_spills <= 4 and scratch <= 16, (name, vgpr_spills, scratch)
    want = set(l.split("  ")[-1].strip() for l in open(GOLDEN) if not l.startswith("#") and l.strip())
    have = set(n for f in FILES for n in kernels(f))
    assert want <= have
    assert have - want == {"k_bank_tick<true, true, BankSensors>", "k_bank_tick<false, true, BankSensors>", "k_bank_commit<true, BankSensors>",
                           "k_bank_burst_sensors<true>", "k_bank_burst_sensors<false>", "k_ingest<false, IngestSensors>"}, sorted(have - want)


def test_kernels_without_a_sensor_argument_compile_to_the_instructions_they_compiled_to():
    lines = open(GOLDEN).read().split("\n")
    recorded = [l.split("hipcc:", 1)[1].strip() for l in lines if l.startswith("# hipcc:")]
    installed = [l.strip() for l in subprocess.run([tool().HIPCC, "--version"], capture_output=True, text=True).stdout.split("\n")[:3] if l.strip()]
    if recorded != installed:
        pytest.skip("the hashes were recorded with another hipcc: %s" % recorded[:1])
    checked = 0
    for l in lines:
        if l.startswith("#") or not l.strip():
            continue
        f, h = l.split()[:2]
        name = l.split("  ")[-1].strip()
        assert "Sensors" not in name and "_sensors" not in name
        assert kernels(f)[name][1] == h, (f, name, "was", h, "is", kernels(f)[name][1])
        checked += 1
    assert checked == 13
