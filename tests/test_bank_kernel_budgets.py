"""The stream bank's kernels as hipcc compiles them, from one table: which kernels each source file holds, and what each
may cost.  Every kernel here runs four workgroups of 256 lanes per compute unit, which needs at most 128 VGPRs per lane
(512 per SIMD lane / 4 waves); a compiler that needs one register more would halve the number of
resident workgroups without a word (LAB_LOG.md, "Stream bank in bursts").  The kernels of the per-stream sensor records
(aof_set_bank_sensors, and the pixel formats that travel with them) are instantiations of their own: with nothing bound
the library launches the kernels without the argument, and those compile to the instructions pinned in
tests/golden/bank_isa_hashes.txt (tools/isa_hashes.py --update writes it; with another compiler than the one named there
the comparison says nothing and is skipped).  Nothing here looks at which instructions a kernel is made of.  Each source
is compiled once (tests/kernel_census.py); hipcc cross-compiles gfx950 without a GPU."""
import subprocess
from collections import namedtuple

import pytest

from kernel_census import kernels, tool

Budget = namedtuple("Budget", "vgprs vgpr_spills sgpr_spills scratch")   # the most a kernel may take; None: not held
BURST = Budget(128, 4, None, 16)    # the burst keeps its plan per round: scalars parked in VGPR lanes, next to no scratch
CLEAN = Budget(128, 0, 0, 0)        # no spilled register, no scratch memory

SENSOR_FORMS = {"k_bank_tick<true, true, BankSensors>", "k_bank_tick<false, true, BankSensors>", "k_bank_commit<true, BankSensors>",
                "k_bank_burst_sensors<true>", "k_bank_burst_sensors<false>", "k_ingest<false, IngestSensors>"}

# source file, the kernels it must hold, whether it may hold no other, the budget of those kernels
CENSUS = [
    ("k_bank_burst.hip", ["k_bank_burst<true, true>", "k_bank_burst<false, true>", "k_bank_burst<true, false>", "k_bank_burst<false, false>",   # SUBPIXEL x CAMERA
                          "k_bank_burst_sensors<true>", "k_bank_burst_sensors<false>"], True, BURST),
    ("k_bank.hip", ["k_bank_tick<true, true>", "k_bank_tick<false, true>", "k_bank_tick<true, true, BankSensors>",        # bound and unbound forms,
                    "k_bank_tick<false, true, BankSensors>", "k_bank_commit<true>", "k_bank_commit<true, BankSensors>"], False, None),   # under the launchers' names
    ("k_ingest.hip", ["k_ingest<false>", "k_ingest<false, IngestSensors>", "k_ingest<true>"], True, None),
    ("k_bank_outbox.hip", ["k_bank_outbox<true>", "k_bank_outbox<false>"], True, CLEAN),     # sources aligned for 16-byte loads, or not
    ("k_bank_imu.hip", ["k_bank_imu", "k_bank_imu_reset"], True, CLEAN),
    ("k_bank_exposure.hip", ["k_bank_exposure", "k_bank_exposure_reset"], True, CLEAN),
    ("k_bank_mavlink_rx.hip", ["k_bank_mavlink_rx", "k_bank_mavlink_rx_reset"], True, CLEAN),
]
PINNED = ("k_bank.hip", "k_bank_burst.hip", "k_ingest.hip")     # the files of tests/golden/bank_isa_hashes.txt


@pytest.mark.parametrize("source,names,exact,budget", CENSUS, ids=[c[0] for c in CENSUS])
def test_a_source_holds_its_kernels(source, names, exact, budget):
    found = kernels(source)
    assert set(names) <= set(found), (source, sorted(set(names) - set(found)), sorted(found))
    if exact:
        assert set(found) == set(names), (source, sorted(found))
    stem = source[:-len(".hip")]
    if stem + "<" in names[0]:     # a template: its instantiations are the listed ones, whatever else the file holds
        assert sorted(n for n in found if n.startswith(stem + "<")) == sorted(n for n in names if n.startswith(stem + "<")), sorted(found)


@pytest.mark.parametrize("source,names,exact,budget", [c for c in CENSUS if c[3]], ids=[c[0] for c in CENSUS if c[3]])
def test_every_listed_kernel_keeps_its_budget(source, names, exact, budget):
    found = kernels(source)
    for name in names:
        _, _, vgprs, vgpr_spills, sgpr_spills, scratch = found[name]
        assert 0 < vgprs <= budget.vgprs, (name, vgprs)
        assert vgpr_spills <= budget.vgpr_spills and scratch <= budget.scratch, (name, vgpr_spills, scratch)
        assert budget.sgpr_spills is None or sgpr_spills <= budget.sgpr_spills, (name, sgpr_spills)


def test_no_plain_form_takes_sensor_records():
    assert not any("false, BankSensors" in n for n in kernels("k_bank.hip")), "no plain form takes records"


def golden_lines():
    return open(tool.BANK_GOLDEN).read().split("\n")


def test_the_sensor_forms_are_the_only_kernels_behind_the_pinned_ones():
    """No kernel was added for the sensor records or the pixel formats but the six sensor instantiations."""
    want = set(l.split("  ")[-1].strip() for l in golden_lines() if not l.startswith("#") and l.strip())
    have = set(n for f in PINNED for n in kernels(f))
    assert want <= have
    assert have - want == SENSOR_FORMS, sorted(have - want)


def test_kernels_without_a_sensor_argument_compile_to_the_instructions_they_compiled_to():
    lines = golden_lines()
    recorded = [l.split("hipcc:", 1)[1].strip() for l in lines if l.startswith("# hipcc:")]
    installed = [l.strip() for l in subprocess.run([tool.HIPCC, "--version"], capture_output=True, text=True).stdout.split("\n")[:3] if l.strip()]
    if recorded != installed:
        pytest.skip("the hashes were recorded with another hipcc: %s" % recorded[:1])
    checked = 0
    for l in lines:
        if l.startswith("#") or not l.strip():
            continue
        f, h = l.split()[:2]
        name = l.split("  ")[-1].strip()
        assert "Sensors" not in name and "_sensors" not in name
        assert kernels(f)[name][1] == h, (f, name, "was", h, "is", kernels(f)[name][1],
                                          "if that is intended, run tools/isa_hashes.py --update and commit the golden file with the change")
        checked += 1
    assert checked == 13
