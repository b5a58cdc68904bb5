"""The sequence MAVLink receive's kernels as hipcc compiles them (csrc/k_sequence_mavlink_rx.hip): the file holds its six
kernels and no other, each with no spilled register and no scratch memory, within the 128 VGPRs of four waves per SIMD and the
static LDS the plan states; the VGPR counts as the compiler gives them (a census, not a target); the library is built from the
two new objects and the facade depends on the section header; the plan and the argument header compile on their own with a
plain host compiler; and the kernel file and the host file compile the one text of the state machine.  No GPU: hipcc
cross-compiles gfx950 and lists dependencies."""
import os
import re
import shutil
import subprocess

import pytest

import sequence_rx_ref as ref
from kernel_census import ROOT, kernels, tool

CSRC = tool.CSRC
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
# VGPRs as hipcc (ROCm 7.2) allots them: recorded, not aimed at
VGPRS = {"k_seq_rx_chunk": 39, "k_seq_rx_entry": 6, "k_seq_rx_frames": 105, "k_seq_rx_scan": 13, "k_seq_rx_pack": 33,
         "k_seq_rx_sample_end": 16}
needs_hipcc = pytest.mark.skipif(not os.path.exists(tool.HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_the_source_holds_its_six_kernels_within_their_budget():
    found = kernels("k_sequence_mavlink_rx.hip")
    assert set(found) == set(VGPRS), sorted(found)
    for name in VGPRS:
        _, _, vgprs, vgpr_spills, sgpr_spills, scratch = found[name]
        assert 0 < vgprs <= 128 and vgpr_spills == 0 and sgpr_spills == 0 and scratch == 0, (name, found[name])
    print({name: found[name][2] for name in VGPRS})
    assert {name: found[name][2] for name in VGPRS} == VGPRS, "the census moved: record what the compiler gives now"


@needs_hipcc
def test_static_lds_stays_inside_the_plans_figure(tmp_path):
    r = subprocess.run([tool.HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-fast-math", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", *INCLUDES, "-c", os.path.join(CSRC, "k_sequence_mavlink_rx.hip"),
                        "-o", str(tmp_path / "k.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(lds) == len(scratch) == 6, (names, lds, scratch)
    limit = ref.plan(ref.C)["static_lds"]
    assert str(limit // 1024) + " * 1024" in re.search(r"kSeqRxLdsMax = ([^;]*);", open(os.path.join(CSRC, "aof_sequence_rx_plan.hpp")).read()).group(1)
    by_name = {n: v for n, v in zip(names, lds)}
    print(by_name)
    assert max(lds) <= limit and not any(scratch), (by_name, scratch)
    frames = next(v for n, v in by_name.items() if "k_seq_rx_frames" in n)
    assert frames == max(lds) and frames >= ref.C + 2 * ref.C, "the frame pass holds the chunk and its 16-bit pointers"


def test_the_library_is_built_from_it():
    make = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS :=(.*)$", make, re.M).group(1).split()
    assert "k_sequence_mavlink_rx.o" in objs and "aof_sequence_mavlink_rx.o" in objs
    rule = re.search(r"^aof_sequence_mavlink_rx\.o:.*\n\t(.*)$", make, re.M)
    assert rule and "-x c++" in rule.group(1) and "$(DEPFLAGS)" in rule.group(1) and "HOSTFLAGS" not in rule.group(1)
    assert re.search(r"^%\.o: %\.hip\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(HIPFLAGS\) \$\(DEPFLAGS\)", make, re.M), "the kernel file takes the pattern rule"
    facade = open(os.path.join(os.path.dirname(CSRC), "facade", "Makefile")).read()
    assert "$(ROOT)/include/aof_sequence_mavlink_rx.h" in facade


@pytest.mark.parametrize("header", ["aof_sequence_rx_plan.hpp", "aof_sequence_mavlink_rx_args.hpp", "aof_mavlink_rx_step.hpp"])
def test_the_internal_headers_compile_alone_with_a_plain_host_compiler(header):
    gxx = shutil.which("g++")
    assert gxx, "no host compiler"
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-x", "c++", *INCLUDES, os.path.join(CSRC, header)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@needs_hipcc
@pytest.mark.parametrize("source, flags", [("k_sequence_mavlink_rx.hip", ["--offload-arch=gfx950"]), ("aof_sequence_mavlink_rx.cpp", ["-x", "c++"])])
def test_both_sides_compile_the_one_text_of_the_state_machine(source, flags):
    out = subprocess.run([tool.HIPCC, "-std=c++17", *flags, "-MM", *INCLUDES, os.path.join(CSRC, source)],
                         check=True, capture_output=True, text=True, timeout=300).stdout
    paths = [w for w in re.split(r"[\s\\]+", out) if w.endswith((".hpp", ".h"))]
    got = {os.path.basename(w) for w in paths}
    assert {"aof.h", "aof_sequence_mavlink_rx.h", "aof_mavlink_rx_step.hpp", "aof_sequence_rx_plan.hpp", "aof_sequence_mavlink_rx_args.hpp"} <= got
    step = [w for w in paths if os.path.basename(w) == "aof_mavlink_rx_step.hpp"]
    assert len(set(os.path.realpath(w) for w in step)) == 1 and os.path.realpath(step[0]) == os.path.realpath(os.path.join(CSRC, "aof_mavlink_rx_step.hpp"))
    wrong = got & {"aof_engine_args.hpp", "aof_bank_args.hpp", "aof_bank_tables.hpp", "aof_sequence_args.hpp", "aof_sequence_imu_args.hpp",
                   "aof_ingest_args.hpp", "aof_resident.hpp"}
    assert not wrong, sorted(wrong)
    if source.endswith(".cpp"):
        assert not any("hip" in os.path.basename(w) for w in paths), "the host file includes no HIP header"
    text = open(os.path.join(CSRC, source)).read()
    assert "rx_byte(" in text and "rx_skip(" in text and "asm" not in text
    assert "rx_crc" not in text and "time_usec |=" not in text, "nothing of the state machine is restated"
