"""The sequence motion field's window pass as hipcc compiles it (csrc/k_sequence_field.hip): the file holds its one kernel
and no other -- the per-pair fit stays k_field.hip's --, within the 128 VGPRs of four waves per SIMD with no spilled register
and no scratch memory; the library is built from it with contraction off; its internal header compiles on its own with a
plain host compiler; and the kernel file reaches neither the engine's nor the bank's internal headers, nor the fit's.  No
GPU: hipcc cross-compiles gfx950 and lists dependencies."""
import os
import re
import shutil
import subprocess

import pytest

from kernel_census import ROOT, kernels, tool

CSRC = tool.CSRC
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
KERNELS = ("k_seq_field_windows",)
needs_hipcc = pytest.mark.skipif(not os.path.exists(tool.HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_the_source_holds_its_kernel_within_its_budget():
    found = kernels("k_sequence_field.hip")
    assert set(found) == set(KERNELS), sorted(found)
    for name in KERNELS:
        _, _, vgprs, vgpr_spills, sgpr_spills, scratch = found[name]
        assert 0 < vgprs <= 128 and vgpr_spills == 0 and sgpr_spills == 0 and scratch == 0, (name, found[name])


def test_the_library_is_built_from_it_with_contraction_off():
    make = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS :=(.*)$", make, re.M).group(1).split()
    for target in ("k_sequence_field.o", "aof_sequence_field.o"):
        assert target in objs, target
        rule = re.search(r"^%s:.*\n\t(.*)$" % re.escape(target), make, re.M)
        assert rule and "-ffp-contract=off" in rule.group(1) and "$(DEPFLAGS)" in rule.group(1), target
    facade = open(os.path.join(os.path.dirname(CSRC), "facade", "Makefile")).read()
    assert "$(ROOT)/include/aof_sequence_field.h" in facade


@pytest.mark.parametrize("header", ["aof_sequence_field_args.hpp", "aof_sequence_args.hpp", "aof_bank_field_step.hpp"])
def test_the_internal_headers_compile_alone_with_a_plain_host_compiler(header):
    gxx = shutil.which("g++")
    assert gxx, "no host compiler"
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-x", "c++", *INCLUDES, os.path.join(CSRC, header)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@needs_hipcc
def test_the_kernel_file_reaches_only_its_own_side():
    out = subprocess.run([tool.HIPCC, "-std=c++17", "--offload-arch=gfx950", "-MM", *INCLUDES, os.path.join(CSRC, "k_sequence_field.hip")],
                         check=True, capture_output=True, text=True, timeout=300).stdout
    got = {os.path.basename(w) for w in re.split(r"[\s\\]+", out) if w.endswith((".hpp", ".h"))}
    assert {"aof.h", "aof_sequence_field.h", "aof_bank_field_step.hpp", "aof_sequence_field_args.hpp"} <= got
    wrong = got & {"aof_engine_args.hpp", "aof_bank_args.hpp", "aof_bank_calls.hpp", "aof_bank_tables.hpp", "aof_sequence_args.hpp",
                   "aof_sequence_imu_args.hpp", "aof_ingest_args.hpp", "aof_resident.hpp", "aof_field_fit.hpp", "aof_host.hpp"}
    assert not wrong, sorted(wrong)


def test_the_step_is_written_once():
    """The window pass and the host loop run aof_bank_field_step.hpp's step; neither restates what a pair adds or what a
    publication takes, and the files the fit's and the bank's kernels are pinned by stay untouched by this call."""
    for name in ("k_sequence_field.hip", "aof_sequence_field.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "bank_field_step(" in text and "seq_field_tick(" in text, name
        assert "sum_zoom" not in text and "aof_atan2f" not in text and "asm" not in text, name
    assert "launch_field(" in open(os.path.join(CSRC, "aof_sequence_field.cpp")).read()
    assert "field_fit" not in open(os.path.join(CSRC, "k_sequence_field.hip")).read()
