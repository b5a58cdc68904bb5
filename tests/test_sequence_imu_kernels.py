"""The sequence IMU call's kernels as hipcc compiles them (csrc/k_sequence_imu.hip): the file holds its five kernels and no
other, each within the 128 VGPRs of four waves per SIMD with no spilled register and no scratch memory; its internal header
and the sequence header it shares a helper with compile on their own with a plain host compiler; and the kernel file reaches
neither the engine's nor the bank's internal headers.  No GPU: hipcc cross-compiles gfx950 and lists dependencies."""
import os
import re
import shutil
import subprocess

import pytest

from kernel_census import ROOT, kernels, tool

CSRC = tool.CSRC
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
KERNELS = ("k_seq_imu_init", "k_seq_imu_samples", "k_seq_imu_records", "k_seq_imu_scan", "k_seq_imu_pack")
needs_hipcc = pytest.mark.skipif(not os.path.exists(tool.HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_the_source_holds_its_five_kernels_within_their_budget():
    found = kernels("k_sequence_imu.hip")
    assert set(found) == set(KERNELS), sorted(found)
    for name in KERNELS:
        _, _, vgprs, vgpr_spills, sgpr_spills, scratch = found[name]
        assert 0 < vgprs <= 128 and vgpr_spills == 0 and sgpr_spills == 0 and scratch == 0, (name, found[name])


@pytest.mark.parametrize("header", ["aof_sequence_imu_args.hpp", "aof_sequence_args.hpp", "aof_imu_step.hpp"])
def test_the_internal_headers_compile_alone_with_a_plain_host_compiler(header):
    gxx = shutil.which("g++")
    assert gxx, "no host compiler"
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-x", "c++", *INCLUDES, os.path.join(CSRC, header)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@needs_hipcc
def test_the_kernel_file_reaches_only_its_own_side():
    out = subprocess.run([tool.HIPCC, "-std=c++17", "--offload-arch=gfx950", "-MM", *INCLUDES, os.path.join(CSRC, "k_sequence_imu.hip")],
                         check=True, capture_output=True, text=True, timeout=300).stdout
    got = {os.path.basename(w) for w in re.split(r"[\s\\]+", out) if w.endswith((".hpp", ".h"))}
    assert {"aof.h", "aof_sequence_imu.h", "aof_imu_step.hpp", "aof_mavlink.hpp", "aof_sequence_imu_args.hpp"} <= got
    wrong = got & {"aof_engine_args.hpp", "aof_bank_args.hpp", "aof_bank_calls.hpp", "aof_bank_tables.hpp", "aof_sequence_args.hpp",
                   "aof_ingest_args.hpp", "aof_resident.hpp", "aof_internal.hpp"}
    assert not wrong, sorted(wrong)
