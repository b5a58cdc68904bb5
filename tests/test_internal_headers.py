"""The library's internal headers are one per concern (csrc/aof_engine_args.hpp, aof_bank_args.hpp, aof_bank_calls.hpp,
aof_ingest_args.hpp, aof_sequence_args.hpp, aof_resident.hpp, aof_host.hpp, ...), and every file includes what it uses.
Two things keep that so.  Every header the host-only plan headers reach compiles ON ITS OWN with a plain host compiler
and no ROCm include path: it is self-contained, and the stand-alone selftests can go on building it that way.  And the
compiler's own dependency output of a handful of kernel files is held to a table: the search engine's kernels do not see
the stream bank, the bank's side calls do not see the engine.  No GPU: nothing is run, hipcc only lists dependencies."""
import os
import re
import shutil
import subprocess

import pytest

from kernel_census import ROOT, tool

CSRC = tool.CSRC
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]

# host only by contract: the plans of every launch and what the aof_set_bank_* calls have bound
PLAN_HEADERS = ("aof_small_plan.hpp", "aof_lane8_plan.hpp", "aof_cols8_plan.hpp", "aof_coarse_plan.hpp", "aof_tile16_plan.hpp",
                "aof_warp_plan.hpp", "aof_batch_plan.hpp", "aof_bank_tables.hpp")

ENGINE = {"aof_engine_args.hpp"}
BANK = {"aof_bank_args.hpp", "aof_bank_tables.hpp", "aof_bank_stream.hpp"}
BANK_CALLS = {"aof_bank_calls.hpp"}
OTHERS = {"aof_sequence_args.hpp", "aof_ingest_args.hpp", "aof_resident.hpp"}
# unit -> internal headers it must not reach
CENSUS = {
    "k_lane8_search_ff.hip": BANK | BANK_CALLS | OTHERS,
    "k_cols8_search_f.hip": BANK | BANK_CALLS | OTHERS,
    "k_search_tile16.hip": BANK | BANK_CALLS | OTHERS,
    "k_coarse.hip": BANK | BANK_CALLS | OTHERS,
    "k_reduce.hip": BANK | BANK_CALLS | OTHERS,
    "k_bank_outbox.hip": ENGINE | {"aof_bank_args.hpp"},
    "k_bank_imu.hip": ENGINE | {"aof_bank_args.hpp"},
    "k_bank_exposure.hip": ENGINE | {"aof_bank_args.hpp"},
    "k_bank_mavlink_rx.hip": ENGINE | {"aof_bank_args.hpp"},
}


def reached(cmd):
    """Base names of the project's headers in a compiler's -MM output."""
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
    return {os.path.basename(w) for w in re.split(r"[\s\\]+", out) if w.endswith((".hpp", ".h"))}


def test_every_header_the_plan_headers_reach_compiles_alone_with_a_plain_host_compiler():
    gxx = shutil.which("g++")
    assert gxx, "no host compiler"
    headers = set(PLAN_HEADERS)
    for h in PLAN_HEADERS:
        headers |= {r for r in reached([gxx, "-std=c++17", "-MM", "-x", "c++", *INCLUDES, os.path.join(CSRC, h)])
                    if os.path.exists(os.path.join(CSRC, r))}
    # what the split made: each is among them, by name, so that a header dropped from the plans' reach is still held
    headers |= {"aof_hd.hpp", "aof_fastdiv.hpp", "aof_engine_args.hpp", "aof_resident.hpp", "aof_sequence_args.hpp",
                "aof_ingest_args.hpp", "aof_bank_args.hpp", "aof_bank_calls.hpp", "aof_host.hpp"}
    bad = {}
    for h in sorted(headers):
        r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-x", "c++", *INCLUDES, os.path.join(CSRC, h)],
                           capture_output=True, text=True, timeout=300)
        if r.returncode:
            bad[h] = r.stderr[-2000:]
    assert not bad, bad


@pytest.mark.skipif(not os.path.exists(tool.HIPCC), reason="hipcc not installed")
def test_the_kernel_files_reach_only_the_headers_of_their_own_side():
    bad = {}
    for unit, forbidden in CENSUS.items():
        got = reached([tool.HIPCC, "-std=c++17", "--offload-arch=gfx950", "-MM", *INCLUDES, os.path.join(CSRC, unit)])
        assert "aof.h" in got, (unit, got)   # (the listing is one: every unit reaches the C ABI)
        wrong = got & (forbidden | {"aof_internal.hpp"})
        if wrong:
            bad[unit] = sorted(wrong)
    assert not bad, bad
