"""UBSan + ASan over the motion-field rule (csrc/aof_field_step.hpp, which the kernel and aof_field_host both compile) and the
host side around it (csrc/aof_field.cpp: the geometry, its range check, the plain loop; csrc/aof_params.cpp: the grids), driven
by a stand-alone program with its own main against one restatement in __int128: the largest grids the range check admits,
shifts at the ends of int8, determinants beyond 2^53 that convert exactly and ones that have to be rounded, arrays allocated
at their exact size (tests/native/field_selftest.cpp).  CPU only; nothing here is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "c++")


def test_the_field_rule_neither_wraps_nor_reads_outside_its_records(tmp_path):
    csrc = os.path.join(ROOT, "aero-optical-flow_amd", "csrc")
    exe = tmp_path / "field_selftest"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow",
           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           os.path.join(ROOT, "tests", "native", "field_selftest.cpp"), os.path.join(csrc, "aof_field.cpp"),
           os.path.join(csrc, "aof_params.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    assert "agree" in r.stdout
