"""UBSan + ASan over the stream bank's motion-field step (csrc/aof_bank_field_step.hpp, which the kernel and
aof_bank_field_host both compile) and the host side around it (csrc/aof_bank_field.cpp, csrc/aof_field.cpp, csrc/aof_params.cpp),
driven by a stand-alone program with its own main against one restatement of the rules: the window worked by hand and a sweep
of every quality code over first and later frames, valid and invalid fits, with and without a per-stream focal table, arrays
allocated at their exact size (tests/native/bank_field_selftest.cpp).  CPU only; nothing here is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "c++")


def test_the_bank_field_step_keeps_its_rules_and_reads_nothing_outside_its_arrays(tmp_path):
    csrc = os.path.join(ROOT, "aero-optical-flow_amd", "csrc")
    exe = tmp_path / "bank_field_selftest"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow",
           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           os.path.join(ROOT, "tests", "native", "bank_field_selftest.cpp"), os.path.join(csrc, "aof_bank_field.cpp"),
           os.path.join(csrc, "aof_field.cpp"), os.path.join(csrc, "aof_params.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    assert "agree" in r.stdout
