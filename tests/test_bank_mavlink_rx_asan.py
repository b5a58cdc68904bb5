"""ASan + UBSan over aof_bank_mavlink_rx_host, driven by a stand-alone program with its own main through the
split-invariance case (tests/native/mavlink_rx_selftest.cpp): every buffer is a heap block of exactly its size, so one
byte read or written outside of it ends the run.  CPU only; nothing here is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_the_host_receive_is_clean_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "aero-optical-flow_amd", "csrc")
    exe = tmp_path / "mavlink_rx_selftest"
    # the translation unit as the library's Makefile compiles it (host only, no kernels), plus the sanitizers
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           os.path.join(ROOT, "tests", "native", "mavlink_rx_selftest.cpp"), os.path.join(csrc, "aof_mavlink_rx.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    assert "cuts of" in r.stdout and "agree" in r.stdout
