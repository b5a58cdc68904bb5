"""UBSan + ASan over the warp rule (csrc/aof_warp_step.hpp, which the warp kernel and aof_warp_host both compile) and the
host side around it (csrc/aof_warp.cpp: the mesh builders, the one-frame host form), driven by a stand-alone program with
its own main against one restatement in 64-bit integers: extreme nodes, planes of one pixel, planes wider and taller than
32 768, crops of 1 x 1 and 9 x 17, every pixel format, planes allocated at their exact size
(tests/native/warp_selftest.cpp).  CPU only; nothing here is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "c++")


def test_the_warp_rule_neither_wraps_nor_reads_outside_its_plane(tmp_path):
    csrc = os.path.join(ROOT, "aero-optical-flow_amd", "csrc")
    exe = tmp_path / "warp_selftest"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "native", "warp_selftest.cpp"),
           os.path.join(csrc, "aof_warp.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    assert "agree" in r.stdout
