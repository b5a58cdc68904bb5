"""UBSan + ASan over the warp rule (csrc/aof_warp_step.hpp, which the warp kernel and aof_warp_host both compile) and the
host side around it (csrc/aof_warp.cpp: the mesh builders, the one-frame host form), driven by a stand-alone program with
its own main against one restatement in 64-bit integers: extreme nodes, planes of one pixel, planes wider and taller than
32 768, crops of 1 x 1 and 9 x 17, every pixel format, planes allocated at their exact size
(tests/native/warp_selftest.cpp).  CPU only; nothing here is loaded into Python."""
import selftest_rig as rig


def test_the_warp_rule_neither_wraps_nor_reads_outside_its_plane(tmp_path):
    exe = rig.build(tmp_path, "warp_selftest", ["tests/native/warp_selftest.cpp", rig.CSRC + "/aof_warp.cpp"], float_cast=True)
    r = rig.run(exe)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    assert "agree" in r.stdout
