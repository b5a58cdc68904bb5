"""ASan + UBSan over aof_bank_mavlink_rx_host, driven by a stand-alone program with its own main through the
split-invariance case (tests/native/mavlink_rx_selftest.cpp): every buffer is a heap block of exactly its size, so one
byte read or written outside of it ends the run.  CPU only; nothing here is loaded into Python."""
import selftest_rig as rig


def test_the_host_receive_is_clean_under_asan_ubsan(tmp_path):
    # the translation unit as the library's Makefile compiles it (host only, no kernels), plus the sanitizers
    exe = rig.build(tmp_path, "mavlink_rx_selftest", ["tests/native/mavlink_rx_selftest.cpp", rig.CSRC + "/aof_mavlink_rx.cpp"], hip_host=True)
    r = rig.run(exe)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    assert "cuts of" in r.stdout and "agree" in r.stdout
