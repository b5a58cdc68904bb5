"""UBSan + ASan over aof_sequence_mavlink_rx_host (csrc/aof_sequence_mavlink_rx.cpp with the state machine of
csrc/aof_mavlink_rx_step.hpp), driven by a stand-alone program with its own main (tests/native/sequence_rx_selftest.cpp) on
the model's family of designed logs (tests/sequence_rx_ref.py) and on four frames cut at EVERY length: the log flush against
the end of its heap allocation, every other array at its exact size, the outputs against the model's bytes, refused calls
write nothing.  CPU only; nothing here is loaded into Python."""
import struct

import numpy as np

import mavlink_rx_ref as rx
import selftest_rig as rig
import sequence_rx_ref as ref


def entry(log, byte_end, M):
    want = ref.model(bytes(log), byte_end, M)
    return b"".join([struct.pack("<4Q", len(log), len(byte_end), M, len(want["samples"])), bytes(log),
                     np.asarray(byte_end, np.uint32).tobytes(), want["samples"].tobytes(), want["sample_end"].tobytes(), want["state"]])


def every_cut():
    """A v1 sample, a signed v2 sample, a frame of another message and a truncated v2 sample: N at every cut of every frame."""
    log = (rx.frame_v1(rx.HIGHRES_IMU, ref.imu(0)) + rx.frame_v2(rx.HIGHRES_IMU, ref.imu(1), signature=ref.SIG) +
           rx.frame_v2(33, bytes(range(40, 60)), truncate=False) + rx.frame_v2(rx.HIGHRES_IMU, ref.imu(2)[:24], truncate=False))
    return [(log[:n], [0, n // 2, n, n + 1], 2 + n % 3) for n in range(len(log) + 1)]


def test_the_host_function_neither_overflows_nor_reads_outside_its_arrays(tmp_path):
    assert ref.SENTINEL == 0xEE
    family = [(c["log"], c["byte_end"], c["max_samples"]) for c in ref.cases()] + every_cut()
    path = tmp_path / "family.bin"
    path.write_bytes(b"".join(entry(*c) for c in family))
    exe = rig.build(tmp_path, "sequence_rx_selftest", ["tests/native/sequence_rx_selftest.cpp", rig.CSRC + "/aof_sequence_mavlink_rx.cpp"])
    r = rig.run(exe, str(path))
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    assert f"agree: {len(family)} logs" in r.stdout
