"""UBSan + ASan over aof_sequence_imu_host (csrc/aof_sequence_imu.cpp with the steps of csrc/aof_imu_step.hpp and the packer of
csrc/aof_mavlink.hpp), driven by a stand-alone program with its own main on the model's family of edge recordings
(tests/sequence_imu_ref.py): every array at its exact size on the heap, the outputs against the model's bytes, refused calls
write nothing (tests/native/sequence_imu_selftest.cpp).  CPU only; nothing here is loaded into Python."""
import struct

import numpy as np

import selftest_rig as rig
import sequence_imu_ref as ref


def listing(recordings):
    out = []
    for r in recordings:
        want = ref.run(r)
        out.append(struct.pack("<5Q", r["n"], r["M"], len(r["samples"]), r["offset0"], r["first_seq"]))
        for a in (r["times"], r["samples"], r["sample_end"], r["records"], want["records"], want["frames"], want["lengths"]):
            out.append(np.ascontiguousarray(a).tobytes())
        out.append(struct.pack("<I", want["sent"]) + want["state"].tobytes())
    return b"".join(out)


def test_the_host_function_neither_overflows_nor_reads_outside_its_arrays(tmp_path):
    family = ref.family()
    assert ref.SENTINEL == 0xA5
    path = tmp_path / "family.bin"
    path.write_bytes(listing(family))
    exe = rig.build(tmp_path, "sequence_imu_selftest", ["tests/native/sequence_imu_selftest.cpp", rig.CSRC + "/aof_sequence_imu.cpp"],
                    fp_contract_off=True, float_cast=True)
    r = rig.run(exe, str(path))
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    assert f"agree: {len(family)} recordings" in r.stdout
