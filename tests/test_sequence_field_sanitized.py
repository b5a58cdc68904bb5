"""UBSan + ASan over aof_sequence_field_host (csrc/aof_sequence_field.cpp with the step of csrc/aof_bank_field_step.hpp and the
fit of csrc/aof_field.cpp), driven by a stand-alone program with its own main that holds it to the frame-by-frame loop of the
contract -- aof_field_host, then bank_field_step for every frame -- on recordings whose arrays are allocated at their exact
size, and checks that refused calls write nothing (tests/native/sequence_field_selftest.cpp).  CPU only; nothing here is
loaded into Python."""
import re

import selftest_rig as rig


def test_the_host_function_is_the_frame_by_frame_loop_and_reads_nothing_outside_its_arrays(tmp_path):
    exe = rig.build(tmp_path, "sequence_field_selftest",
                    ["tests/native/sequence_field_selftest.cpp", rig.CSRC + "/aof_sequence_field.cpp", rig.CSRC + "/aof_field.cpp",
                     rig.CSRC + "/aof_params.cpp"], fp_contract_off=True, float_cast=True)
    r = rig.run(exe)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    m = re.search(r"agree: (\d+) records over (\d+) pairs", r.stdout)
    assert m and int(m.group(1)) >= 60 and int(m.group(2)) >= 1000, r.stdout
