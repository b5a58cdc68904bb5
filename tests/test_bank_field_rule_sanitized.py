"""UBSan + ASan over the stream bank's motion-field step (csrc/aof_bank_field_step.hpp, which the kernel and
aof_bank_field_host both compile) and the host side around it (csrc/aof_bank_field.cpp, csrc/aof_field.cpp, csrc/aof_params.cpp),
driven by a stand-alone program with its own main against one restatement of the rules: the window worked by hand and a sweep
of every quality code over first and later frames, valid and invalid fits, with and without a per-stream focal table, arrays
allocated at their exact size (tests/native/bank_field_selftest.cpp).  CPU only; nothing here is loaded into Python."""
import selftest_rig as rig


def test_the_bank_field_step_keeps_its_rules_and_reads_nothing_outside_its_arrays(tmp_path):
    exe = rig.build(tmp_path, "bank_field_selftest", ["tests/native/bank_field_selftest.cpp", rig.CSRC + "/aof_bank_field.cpp",
                                                      rig.CSRC + "/aof_field.cpp", rig.CSRC + "/aof_params.cpp"],
                    fp_contract_off=True, float_cast=True)
    r = rig.run(exe)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    assert "agree" in r.stdout
