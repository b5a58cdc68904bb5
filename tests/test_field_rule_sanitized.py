"""UBSan + ASan over the motion-field rule (csrc/aof_field_step.hpp, which the kernel and aof_field_host both compile) and the
host side around it (csrc/aof_field.cpp: the geometry, its range check, the plain loop; csrc/aof_params.cpp: the grids), driven
by a stand-alone program with its own main against one restatement in __int128: the largest grids the range check admits,
shifts at the ends of int8, determinants beyond 2^53 that convert exactly and ones that have to be rounded, arrays allocated
at their exact size (tests/native/field_selftest.cpp).  CPU only; nothing here is loaded into Python."""
import selftest_rig as rig


def test_the_field_rule_neither_wraps_nor_reads_outside_its_records(tmp_path):
    exe = rig.build(tmp_path, "field_selftest", ["tests/native/field_selftest.cpp", rig.CSRC + "/aof_field.cpp", rig.CSRC + "/aof_params.cpp"],
                    fp_contract_off=True, float_cast=True)
    r = rig.run(exe)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    assert "agree" in r.stdout
