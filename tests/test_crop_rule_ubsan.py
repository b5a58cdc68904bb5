"""UBSan + ASan over the validity rule of a crop source (csrc/aof_bank_sensor_rule.hpp: bank_pixel_layout,
bank_sensor_valid_groups and bank_sensor_valid_format, which the kernels and the host's aof_bank_sensor_valid / _format /
_binned decide with), driven by a stand-alone program with its own main against one 128-bit restatement by pixel groups
over every format byte, every bin byte that matters and edge values on every axis (tests/native/crop_rule_selftest.cpp).
CPU only; nothing here is loaded into Python."""
import selftest_rig as rig


def test_the_rule_of_a_crop_source_neither_wraps_nor_overflows(tmp_path):
    exe = rig.build(tmp_path, "crop_rule_selftest", ["tests/native/crop_rule_selftest.cpp"])
    r = rig.run(exe)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    assert "agree" in r.stdout
