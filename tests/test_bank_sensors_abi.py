"""The host-only side of the per-stream sensor records (include/aof.h, "the stream bank with per-stream sensors"): the
struct has the header's layout, the two helpers give the records their scalars mean, the library's validity rule -- the
kernels' function compiled for the host -- agrees with the Python integers of tests/bank_sensors_ref.py at every edge,
and the calls refuse what they can refuse without a device.  (No context exists without a device: of
aof_set_bank_sensors only the NULL context is reachable here; its other refusals, and the binding they leave alone:
tests/test_gpu_bank_sensors.py::test_bindings_and_refusals.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import bank_sensors_ref as sref

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aof_set_bank_sensors", "aof_bank_sensor_from_camera", "aof_bank_sensor_centred", "aof_bank_sensor_valid",
         "aof_ingest_sensors_device")


def test_library_header_and_binding_have_the_entry_points(aof):
    text = open(os.path.join(ROOT, "include", "aof.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", text), name
        assert name in aof.EXPORTS and getattr(aof.lib, name).restype is C.c_int
    assert re.search(r"#define AOF_TICK_BAD_SENSOR \(-5\)", text) and aof.TICK_BAD_SENSOR == -5 == sref.TICK_BAD_SENSOR
    assert callable(aof.FlowEngine.set_bank_sensors) and callable(aof.ingest_sensors)
    assert aof.BANK_SENSOR_DTYPE == sref.SENSOR_DTYPE


def test_the_record_has_the_headers_layout(aof, tmp_path):
    fields = ("offset", "pitch", "width", "height", "x0", "y0", "reserved")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "aof.h"\nint main(void) { printf("%zu", sizeof(aof_bank_sensor));\n'
           + "".join(f'printf(" %zu", offsetof(aof_bank_sensor, {f}));\n' for f in fields) + "return 0; }\n")
    f = tmp_path / "sizes.c"
    f.write_text(src)
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32, 0, 8, 12, 16, 20, 24, 28]
    assert got == [C.sizeof(aof.BankSensor)] + [getattr(aof.BankSensor, n).offset for n in fields]
    assert got[1:] == [aof.BANK_SENSOR_DTYPE.fields[n][1] for n in fields]


def test_the_helpers_give_the_records_their_scalars_mean(aof):
    p = aof.px4flow_params(64, 64)
    cam = aof.bank_camera_params(320, 240, 64, 64)
    assert [tuple(r) for r in aof.bank_sensor_from_camera(p, cam, n=3)] == [(0, 320, 320, 240, 128, 88, 0), (76800, 320, 320, 240, 128, 88, 0),
                                                                            (153600, 320, 320, 240, 128, 88, 0)]
    cam = aof.bank_camera_params(97, 81, 64, 64, camera_stride=8000)           # odd sizes: 97 // 2 - 32, 81 // 2 - 32
    assert tuple(aof.bank_sensor_from_camera(p, cam, 3)) == (24000, 97, 97, 81, 16, 8, 0)
    assert tuple(aof.bank_sensor_centred(p, 12345, 88, 80, 72)) == (12345, 88, 80, 72, 8, 4, 0)
    assert tuple(aof.bank_sensor_centred(p, (1 << 63) + 5, 64, 64, 64)) == ((1 << 63) + 5, 64, 64, 64, 0, 0, 0)
    p2 = aof.px4flow_params(128, 128, pyramid_levels=2, mean_subtract=1)
    assert tuple(aof.bank_sensor_centred(p2, 0, 152, 144, 136)) == (0, 152, 144, 136, 8, 4, 0)
    rec = aof.BankSensor()
    fc, ce = aof.lib.aof_bank_sensor_from_camera, aof.lib.aof_bank_sensor_centred
    assert fc(None, C.byref(cam), 0, C.byref(rec)) == EINVAL and fc(C.byref(p), None, 0, C.byref(rec)) == EINVAL
    assert fc(C.byref(p), C.byref(cam), 0, None) == EINVAL and fc(C.byref(p), C.byref(cam), -1, C.byref(rec)) == EINVAL
    assert fc(C.byref(p), C.byref(aof.bank_camera_params(63, 240, 64, 64)), 0, C.byref(rec)) == EINVAL       # narrower than the crop
    assert ce(None, 0, 64, 64, 64, C.byref(rec)) == EINVAL and ce(C.byref(p), 0, 64, 64, 64, None) == EINVAL
    assert ce(C.byref(p), 0, 79, 80, 72, C.byref(rec)) == EINVAL and ce(C.byref(p), 0, 80, 80, 63, C.byref(rec)) == EINVAL
    assert bytes(rec) == bytes(32), "a refused call writes nothing"


def test_the_librarys_rule_is_the_python_rule_at_every_edge(aof):
    """aof_bank_sensor_valid (the kernels' rule, host build) against bank_sensors_ref.valid: every inequality at equality
    and one beyond, offsets near 2^64, (height - 1) * pitch near 2^62, bases that would wrap a careless sum."""
    top = (1 << 64) - 1
    tall = (5, (1 << 31) - 1, 64, (1 << 31) - 1, 0, 0)
    ext = ((1 << 31) - 2) * ((1 << 31) - 1) + 64
    recs = [(100, 88, 80, 72, 16, 8), (100, 80, 80, 72, 16, 8), (100, 79, 80, 72, 16, 8), (100, 88, 80, 72, 17, 8), (100, 88, 80, 72, 16, 9),
            (100, 88, 80, 72, -1, 8), (100, 88, 80, 72, 16, -1), (100, 88, 0, 72, 0, 0), (100, 88, 80, 0, 0, 0), (0, 64, 64, 64, 0, 0),
            (top, 88, 80, 72, 16, 8), (top - 10, 88, 80, 72, 16, 8), (top - 6328 + 100, 88, 80, 72, 16, 8), (top - 6328 + 101, 88, 80, 72, 16, 8),
            tall, (100, 88, 80, 72, (1 << 31) - 1, 8), (100, (1 << 31) - 1, (1 << 31) - 1, 72, (1 << 31) - 64, 8)]
    sizes = [0, 1, 4095, 4096, 6427, 6428, 6429, 1 << 40, 4 + ext, 5 + ext, top - 1, top]
    bases = [0, 1, 500, top - ext - 5, top - ext - 4, top - 6428, top - 6427, top]
    checked = valid = 0
    for r in recs:
        rec = sref.record(*r)
        for nbytes in sizes:
            for base in bases:
                want = sref.valid(rec, 64, 64, nbytes, base)
                assert aof.bank_sensor_valid(rec, 64, 64, nbytes, base) == want, (r, nbytes, base)
                checked, valid = checked + 1, valid + want
    assert valid > 40 and checked - valid > 400
    assert aof.lib.aof_bank_sensor_valid(None, 64, 64, 0, 1) == EINVAL


def test_calls_refuse_what_they_can_without_a_device(aof):
    buf = np.full(1 << 14, 0xEE, np.uint8)
    d = buf.ctypes.data
    base = d + (-d) % 16
    setter, ingest = aof.lib.aof_set_bank_sensors, aof.lib.aof_ingest_sensors_device
    for args in ((base, 4, 1 << 20), (None, 0, 0), (base + 8, 4, 1 << 20), (base, 0, 1 << 20), (base, 4, 0)):
        assert setter(None, *args) == EINVAL
    ok = (64, 64, d, 1 << 14, base, 2, d, 4096, d, d, None)
    bad = [{0: 0}, {1: 0}, {2: None}, {3: 0}, {4: None}, {4: base + 8}, {5: -1}, {6: None, 8: None}, {7: 4095}]
    for change in bad:
        args = list(ok)
        for i, v in change.items():
            args[i] = v
        assert ingest(*args) == EINVAL, change
    args = list(ok)
    args[5] = 0
    assert ingest(*args) == 0, "no frames: nothing to do, nothing launched"
    assert (buf == 0xEE).all()
