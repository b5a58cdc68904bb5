"""The host-only side of the packed-pixel formats (include/aof.h, "the stream bank with packed sensor pixels"): the entry
points exist in header, library and binding, the three constants have the header's values, and the calls refuse what they
can refuse without a device, writing nothing.  (No context exists without a device: of aof_set_bank_pixel_formats only the
NULL context is reachable here; formats bound without sensors, a count mismatch and the binding a refusal leaves alone:
tests/test_gpu_bank_pixels.py::test_bindings_and_refusals.)"""
import ctypes as C
import os
import re

import numpy as np

import bank_pixels_ref as pref

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aof_set_bank_pixel_formats", "aof_bank_sensor_valid_format", "aof_ingest_sensor_formats_device")


def test_library_header_and_binding_have_the_entry_points_and_the_constants(aof):
    text = open(os.path.join(ROOT, "include", "aof.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", text), name
        assert name in aof.EXPORTS and getattr(aof.lib, name).restype is C.c_int
    for name, value in (("GREY8", 0), ("LUMA16_LO", 1), ("LUMA16_HI", 2)):
        assert re.search(r"#define AOF_PIXEL_%s\s+%d\b" % (name, value), text), name
        assert getattr(aof, "PIXEL_" + name) == value == getattr(pref, name)
    assert callable(aof.FlowEngine.set_bank_pixel_formats)
    assert callable(aof.OpticalFlowBank.enableCameraPacked) and callable(aof.OpticalFlowBank.setStreamPixelFormat)
    facade = open(os.path.join(ROOT, "aero-optical-flow_amd", "facade", "include", "flow_bank.hpp")).read()
    assert "int enableCameraPacked(" in facade and "int setStreamPixelFormat(" in facade
    # the record keeps its 32 bytes and its field names: the format is a parallel array
    assert aof.BANK_SENSOR_DTYPE.itemsize == 32 and aof.BANK_SENSOR_DTYPE.names[-1] == "reserved"


def test_calls_refuse_what_they_can_without_a_device(aof):
    buf = np.full(1 << 14, 0xEE, np.uint8)
    d = buf.ctypes.data
    base = d + (-d) % 16
    setter, ingest = aof.lib.aof_set_bank_pixel_formats, aof.lib.aof_ingest_sensor_formats_device
    for args in ((d, 4), (None, 0), (d + 1, 4), (d, 0), (d, -1)):
        assert setter(None, *args) == EINVAL
    ok = (64, 64, d, 1 << 14, base, d, 2, d, 4096, d, d, None)
    bad = [{0: 0}, {1: 0}, {2: None}, {3: 0}, {4: None}, {4: base + 8}, {6: -1}, {7: None, 9: None}, {8: 4095}]
    for change in bad:
        for formats in (d, d + 3, None):          # (any alignment, or all grey: the refusals do not depend on it)
            args = list(ok)
            args[5] = formats
            for i, v in change.items():
                args[i] = v
            assert ingest(*args) == EINVAL, change
    args = list(ok)
    args[6] = 0
    assert ingest(*args) == 0, "no frames: nothing to do, nothing launched"
    assert (buf == 0xEE).all(), "a refused call writes nothing"
