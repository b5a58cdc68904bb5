"""The host-only side of the raw mono pixels (include/aof.h, "the stream bank with raw mono pixels"): the format macros carry
the header's values in the binding, the new export aof_bank_pixel_row_bytes exists in header, library and binding and
answers as the header says at its edges, and the NULL / -EINVAL paths write nothing.  No device is needed."""
import ctypes as C
import os
import re

import pytest

import bank_raw_ref as rref

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MACROS = {"AOF_PIXEL_Y10": 4, "AOF_PIXEL_Y12": 5, "AOF_PIXEL_Y14": 6, "AOF_PIXEL_Y10P": 7, "AOF_PIXEL_Y12P": 8}


def header():
    return open(os.path.join(ROOT, "include", "aof.h")).read()


def test_the_defines_carry_the_headers_values_in_the_binding(aof):
    text = header()
    for name, value in MACROS.items():
        m = re.search(r"#define " + name + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value, name
        assert getattr(aof, name[len("AOF_"):]) == value, name
    assert (rref.Y10, rref.Y12, rref.Y14, rref.Y10P, rref.Y12P) == tuple(MACROS.values())
    assert (aof.PIXEL_GREY8, aof.PIXEL_LUMA16_LO, aof.PIXEL_LUMA16_HI) == (0, 1, 2), "the older codes keep their values"
    assert not re.search(r"#define AOF_PIXEL_\w+\s+3\b", text), "3 stays no format"


def test_the_new_export_is_in_the_header_the_library_and_the_binding(aof):
    name = "aof_bank_pixel_row_bytes"
    assert re.search(r"\bint " + name + r"\(uint8_t format, int32_t width, int64_t \*out\);", header())
    assert name in aof.EXPORTS and getattr(aof.lib, name).restype is C.c_int
    assert callable(aof.bank_pixel_row_bytes)
    assert aof.BANK_SENSOR_DTYPE.itemsize == 32, "the record keeps its 32 bytes: the format is a parallel byte"


def test_row_bytes_at_its_edges(aof):
    top = 2 ** 31 - 1
    for fmt in range(256):
        G, Bg = rref.GROUPS[fmt][:2] if fmt in rref.GROUPS else (None, None)
        for width in (-(2 ** 31), -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 66, 640, top - 3, top - 1, top):
            want = rref.row_bytes(fmt, width)
            out = C.c_int64(-77)
            rc = aof.lib.aof_bank_pixel_row_bytes(fmt, width, C.byref(out))
            if want is None:
                assert rc == EINVAL and out.value == -77, (fmt, width, "a refused call writes nothing")
                with pytest.raises(aof.AofError):
                    aof.bank_pixel_row_bytes(fmt, width)
            else:
                assert rc == 0 and out.value == want == width // G * Bg, (fmt, width)
                assert aof.bank_pixel_row_bytes(fmt, width) == want
    assert rref.row_bytes(rref.Y10P, top - 3) == (top - 3) // 4 * 5 > 2 ** 31, "a row of more than 2^31 bytes is counted in 64 bits"
    assert rref.row_bytes(rref.Y10, top) == 2 * top
    assert [rref.row_bytes(f, 640) for f in (0, 1, 2, 4, 5, 6, 7, 8)] == [640, 1280, 1280, 1280, 1280, 1280, 800, 960]
    assert all(rref.row_bytes(f, 640) is None for f in rref.NO_FORMATS)


def test_null_and_einval_paths(aof):
    out = C.c_int64(-77)
    fn = aof.lib.aof_bank_pixel_row_bytes
    assert fn(rref.Y10P, 640, None) == EINVAL and fn(rref.GREY8, 640, None) == EINVAL
    for fmt, width in ((3, 640), (9, 640), (255, 640), (rref.Y10P, 642), (rref.Y10P, 641), (rref.Y12P, 641), (rref.Y12, 0), (rref.Y12, -4)):
        assert fn(fmt, width, C.byref(out)) == EINVAL and out.value == -77, (fmt, width)
    assert aof.lib.aof_bank_sensor_valid_format(None, rref.Y10P, 64, 64, 0, 1) == EINVAL
    assert aof.lib.aof_bank_sensor_valid_binned(None, rref.Y12, 2, 64, 64, 0, 1) == EINVAL
    p = aof.px4flow_params(64, 64)
    rec = aof.BankSensor()
    centred = aof.lib.aof_bank_sensor_centred_binned
    for args in ((0, 800, 640, 480, 3, 1), (0, 800, 640, 480, 9, 1), (0, 799, 640, 480, rref.Y10P, 1), (0, 805, 642, 480, rref.Y10P, 1),
                 (0, 961, 641, 480, rref.Y12P, 1), (0, 800, 640, 480, rref.Y10P, 3)):
        C.memset(C.byref(rec), 0xEE, C.sizeof(rec))
        assert centred(C.byref(p), *args, C.byref(rec)) == EINVAL, args
        assert bytes(rec) == b"\xee" * 32, "a refused call writes nothing"
    assert centred(C.byref(p), 0, 800, 640, 480, rref.Y10P, 1, None) == EINVAL
    assert centred(None, 0, 800, 640, 480, rref.Y10P, 1, C.byref(rec)) == EINVAL
