"""The host-only side of the warp (include/aof.h, "the stream bank with a lens"): the entry points exist in header, library
and binding, the structs and macros have the header's sizes and values, and the calls refuse what they can refuse without
a device, writing nothing.  The rule itself: tests/test_bank_warp_ref.py (against the numpy model) and
tests/test_warp_rule_sanitized.py (under UBSan and ASan).  What needs a context -- a wrong stream count, a binning bound
as well -- is in tests/test_gpu_bank_warp.py."""
import ctypes as C
import os
import re

import numpy as np

import bank_warp_ref as wref
import crop_source_ref as csr

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aof_warp_mesh_size", "aof_warp_mesh_identity", "aof_warp_mesh_from_lens", "aof_set_bank_warps", "aof_ingest_warped_device",
         "aof_warp_host")


def test_library_header_and_binding_have_the_entry_points_and_the_macros(aof):
    text = open(os.path.join(ROOT, "include", "aof.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", text), name
        assert name in aof.EXPORTS and getattr(aof.lib, name).restype is C.c_int
    assert re.search(r"#define AOF_WARP_CELL\s+8\b", text) and aof.WARP_CELL == 8 == wref.CELL
    assert re.search(r"#define AOF_WARP_FRAC_BITS\s+5\b", text) and aof.WARP_FRAC_BITS == 5 == wref.FRAC
    assert re.search(r"#define AOF_WARP_NONE\s+INT32_MIN\b", text) and aof.WARP_NONE == -2**31 == wref.NONE
    for method in ("set_bank_warps", "ingest_warped", "warp_host"):
        assert callable(getattr(aof.FlowEngine, method)), method
    for fn in ("warp_mesh_size", "warp_mesh_identity", "warp_mesh_from_lens"):
        assert callable(getattr(aof, fn)), fn
    assert callable(aof.OpticalFlowBank.setStreamWarp) and callable(aof.OpticalFlowBank.setStreamLens)
    facade = open(os.path.join(ROOT, "aero-optical-flow_amd", "facade", "include", "flow_bank.hpp")).read()
    assert "int setStreamWarp(" in facade and "int setStreamLens(" in facade
    assert aof.lib.aof_version() == 102


def test_struct_sizes(aof):
    assert aof.WARP_POINT_DTYPE.itemsize == 8 == wref.POINT_DTYPE.itemsize and aof.WARP_POINT_DTYPE == wref.POINT_DTYPE
    assert C.sizeof(aof.Lens) == 13 * 8
    assert [n for n, _ in aof.Lens._fields_] == ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "out_fx", "out_fy", "out_cx", "out_cy"]
    text = open(os.path.join(ROOT, "include", "aof.h")).read()
    assert re.search(r"typedef struct aof_warp_point \{[^}]*int32_t x, y;\s*\} aof_warp_point;", text)
    assert aof.BANK_SENSOR_DTYPE.itemsize == 32, "the record keeps its 32 bytes: the meshes are an array of their own"


def test_the_mesh_builders_refuse_and_write_nothing(aof):
    p = aof.px4flow_params(64, 64)
    nx, ny = C.c_int32(-7), C.c_int32(-7)
    size = aof.lib.aof_warp_mesh_size
    assert size(None, C.byref(nx), C.byref(ny)) == EINVAL and size(C.byref(p), None, C.byref(ny)) == EINVAL
    assert size(C.byref(p), C.byref(nx), None) == EINVAL and (nx.value, ny.value) == (-7, -7)
    assert size(C.byref(p), C.byref(nx), C.byref(ny)) == 0 and (nx.value, ny.value) == (9, 9)
    for w, h in ((1, 1), (8, 8), (9, 17), (20, 12), (16, 136), (640, 480)):
        p.width, p.height = w, h
        assert aof.warp_mesh_size(p) == ((w + 7) // 8 + 1, (h + 7) // 8 + 1)
    for w, h in ((0, 64), (64, 0), (-1, 64)):
        p.width, p.height = w, h
        assert size(C.byref(p), C.byref(nx), C.byref(ny)) == EINVAL
    p.width, p.height = 64, 64
    out = np.full(81 * 8 + 16, 0xEE, np.uint8)
    ident, lens = aof.lib.aof_warp_mesh_identity, aof.lib.aof_warp_mesh_from_lens
    assert ident(None, 0, 0, out.ctypes.data) == EINVAL and ident(C.byref(p), 0, 0, None) == EINVAL
    # the last node, (x0 + 64) * 32, must be an int32; the first node's x must not be AOF_WARP_NONE
    top = (2**31 - 1) // 32 - 64
    assert ident(C.byref(p), top + 1, 0, out.ctypes.data) == EINVAL and ident(C.byref(p), 0, top + 1, out.ctypes.data) == EINVAL
    assert ident(C.byref(p), -2**26, 0, out.ctypes.data) == EINVAL and (out == 0xEE).all(), "a refused call writes nothing"
    assert ident(C.byref(p), top, -2**26, out.ctypes.data) == 0 and (out[81 * 8:] == 0xEE).all()
    got = out[:81 * 8].view(wref.POINT_DTYPE).reshape(9, 9)
    assert got[8, 8]["x"] == (top + 64) * 32 and got[0, 0]["y"] == -2**31
    out[:] = 0xEE
    good = aof.Lens(70, 70, 48, 40, -0.2, 0, 0, 0, 0, 70, 70, 32, 32)
    assert lens(None, C.byref(good), out.ctypes.data) == EINVAL and lens(C.byref(p), None, out.ctypes.data) == EINVAL
    assert lens(C.byref(p), C.byref(good), None) == EINVAL
    for name, v in (("out_fx", 0.0), ("out_fy", 0.0), ("out_fx", float("nan")), ("out_fy", float("inf"))):
        bad = aof.Lens.from_buffer_copy(bytes(good))
        setattr(bad, name, v)
        assert lens(C.byref(p), C.byref(bad), out.ctypes.data) == EINVAL, name
    assert (out == 0xEE).all(), "a refused call writes nothing"
    assert lens(C.byref(p), C.byref(good), out.ctypes.data) == 0 and (out[81 * 8:] == 0xEE).all()


def test_calls_refuse_what_they_can_without_a_device(aof):
    buf = np.full(1 << 14, 0xEE, np.uint8)
    d = buf.ctypes.data
    base = d + (-d) % 16
    setter, ingest = aof.lib.aof_set_bank_warps, aof.lib.aof_ingest_warped_device
    for args in ((base, 4), (None, 0), (base + 8, 4), (base, 0), (base, -1)):
        assert setter(None, *args) == EINVAL
    #     w   h   camera bytes   sensors formats points n frames stride hist ok stream
    ok = (64, 64, d, 1 << 14, base, d, base + 64, 2, d, 4096, d, d, None)
    bad = [{0: 0}, {1: 0}, {2: None}, {3: 0}, {4: None}, {4: base + 8}, {6: None}, {6: base + 8}, {6: base + 1}, {7: -1}, {8: None, 10: None}, {9: 4095}]
    for change in bad:
        for formats in (d, d + 3, None):          # (any alignment, or all grey: the refusals do not depend on it)
            args = list(ok)
            args[5] = formats
            for i, v in change.items():
                args[i] = v
            assert ingest(*args) == EINVAL, change
    args = list(ok)
    args[7] = 0
    assert ingest(*args) == 0, "no frames: nothing to do, nothing launched"
    assert (buf == 0xEE).all(), "a refused call writes nothing"


def test_warp_host_refuses_and_answers_an_invalid_record_with_zero(aof):
    w, h = 20, 12
    plane = np.random.default_rng(4).integers(0, 256, 44 * 36, dtype=np.uint8)
    rec = aof.BankSensor.from_buffer_copy(csr.record(0, 44, 44, 36, 12, 12).tobytes())
    mesh = wref.identity(w, h, 12, 12)
    crop, hist = np.full(w * h + 8, 0xEE, np.uint8), np.full(12, 0xEEEEEEEE, np.uint32)
    fn = aof.lib.aof_warp_host
    ok = [w, h, plane.ctypes.data, plane.size, C.byref(rec), 0, mesh.ctypes.data, crop.ctypes.data, hist.ctypes.data]
    for change in ({0: 0}, {1: 0}, {2: None}, {4: None}, {6: None}, {7: None, 8: None}):
        args = list(ok)
        for i, v in change.items():
            args[i] = v
        assert fn(*args) == EINVAL, change
    for change in ({3: plane.size - 1}, {5: 3}, {5: 9}, {0: 33}, {1: 25}):          # the record's own rule says no: nothing read, nothing written
        args = list(ok)
        for i, v in change.items():
            args[i] = v
        assert fn(*args) == 0, change
    assert (crop == 0xEE).all() and (hist == 0xEEEEEEEE).all()
    assert fn(*ok) == 1 and (crop[w * h:] == 0xEE).all() and (hist[10:] == 0xEEEEEEEE).all()
    assert np.array_equal(crop[:w * h].reshape(h, w), plane.reshape(36, 44)[12:24, 12:32])
    assert hist[:10].tolist() == wref.histogram(crop[:w * h].reshape(h, w)).tolist()
    only_hist = list(ok)
    only_hist[7] = None
    assert fn(*only_hist) == 1
