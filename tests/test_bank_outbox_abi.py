"""The outbox structures and aof_outbox_layout (include/aof.h, "the stream bank's outbox"): sizes and offsets of the
three structures as a C compiler lays them out, the layout's arithmetic and what it refuses.  CPU only."""
import ctypes as C

import numpy as np

EINVAL = -22


class Flow(C.Structure):
    _fields_ = [("flow_x", C.c_float), ("flow_y", C.c_float), ("count", C.c_uint32), ("quality", C.c_uint8), ("flags", C.c_uint8),
                ("pred_x", C.c_int8), ("pred_y", C.c_int8)]


class TickRecord(C.Structure):
    _fields_ = [("quality", C.c_int32), ("dt_us", C.c_int32), ("flow_x", C.c_float), ("flow_y", C.c_float), ("gyro_x", C.c_float),
                ("gyro_y", C.c_float), ("gyro_z", C.c_float), ("frame", C.c_uint32), ("pixel", Flow)]


class ExposureRecord(C.Structure):
    _fields_ = [("hist", C.c_uint32 * 10), ("msv", C.c_float), ("due", C.c_uint32)]


class Entry(C.Structure):
    _fields_ = [("stream", C.c_uint32), ("round", C.c_uint16), ("mavlink_len", C.c_uint8), ("reserved0", C.c_uint8),
                ("mavlink", C.c_uint8 * 56), ("record", TickRecord), ("derotated", C.c_float * 2), ("reserved1", C.c_uint8 * 8)]


class Exposure(C.Structure):
    _fields_ = [("stream", C.c_uint32), ("round", C.c_uint16), ("reserved0", C.c_uint16), ("exposure", ExposureRecord),
                ("reserved1", C.c_uint8 * 8)]


class Header(C.Structure):
    _fields_ = [("tag", C.c_uint64), ("n_messages", C.c_uint32), ("messages_found", C.c_uint32), ("n_exposures", C.c_uint32),
                ("exposures_found", C.c_uint32), ("reserved", C.c_uint8 * 40)]


def test_structure_sizes_and_offsets(aof):
    assert (C.sizeof(Entry), C.sizeof(Exposure), C.sizeof(Header)) == (128, 64, 64)
    assert C.sizeof(TickRecord) == 48 and C.sizeof(ExposureRecord) == 48
    for struct, dtype in ((Entry, aof.OUTBOX_ENTRY_DTYPE), (Exposure, aof.OUTBOX_EXPOSURE_DTYPE), (Header, aof.OUTBOX_HEADER_DTYPE)):
        assert dtype.itemsize == C.sizeof(struct)
        assert [(n, getattr(struct, n).offset) for n, *_ in struct._fields_] == [(n, dtype.fields[n][1]) for n in dtype.names]
    assert Entry.mavlink.offset == 8 and Entry.record.offset == 64 and Entry.derotated.offset == 112
    assert Exposure.exposure.offset == 8 and Header.n_messages.offset == 8


def test_layout_arithmetic_and_refusals(aof):
    for cm, ce in ((0, 0), (1, 0), (0, 1), (37, 0), (8, 5), (4096, 4096), (16 * 16384, 16 * 16384)):
        L = aof.outbox_layout(cm, ce)
        assert (L.messages, L.exposures, L.total_bytes) == (64, 64 + 128 * cm, 64 + 128 * cm + 64 * ce)
        assert L.messages % 64 == 0 and L.exposures % 64 == 0 and L.total_bytes % 64 == 0
    L = aof.OutboxLayout()
    assert aof.lib.aof_outbox_layout(1, 1, None) == EINVAL
    assert aof.lib.aof_outbox_layout(1 << 31, 0, C.byref(L)) == EINVAL and aof.lib.aof_outbox_layout(0, 1 << 31, C.byref(L)) == EINVAL
    assert aof.lib.aof_outbox_layout((1 << 31) - 1, (1 << 31) - 1, C.byref(L)) == 0
    assert L.total_bytes == 64 + 192 * ((1 << 31) - 1)


def test_host_only_refusals_need_no_device(aof):
    """What the collect call and the host allocator refuse before they touch a device."""
    out = C.c_void_p(1)
    assert aof.lib.aof_outbox_alloc_host(64, None) == EINVAL
    assert aof.lib.aof_outbox_alloc_host(0, C.byref(out)) == EINVAL and out.value is None
    assert aof.lib.aof_outbox_free_host(None) == 0
    assert aof.lib.aof_bank_collect_device(None, 1, 1, None, None, None, None, None, 1, 0, None, 0, 1, None, None) == EINVAL


def test_outbox_view_reads_the_layout(aof):
    L = aof.outbox_layout(3, 2)
    box = np.zeros(L.total_bytes, np.uint8)
    box[:64].view(aof.OUTBOX_HEADER_DTYPE)[0] = (7, 2, 5, 1, 1, np.zeros(40, np.uint8))
    box[L.messages + 128:L.messages + 132].view("<u4")[0] = 31
    box[L.exposures:L.exposures + 4].view("<u4")[0] = 9
    header, messages, exposures = aof.outbox_view(box, 3, 2)
    assert int(header["tag"]) == 7 and len(messages) == 2 and len(exposures) == 1
    assert int(messages[1]["stream"]) == 31 and int(exposures[0]["stream"]) == 9
