"""The independent MAVLink 2 serializer of the tests: the checksum and the OPTICAL_FLOW_RAD frame (field mapping of
mainloop.cpp:359-371, frame of mavlink_tcp.cpp:142-162) restated from the public serialization rules in ``struct`` and
plain Python.  It never calls the library: the library's packers are checked against it (tests/test_mavlink.py)."""
import struct

import numpy as np


def x25(data, crc=0xFFFF):
    """CRC-16/MCRF4XX as MAVLink accumulates it; 0x6F91 on b"123456789"."""
    for b in bytes(data):
        tmp = (b ^ (crc & 0xFF)) & 0xFF
        tmp = (tmp ^ (tmp << 4)) & 0xFF
        crc = ((crc >> 8) ^ (tmp << 8) ^ (tmp << 3) ^ (tmp >> 4)) & 0xFFFF
    return crc


def py_frame_id(offset_ts, img_time_us, dt_us, fx, fy, gyro, quality, seq, system_id=1, component_id=100):
    """One OPTICAL_FLOW_RAD frame (message 106, CRC_EXTRA 138) with the sender's identity in the header."""
    payload = struct.pack("<QIfffffIfhBB", offset_ts + img_time_us, dt_us & 0xFFFFFFFF, fx, fy,
                          np.float32(-gyro[1]), np.float32(gyro[0]), np.float32(gyro[2]), 0, -1.0, 0, 0, quality & 0xFF)
    assert len(payload) == 44
    while len(payload) > 1 and payload[-1] == 0:
        payload = payload[:-1]
    hdr = bytes([len(payload), 0, 0, seq, system_id, component_id, 106, 0, 0])
    crc = x25(bytes([138]), x25(hdr + payload))
    return b"\xfd" + hdr + payload + struct.pack("<H", crc)


def py_frame(offset_ts, img_time_us, dt_us, fx, fy, gyro, quality, seq):
    """The frame with the reference's identity: system 1, component 100."""
    return py_frame_id(offset_ts, img_time_us, dt_us, fx, fy, gyro, quality, seq)
