"""Inputs and expected outputs of the per-stream bank tests (tests/test_gpu_bank_streams.py): a bank whose S streams are
S different cameras -- own focal lengths, output rate, vehicle-time offset and MAVLink identity (aof_bank_stream,
include/aof.h).  The expected values are bank_ref's: one oracle chain per stream, built with that stream's values, and a
packer that writes the stream's system and component id into the frame header (tests/mavlink_model.py).  Nothing here touches the GPU."""
from functools import partial

import numpy as np

import bank_ref as ref
from bank_ref import FX, FY
from mavlink_model import py_frame_id

# focal_x, focal_y, output_rate, offset_timestamp_usec, system_id, component_id, first_seq.  Stream 1: a sequence number
# that wraps, an offset beyond 32 bits; 2: no limiter; 3: offset 0, no frame is ever sent; 4: focal lengths below the
# pixel flows, which takes aof_atan2f into its swap branch; 5: a rate above the frame rate.  Where the issue's table
# sets no value, any valid one stands.
TABLE = [
    (FX, FY, 15, 5_000_000, 1, 100, 0),
    (100.0, 350.5, 10, 9_000_000_000, 2, 100, 250),
    (FX, FY, 0, 7, 255, 1, 0),
    (FX, FY, 15, 0, 3, 100, 9),
    (0.75, 0.75, 30, 123_456_789, 4, 101, 17),
    (320.25, 180.5, 200, 1 << 40, 5, 1, 128),
]
LIMITED_STREAMS = [s for s, row in enumerate(TABLE) if 0 < row[2] <= 30]
DECOY = (33.0, 44.0, 0, 77_777, 9, 9, 99)   # what a record behind the S real ones holds (the burst indexing test)


def row(s):
    return TABLE[s % len(TABLE)]


def records(aof, S, rows=None):
    """BANK_STREAM_DTYPE [S]: stream s holds rows[s] (default: the table, cycled)."""
    out = np.zeros(S, aof.BANK_STREAM_DTYPE)
    for s in range(S):
        fx, fy, rate, offset, sysid, compid, seq = rows[s] if rows is not None else row(s)
        out[s] = (fx, fy, rate, sysid, compid, seq, 0, offset, 0)
    return out


def chain(aof, orc, p, r, use_gyro=True):
    """bank_ref's oracle chain for a stream with the values of table row r."""
    fx, fy, rate, offset, sysid, compid, seq = r
    c = ref.oracle_chain(aof, orc, p, rate, offset, seq, use_gyro, fx=fx, fy=fy)
    c.pack = partial(py_frame_id, system_id=sysid, component_id=compid)
    return c


def expected(aof, orc, p, run, rows=None, use_gyro=True):
    """records [T, S] and wire [T][S] of one chain per stream (rows: per stream, default the table cycled)."""
    return ref.expected(run, [chain(aof, orc, p, rows[s] if rows is not None else row(s), use_gyro) for s in range(run.S)])
