"""Inputs and expected values of the per-stream sensor tests (tests/test_bank_sensors_ref.py, tests/test_bank_sensors_abi.py,
tests/test_gpu_bank_sensors.py): the sensor record of include/aof.h (aof_bank_sensor) and its validity rule restated in
Python integers, the crop a record means by numpy slicing, the layout tables of the tests and a packer that lays S
sensor frames of different sizes, pitches and alignments into one byte buffer.  Nothing here touches the GPU or the
library under test."""
import numpy as np

import bank_cases
import bank_rig
from bank_rig import GATED, LIMITED

SENSOR_DTYPE = np.dtype([("offset", "<u8"), ("pitch", "<i4"), ("width", "<i4"), ("height", "<i4"), ("x0", "<i4"), ("y0", "<i4"),
                         ("reserved", "<u4")])
assert SENSOR_DTYPE.itemsize == 32
TICK_BAD_SENSOR = -5

# (cfg, S, seed) of the two configurations; tests/test_bank_sensors_ref.py asserts the census on the oracle's records
CASES = {"px4-64": (5, 71), "opencv-128": (3, 72)}
T = 48
INTERVAL = 200_000

# sensor width, height, pitch, offset mod 16, crop origin (None: the centre); the order in which the frames lie in the buffer
TABLES = {
    "px4-64": ([(96, 80, 96, 0, None),       # the aligned case: what aof_bank_sensor_from_camera gives
                (80, 72, 88, 8, (3, 5)),     # padded rows, x0 off a dword
                (64, 64, 64, 1, (0, 0)),     # crop == sensor; placed last: its last byte is the buffer's last valid byte
                (131, 70, 131, 7, (67, 6)),  # odd pitch, the crop touches the right and bottom edges
                (320, 240, 320, 0, None)],   # a large sensor between small ones
               [0, 1, 4, 3, 2]),
    "opencv-128": ([(160, 144, 160, 0, None),
                    (144, 136, 152, 8, (3, 5)),
                    (197, 134, 197, 7, (69, 6))],
                   [0, 1, 2]),
}
UNIFORM = {"px4-64": (96, 80), "opencv-128": (160, 144)}      # rig B: every stream's sensor, its crop at the centre
SCALARS = {"px4-64": (72, 66), "opencv-128": (136, 130)}      # what aof_bank_camera holds while records are bound: no stream's


def _format(fmt):
    """(bytes per pixel, the luma's byte in the pixel) of a pixel format, None of a value that is none.  The formats are
    bank_pixels_ref's, imported late: that module builds its tables on this one's."""
    import bank_pixels_ref as pref
    return (pref.bpp_of(fmt), pref.phase_of(fmt)) if fmt in pref.FORMATS else None


def valid(rec, w, h, camera_bytes, base=0, fmt=0):
    """The rule of include/aof.h in Python integers (which do not wrap); fmt: the stream's pixel format, 0 is grey."""
    if _format(fmt) is None:
        return False
    bpp = _format(fmt)[0]
    off, pitch, width, height, x0, y0 = (int(rec[n]) for n in ("offset", "pitch", "width", "height", "x0", "y0"))
    if width < 1 or height < 1 or pitch < width * bpp:
        return False
    if x0 < 0 or y0 < 0 or x0 + w > width or y0 + h > height:
        return False
    return base + off + (height - 1) * pitch + width * bpp <= camera_bytes


def extent(rec, fmt=0):
    """Bytes from the frame's first to behind its last."""
    return (int(rec["height"]) - 1) * int(rec["pitch"]) + int(rec["width"]) * _format(fmt)[0]


def crop(buffer, rec, w, h, base=0):
    """The w x h crop the record means, out of the flat uint8 buffer."""
    start = base + int(rec["offset"])
    pitch, x0, y0 = int(rec["pitch"]), int(rec["x0"]), int(rec["y0"])
    rows = [buffer[start + (y0 + y) * pitch + x0:start + (y0 + y) * pitch + x0 + w] for y in range(h)]
    return np.stack(rows)


def record(offset, pitch, width, height, x0, y0):
    r = np.zeros((), SENSOR_DTYPE)
    r["offset"], r["pitch"], r["width"], r["height"], r["x0"], r["y0"] = offset, pitch, width, height, x0, y0
    return r


def layout(table, order, w, h, start=0):
    """The records [S] of a table's sensors laid one behind the other in `order`, each at the next offset with the
    table's residue mod 16, and the bytes the buffer needs: the last frame's last byte is the buffer's last.  A table with
    a format as its rows' last column (bank_pixels_ref.TABLES, the pitch in bytes of that format) gives (records,
    formats [S] uint8, bytes)."""
    recs, fmts = np.zeros(len(table), SENSOR_DTYPE), np.zeros(len(table), np.uint8)
    cursor = start
    for s in order:
        width, height, pitch, mod, origin = table[s][:5]
        fmts[s] = table[s][5] if len(table[s]) > 5 else 0
        off = cursor + (mod - cursor) % 16
        x0, y0 = origin if origin is not None else (width // 2 - w // 2, height // 2 - h // 2)
        recs[s] = record(off, pitch, width, height, x0, y0)
        cursor = off + extent(recs[s], int(fmts[s]))
    return (recs, fmts, cursor) if len(table[0]) > 5 else (recs, cursor)


def pack(recs, frames, nbytes, seed, fmts=None):
    """A noise buffer of nbytes in which every record's crop, read in its format (fmts None: all grey), holds frames[s]
    ([S, h, w]).  Every other byte -- the chroma or low byte of each packed pixel included -- keeps the seeded noise, which
    does not depend on the frames."""
    buf = np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
    h, w = frames.shape[1:]
    for s, rec in enumerate(recs):
        bpp, phase = _format(0 if fmts is None else int(fmts[s]))
        pitch = int(rec["pitch"])
        start = int(rec["offset"]) + int(rec["y0"]) * pitch + int(rec["x0"]) * bpp + phase
        for y in range(h):
            buf[start + y * pitch:start + y * pitch + w * bpp:bpp] = frames[s, y]
    return buf


_cases = {}


def case(aof, orc, synth, cfg, K=None):
    """(p, run, want, wire, due, after, derot) of a configuration: bank_ref.make_run's 48 ticks with the saturated patches
    of bank_camera_ref, the oracle chain's records and wire frames, the exposure gate and the de-rotated pairs, with the
    census asserted on the oracle's records (bank_cases.prepare).  K: a burstable run (a stream keeps its leading frames
    of every K rounds), without the census.  Computed once and left unchanged."""
    if (cfg, K) not in _cases:
        S, seed = CASES[cfg]
        p = bank_rig.params_of(aof, cfg)
        if K is None:
            _cases[(cfg, K)] = (p,) + bank_cases.prepare(aof, orc, synth, p, S, T, seed, INTERVAL, 15, False, True, LIMITED, GATED, True, True)
        else:
            import bank_camera_ref as cref
            import bank_ref as ref
            run = cref.add_saturated_patches(ref.make_run(synth, p.width, p.height, S, T, seed))
            _cases[(cfg, K)] = (p, bank_rig.burstable(run, K))
    return _cases[(cfg, K)]
