"""Inputs and expected values of the raw-mono-pixel tests (tests/test_bank_raw_ref.py, tests/test_bank_raw_abi.py,
tests/test_gpu_bank_raw.py): the formats of include/aof.h "raw mono pixels" (AOF_PIXEL_Y10 .. AOF_PIXEL_Y12P) beside the
three older ones as a table of pixel groups, the grey value of a sensor pixel byte by byte from the header's formulas, the
validity rule in Python integers, a packer whose every bit that is not a grey value is seeded noise, and the layout tables
of the two small configurations.  Plain numpy: nothing here touches the GPU or the library under test."""
import hashlib

import numpy as np

import bank_binning_ref as bref
import bank_sensors_ref as sref

GREY8, LUMA16_LO, LUMA16_HI, Y10, Y12, Y14, Y10P, Y12P = 0, 1, 2, 4, 5, 6, 7, 8
NEW = (Y10, Y12, Y14, Y10P, Y12P)
NAMES = {GREY8: "GREY8", LUMA16_LO: "LUMA16_LO", LUMA16_HI: "LUMA16_HI", Y10: "Y10", Y12: "Y12", Y14: "Y14", Y10P: "Y10P", Y12P: "Y12P"}
# format: (G pixels per group, Bg bytes per group, the grey value's shift inside a 16-bit word or None)
GROUPS = {GREY8: (1, 1, None), LUMA16_LO: (1, 2, 0), LUMA16_HI: (1, 2, 8), Y10: (1, 2, 2), Y12: (1, 2, 4), Y14: (1, 2, 6),
          Y10P: (4, 5, None), Y12P: (2, 3, None)}
NO_FORMATS = (3, 9, 255)
BINS = bref.BINS
SENSOR_DTYPE = sref.SENSOR_DTYPE

T = 15                      # ticks 0..9, two ticks nobody is given, and the burst of K = 3 on ticks 12..14
TICKS, K, BURST = 10, 3, 4  # (burst BURST of K rounds: ticks BURST * K ..)
INTERVAL = 50_000           # the exposure gate opens several times
RATE = 15
DENSITY = 0.9               # a stream has a frame in nine ticks of ten
SEEDS = {"px4-64": 96, "opencv-128": 97}    # (test_bank_raw_ref.py: every stream's chain publishes and holds)
SIZES = {"px4-64": (64, 64), "opencv-128": (128, 128)}


def row_bytes(fmt, width):
    """(width / G) * Bg, None where the header's function answers -EINVAL."""
    if fmt not in GROUPS or width < 1 or width % GROUPS[fmt][0]:
        return None
    G, Bg, _ = GROUPS[fmt]
    return width // G * Bg


def valid(rec, fmt, b, w, h, camera_bytes, base=0):
    """The rule of include/aof.h in Python integers (which do not wrap)."""
    if fmt not in GROUPS or b not in BINS:
        return False
    G, Bg, _ = GROUPS[fmt]
    off, pitch, width, height, x0, y0 = (int(rec[n]) for n in ("offset", "pitch", "width", "height", "x0", "y0"))
    if width < 1 or height < 1 or width % G or x0 % G:
        return False
    rb = width // G * Bg
    if pitch < rb:
        return False
    if x0 < 0 or y0 < 0 or x0 + b * w > width or y0 + b * h > height:
        return False
    return base + off + (height - 1) * pitch + rb <= camera_bytes


def extent(rec, fmt):
    """Bytes from the frame's first to behind its last."""
    return (int(rec["height"]) - 1) * int(rec["pitch"]) + row_bytes(fmt, int(rec["width"]))


def grey(buffer, row, fmt, X):
    """The grey value of sensor pixel X of the row that starts at byte `row` of the flat buffer (arrays broadcast): the
    header's table, byte by byte."""
    G, Bg, shift = GROUPS[fmt]
    buffer, row, X = np.asarray(buffer), np.asarray(row, np.int64), np.asarray(X, np.int64)
    if shift is None:
        return buffer[row + (X // G) * Bg + X % G]
    v = buffer[row + 2 * X].astype(np.uint32) | buffer[row + 2 * X + 1].astype(np.uint32) << 8
    return ((v >> shift) & 0xFF).astype(np.uint8)


def put_grey(buffer, row, fmt, X, values):
    """Writes grey values into the buffer and leaves every other bit of it as it is: the low bits of a sample, the bits
    above it, the low-bits bytes of the packed groups."""
    G, Bg, shift = GROUPS[fmt]
    row, X = np.asarray(row, np.int64), np.asarray(X, np.int64)
    values = np.asarray(values, np.uint8)
    if shift is None:
        buffer[row + (X // G) * Bg + X % G] = values
        return
    lo, hi = row + 2 * X, row + 2 * X + 1
    word = buffer[lo].astype(np.uint32) | buffer[hi].astype(np.uint32) << 8
    word = (word & ~np.uint32(0xFF << shift)) | values.astype(np.uint32) << shift
    buffer[lo], buffer[hi] = (word & 0xFF).astype(np.uint8), (word >> 8).astype(np.uint8)


def pack(grey_plane, fmt, pitch, seed):
    """A sensor frame of `fmt` whose grey values are grey_plane [H, W]: (H - 1) * pitch + row_bytes bytes of seeded noise
    -- the samples' low bits, the bits above the sample, the packed forms' low-bits bytes and the row padding keep it, and
    it does not depend on the plane."""
    H, W = grey_plane.shape
    rb = row_bytes(fmt, W)
    assert rb is not None and pitch >= rb
    buf = np.random.default_rng(seed).integers(0, 256, (H - 1) * pitch + rb, dtype=np.uint8)
    put_grey(buf, np.arange(H)[:, None] * pitch, fmt, np.arange(W)[None, :], grey_plane)
    return buf


def footprint(buffer, rec, fmt, b, w, h, base=0):
    """The grey values of the footprint the record, its format and its bin mean: [b*h, b*w]."""
    pitch, x0, y0 = int(rec["pitch"]), int(rec["x0"]), int(rec["y0"])
    Y, X = np.arange(b * h, dtype=np.int64)[:, None], np.arange(b * w, dtype=np.int64)[None, :]
    return grey(buffer, base + int(rec["offset"]) + (y0 + Y) * pitch, fmt, x0 + X)


def crop(buffer, rec, fmt, b, w, h, base=0):
    """The w x h crop: the once-rounded mean (bank_binning_ref.bin_plane) of bin x bin grey values."""
    return bref.bin_plane(footprint(buffer, rec, fmt, b, w, h, base), b)


def record(*a):
    return sref.record(*a)


# ---- the layout tables: rows as bank_pixels_ref.TABLES (width, height, pitch in bytes, offset mod 16, origin, format), the
# streams' bins, and the frames' order in the buffer ----

def table(cfg):
    """Ten streams: every new format; a tight (0, 3, 7, 9), a padded (1, 5, 8) and an odd (2, 4, 6) pitch; offsets with
    residues 0, 1, 7, 8 mod 16; crops that touch the right and bottom edge (2, 3); a Y10P and a Y12 stream binned 2x (5,
    6), a Y10 stream binned 4x (7); and as the buffer's last frame a Y10P one whose crop is the sensor (9): camera_bytes
    ends on that frame's last low-bits byte."""
    w, h = SIZES[cfg]
    rb = row_bytes
    rows = [(w + 32, h + 16, rb(Y10, w + 32), 0, None, Y10),
            (w + 16, h + 8, rb(Y12, w + 16) + 16, 8, (3, 5), Y12),
            (w + 3, h + 6, rb(Y14, w + 3) + 1, 7, (3, 6), Y14),
            (w + 8, h + 4, rb(Y10P, w + 8), 1, (8, 4), Y10P),
            (w + 6, h + 9, rb(Y12P, w + 6) + 4, 7, (2, 3), Y12P),
            (2 * w + 12, 2 * h + 5, rb(Y10P, 2 * w + 12) + 6, 8, (4, 3), Y10P),
            (2 * w + 5, 2 * h + 2, rb(Y12, 2 * w + 5) + 3, 1, (3, 1), Y12),
            (4 * w + 4, 4 * h + 2, rb(Y10, 4 * w + 4), 0, (1, 1), Y10),
            (w + 20, h + 10, rb(Y12P, w + 20) + 12, 8, None, Y12P),
            (w, h, rb(Y10P, w), 1, (0, 0), Y10P)]
    bins = np.array([1, 1, 1, 1, 1, 2, 2, 4, 1, 1], np.uint8)
    order = [0, 5, 1, 7, 2, 3, 6, 4, 8, 9]
    return rows, bins, order


S = 10


def layout(rows, order, bins, w, h, start=0):
    """The records [S], formats [S] and the bytes of the buffer: the frames one behind the other in `order`, each at the
    next offset with its row's residue mod 16; the last frame's last byte is the buffer's last."""
    recs, fmts = np.zeros(len(rows), SENSOR_DTYPE), np.zeros(len(rows), np.uint8)
    cursor = start
    for s in order:
        width, height, pitch, mod, origin, fmt = rows[s]
        b = int(bins[s])
        off = cursor + (mod - cursor) % 16
        x0, y0 = origin if origin is not None else (width // 2 - b * w // 2, height // 2 - b * h // 2)
        recs[s], fmts[s] = sref.record(off, pitch, width, height, x0, y0), fmt
        cursor = off + extent(recs[s], fmt)
    return recs, fmts, cursor


def pack_buffer(recs, fmts, bins, frames, nbytes, seed):
    """A noise buffer of nbytes in which stream s's footprint, read in its format and binned by bins[s], gives frames[s]
    ([S, h, w]); the footprint's sensor pixels are bank_binning_ref.spread's noise around each crop pixel."""
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, nbytes, dtype=np.uint8)
    h, w = frames.shape[1:]
    for s, rec in enumerate(recs):
        fmt, b = int(fmts[s]), int(bins[s])
        foot = bref.spread(frames[s], b, rng)
        pitch, x0, y0 = int(rec["pitch"]), int(rec["x0"]), int(rec["y0"])
        put_grey(buf, int(rec["offset"]) + (y0 + np.arange(b * h)[:, None]) * pitch, fmt, x0 + np.arange(b * w)[None, :], foot)
    return buf


def grey_table(w, h, n=S):
    """The twin bank's sensors: grey frames that hold the crops, a few pixels larger than the crop."""
    return [(w + 5 + s % 2, h + 3, w + 8 + s % 3, (0, 9, 3)[s % 3], (3 + s % 2, 2)) for s in range(n)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def burst_counts(run):
    """count [T // K, S] as aof_bank_burst takes it: the frames of the one burst the tests push, zero elsewhere."""
    given = np.zeros((T // K, run.S), np.uint8)
    given[BURST] = run.active[BURST * K:BURST * K + K].sum(axis=0)
    return given


_cases = {}


def case(aof, orc, synth, cfg):
    """(p, run, want, wire) of a configuration: ten streams over T ticks (bank_ref.make_run, a stream idle in one tick of
    ten, with the saturated patches of bank_camera_ref; ticks 10 and 11 belong to nobody, so the chain sees exactly what
    the device test pushes: ticks 0..9, then the burst of K = 3 on ticks 12..14, where a stream keeps its leading frames), and the oracle chain's records and wire frames over the
    frames -- which are the crops the streams are to see.  Computed once and left unchanged."""
    if cfg not in _cases:
        import bank_camera_ref as cref
        import bank_ref as ref
        import bank_rig
        p = bank_rig.params_of(aof, cfg)
        run = cref.add_saturated_patches(ref.make_run(synth, p.width, p.height, S, T, SEEDS[cfg], density=DENSITY))
        run.active[TICKS:BURST * K] = 0
        run.active[BURST * K:] = run.active[BURST * K:].cumprod(axis=0)     # (a burst's frames are a stream's leading rounds)
        want, wire = ref.expected(run, [ref.oracle_chain(aof, orc, p, RATE, bank_rig.OFFSET, 0, True) for _ in range(S)])
        _cases[cfg] = (p, run, want, wire)
    return _cases[cfg]
