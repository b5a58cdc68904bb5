"""The ONE model of a crop source in numpy and Python integers: a sensor record (aof_bank_sensor, include/aof.h), a pixel
format (AOF_PIXEL_*, a table of pixel groups) and a bin mean a crop of w x h grey pixels in a flat byte buffer.  The
validity rule (integers that do not wrap), the grey value of a sensor pixel byte by byte from the header's formulas, the
once-rounded binned crop, the layout of a table's frames one behind the other and the packer that writes wanted crops into
a buffer of seeded noise.  bank_sensors_ref, bank_pixels_ref, bank_binning_ref and bank_raw_ref keep their tables and case
builders and ask here; a new layout or bin is a change to GROUPS or BINS.  Nothing here touches the GPU or the library
under test."""
import numpy as np

SENSOR_DTYPE = np.dtype([("offset", "<u8"), ("pitch", "<i4"), ("width", "<i4"), ("height", "<i4"), ("x0", "<i4"), ("y0", "<i4"),
                         ("reserved", "<u4")])
assert SENSOR_DTYPE.itemsize == 32

GREY8, LUMA16_LO, LUMA16_HI, Y10, Y12, Y14, Y10P, Y12P = 0, 1, 2, 4, 5, 6, 7, 8
# format: (G pixels per group, Bg bytes per group, the grey value's shift inside a 16-bit word or None)
GROUPS = {GREY8: (1, 1, None), LUMA16_LO: (1, 2, 0), LUMA16_HI: (1, 2, 8), Y10: (1, 2, 2), Y12: (1, 2, 4), Y14: (1, 2, 6),
          Y10P: (4, 5, None), Y12P: (2, 3, None)}
NO_FORMATS = (3, 9, 255)
BINS = (1, 2, 4)
BAD_BINS = (0, 3, 8, 255)


def record(offset, pitch, width, height, x0, y0):
    r = np.zeros((), SENSOR_DTYPE)
    r["offset"], r["pitch"], r["width"], r["height"], r["x0"], r["y0"] = offset, pitch, width, height, x0, y0
    return r


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
    off, pitch, width, height, x0, y0 = (int(rec[n]) for n in ("offset", "pitch", "width", "height", "x0", "y0"))
    rb = row_bytes(fmt, width)
    if height < 1 or rb is None or x0 % GROUPS[fmt][0] or pitch < rb:
        return False
    if x0 < 0 or y0 < 0 or x0 + b * w > width or y0 + b * h > height:
        return False
    return base + off + (height - 1) * pitch + rb <= camera_bytes


def extent(rec, fmt=GREY8):
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


def footprint(buffer, rec, fmt, b, w, h, base=0):
    """The grey values of the footprint the record, its format and its bin mean: [b*h, b*w]."""
    pitch, x0, y0 = int(rec["pitch"]), int(rec["x0"]), int(rec["y0"])
    Y, X = np.arange(b * h, dtype=np.int64)[:, None], np.arange(b * w, dtype=np.int64)[None, :]
    return grey(buffer, base + int(rec["offset"]) + (y0 + Y) * pitch, fmt, x0 + X)


def bin_plane(plane, b):
    """The binned image of a grey plane [b*h, b*w]: (the sum of each b x b block + b*b/2) >> (2 log2 b).  Integers only."""
    q = np.asarray(plane).astype(np.int64)
    H, W = q.shape
    assert H % b == 0 and W % b == 0
    sums = q.reshape(H // b, b, W // b, b).sum(axis=(1, 3))
    return ((sums + b * b // 2) >> {1: 0, 2: 2, 4: 4}[b]).astype(np.uint8)


def crop(buffer, rec, fmt, b, w, h, base=0):
    """The w x h crop: the once-rounded mean of bin x bin grey values."""
    return bin_plane(footprint(buffer, rec, fmt, b, w, h, base), b)


def spread(crop, b, rng):
    """A footprint [b*h, b*w] of noisy sensor pixels whose binned image is `crop`: per crop pixel v, b*b values around v whose
    sum is b*b*v + r, r drawn from the whole range that rounds to v (-b*b/2 .. b*b/2 - 1).  b 1: the crop, nothing drawn."""
    h, w = crop.shape
    n = b * b
    if b == 1:
        return crop.copy()
    v = crop.astype(np.int64)
    target = np.clip(n * v + rng.integers(-(n // 2), n // 2, v.shape), 0, 255 * n)
    vals = np.clip(v[..., None] + rng.integers(-40, 41, v.shape + (n,)), 0, 255)
    diff = target - vals.sum(-1)
    for i in rng.permutation(n):                       # hand the difference out, each value within 0..255
        step = np.clip(diff, -vals[..., i], 255 - vals[..., i])
        vals[..., i] += step
        diff -= step
    assert (diff == 0).all()
    out = vals.reshape(h, w, b, b).transpose(0, 2, 1, 3).reshape(h * b, w * b).astype(np.uint8)
    assert (bin_plane(out, b) == crop).all()
    return out


def layout(rows, order, w, h, bins=None, start=0):
    """The records [S], formats [S] and the bytes of the buffer: the frames of `rows` -- (width, height, pitch in bytes,
    offset mod 16, crop origin or None for the centre of the footprint[, format: grey without the column]) -- one behind
    the other in `order`, each at the next offset with its row's residue mod 16; the last frame's last byte is the
    buffer's last.  bins: the streams' bins [S], default 1."""
    recs, fmts = np.zeros(len(rows), SENSOR_DTYPE), np.zeros(len(rows), np.uint8)
    cursor = start
    for s in order:
        width, height, pitch, mod, origin = rows[s][:5]
        fmts[s] = rows[s][5] if len(rows[s]) > 5 else GREY8
        b = 1 if bins is None else int(bins[s])
        off = cursor + (mod - cursor) % 16
        x0, y0 = origin if origin is not None else (width // 2 - b * w // 2, height // 2 - b * h // 2)
        recs[s] = record(off, pitch, width, height, x0, y0)
        cursor = off + extent(recs[s], int(fmts[s]))
    return recs, fmts, cursor


def pack(recs, frames, nbytes, seed, fmts=None, bins=None):
    """A noise buffer of nbytes in which stream s's footprint, read in its format (fmts None: grey) and binned by bins[s]
    (None: 1), gives frames[s] ([S, h, w]); a binned footprint's sensor pixels are spread's noise around each crop pixel.
    Every bit that is not a grey value -- the chroma or low byte of a 16-bit pixel, the bits around a raw sample, the
    low-bits bytes of the packed groups, everything outside the footprints -- keeps the seeded noise, which does not
    depend on the frames."""
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, nbytes, dtype=np.uint8)
    h, w = frames.shape[1:]
    for s, rec in enumerate(recs):
        fmt, b = GREY8 if fmts is None else int(fmts[s]), 1 if bins is None else int(bins[s])
        foot = spread(frames[s], b, rng)
        pitch, x0, y0 = int(rec["pitch"]), int(rec["x0"]), int(rec["y0"])
        put_grey(buf, int(rec["offset"]) + (y0 + np.arange(b * h)[:, None]) * pitch, fmt, x0 + np.arange(b * w)[None, :], foot)
    return buf
