"""Inputs and expected values of the binning tests (tests/test_bank_binning_ref.py, tests/test_bank_binning_abi.py,
tests/test_gpu_bank_binning.py): the binned crop of include/aof.h ("binned sensor pixels", aof_set_bank_binning) as an
integer numpy model, the validity rule with a bin in Python integers, the layout tables (one stream per layout x bin) and a
packer that writes the footprint of a WANTED binned crop into a buffer of noise: bin x bin sensor pixels per crop pixel
whose rounded mean is that pixel, every one of them noise around it; the chroma / low byte of packed pixels and everything
outside the footprint are noise too.  The rule, the layouts and the formats build on bank_sensors_ref and
bank_pixels_ref.  Nothing here touches the GPU or the library under test."""
import numpy as np

import bank_cases
import bank_pixels_ref as pref
import bank_rig
import bank_sensors_ref as sref

BINS = (1, 2, 4)
BIN_MAX = 4
BAD_BINS = (0, 3, 8, 255)
T = 12
INTERVAL = 50_000           # the exposure gate opens several times in twelve ticks
RATE = 15
CASES = {"px4-64": 81, "opencv-128": 82}       # cfg: the seed of its nine-stream run
COMBOS = [(fmt, b) for fmt in pref.FORMATS for b in BINS]     # stream s: layout x bin
S = len(COMBOS)
ORDER = [4, 0, 7, 2, 5, 1, 3, 6, 8]    # the frames' order in the buffer; the last one (LUMA16_HI, bin 4) ends on the buffer's last byte


def log2(b):
    return {1: 0, 2: 1, 4: 2}[b]


def bin_plane(grey, b):
    """The binned image of a grey plane [b*h, b*w]: (the sum of each b x b block + b*b/2) >> (2 log2 b).  Integers only."""
    q = np.asarray(grey).astype(np.int64)
    H, W = q.shape
    assert H % b == 0 and W % b == 0
    sums = q.reshape(H // b, b, W // b, b).sum(axis=(1, 3))
    return ((sums + b * b // 2) >> (2 * log2(b))).astype(np.uint8)


def valid(rec, fmt, b, w, h, camera_bytes, base=0):
    """The rule of include/aof.h with a bin, in Python integers (which do not wrap)."""
    if b not in BINS or fmt not in pref.FORMATS:
        return False
    bpp = pref.bpp_of(fmt)
    off, pitch, width, height, x0, y0 = (int(rec[n]) for n in ("offset", "pitch", "width", "height", "x0", "y0"))
    if width < 1 or height < 1 or pitch < width * bpp:
        return False
    if x0 < 0 or y0 < 0 or x0 + b * w > width or y0 + b * h > height:
        return False
    return base + off + (height - 1) * pitch + width * bpp <= camera_bytes


def table(w, h):
    """One sensor per layout x bin, just large enough for its footprint plus a few pixels: an odd width, an odd pitch (for
    the packed layouts: an odd number of bytes), odd x0 and y0, offsets at mixed residues mod 16.  Rows as
    bank_pixels_ref.TABLES: (width, height, pitch, offset mod 16, origin, format); and the bins [S]."""
    rows, bins = [], []
    for s, (fmt, b) in enumerate(COMBOS):
        x0, y0 = 1 + 2 * (s % 3), 3 - 2 * (s % 2)
        width, height = x0 + b * w + 2 * (s % 2), y0 + b * h + s % 3       # (s even: the footprint touches the right edge)
        pitch = width * pref.bpp_of(fmt) + 2 * (s % 4) + (1 - (width * pref.bpp_of(fmt)) % 2)
        rows.append((width, height, pitch, (1, 8, 7, 0, 15)[s % 5], (x0, y0), fmt))
        bins.append(b)
        assert pitch % 2 == 1 and x0 % 2 == 1 and y0 % 2 == 1
    return rows, np.array(bins, np.uint8)


def grey_table(w, h):
    """The twin bank's sensors: grey frames that hold the host-binned crops, a few pixels larger than the crop."""
    return [(w + 5 + s % 2, h + 3, w + 8 + s % 3, (0, 9, 3)[s % 3], (3 + s % 2, 2), pref.GREY8) for s in range(S)]


def spread(crop, b, rng):
    """A footprint [b*h, b*w] of noisy sensor pixels whose binned image is `crop`: per crop pixel v, b*b values around v whose
    sum is b*b*v + r, r drawn from the whole range that rounds to v (-b*b/2 .. b*b/2 - 1)."""
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


def footprint(buffer, rec, fmt, b, w, h, base=0):
    """The grey bytes of the footprint the record, its format and its bin mean: [b*h, b*w], byte by byte by the header's formula."""
    bpp, phase = pref.bpp_of(fmt), pref.phase_of(fmt)
    pitch, x0, y0 = int(rec["pitch"]), int(rec["x0"]), int(rec["y0"])
    Y, X = np.arange(b * h, dtype=np.int64)[:, None], np.arange(b * w, dtype=np.int64)[None, :]
    return np.asarray(buffer)[base + int(rec["offset"]) + (y0 + Y) * pitch + (x0 + X) * bpp + phase]


def crop(buffer, rec, fmt, b, w, h, base=0):
    """The w x h binned crop: the model on the footprint."""
    return bin_plane(footprint(buffer, rec, fmt, b, w, h, base), b)


def pack(recs, fmts, bins, frames, nbytes, seed):
    """A noise buffer of nbytes in which stream s's footprint, read in its format and binned by bins[s], gives frames[s]."""
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, nbytes, dtype=np.uint8)
    h, w = frames.shape[1:]
    for s, rec in enumerate(recs):
        fmt, b = int(fmts[s]), int(bins[s])
        bpp, phase = pref.bpp_of(fmt), pref.phase_of(fmt)
        pitch = int(rec["pitch"])
        start = int(rec["offset"]) + int(rec["y0"]) * pitch + int(rec["x0"]) * bpp + phase
        foot = spread(frames[s], b, rng)
        for y in range(b * h):
            buf[start + y * pitch:start + y * pitch + b * w * bpp:bpp] = foot[y]
    return buf


_cases = {}


def case(aof, orc, synth, cfg, K=None):
    """(p, run, want, wire, due, after, derot) of a configuration: nine streams over twelve ticks (bank_ref.make_run with the
    saturated patches of bank_camera_ref), the oracle chain's records and wire frames, the exposure gate and the de-rotated
    pairs.  The run's frames are the BINNED crops the streams are to see: they translate by whole pixels per frame, which is
    what a sensor frame translating by bin times as many sensor pixels bins to.  K: a burstable run.  Computed once and
    left unchanged."""
    if (cfg, K) not in _cases:
        p = bank_rig.params_of(aof, cfg)
        if K is None:
            _cases[(cfg, K)] = (p,) + bank_cases.prepare(aof, orc, synth, p, S, T, CASES[cfg], INTERVAL, RATE, False, True, None, None,
                                                         True, True)
        else:
            import bank_camera_ref as cref
            import bank_ref as ref
            run = cref.add_saturated_patches(ref.make_run(synth, p.width, p.height, S, T, CASES[cfg]))
            _cases[(cfg, K)] = (p, bank_rig.burstable(run, K))
    return _cases[(cfg, K)]
