"""Inputs and expected values of the raw-mono-pixel tests (tests/test_bank_raw_ref.py, tests/test_bank_raw_abi.py,
tests/test_gpu_bank_raw.py): the formats of include/aof.h "raw mono pixels" (AOF_PIXEL_Y10 .. AOF_PIXEL_Y12P) beside the
three older ones (crop_source_ref's table of pixel groups, its grey value byte by byte, rule and packer), the layout tables
of the two small configurations and their fifteen-tick case.  Plain numpy: nothing here touches the GPU or the library
under test."""
import hashlib

import numpy as np

import crop_source_ref as csr
from crop_source_ref import GREY8, LUMA16_LO, LUMA16_HI, Y10, Y12, Y14, Y10P, Y12P

NEW = (Y10, Y12, Y14, Y10P, Y12P)
NAMES = {GREY8: "GREY8", LUMA16_LO: "LUMA16_LO", LUMA16_HI: "LUMA16_HI", Y10: "Y10", Y12: "Y12", Y14: "Y14", Y10P: "Y10P", Y12P: "Y12P"}
GROUPS, NO_FORMATS, BINS, SENSOR_DTYPE = csr.GROUPS, csr.NO_FORMATS, csr.BINS, csr.SENSOR_DTYPE

T = 15                      # ticks 0..9, two ticks nobody is given, and the burst of K = 3 on ticks 12..14
TICKS, K, BURST = 10, 3, 4  # (burst BURST of K rounds: ticks BURST * K ..)
INTERVAL = 50_000           # the exposure gate opens several times
RATE = 15
DENSITY = 0.9               # a stream has a frame in nine ticks of ten
SEEDS = {"px4-64": 96, "opencv-128": 97}    # (test_bank_raw_ref.py: every stream's chain publishes and holds)
SIZES = {"px4-64": (64, 64), "opencv-128": (128, 128)}


row_bytes, valid, extent, grey, put_grey, footprint, crop, record = (csr.row_bytes, csr.valid, csr.extent, csr.grey, csr.put_grey,
                                                                     csr.footprint, csr.crop, csr.record)


def pack_buffer(recs, fmts, bins, frames, nbytes, seed):
    """crop_source_ref.pack with formats and bins where the raw tests write them."""
    return csr.pack(recs, frames, nbytes, seed, fmts, bins)


def pack(grey_plane, fmt, pitch, seed):
    """A sensor frame of `fmt` whose grey values are grey_plane [H, W]: (H - 1) * pitch + row_bytes bytes, crop_source_ref's
    packer on the one record that is the whole frame."""
    H, W = grey_plane.shape
    rec = csr.record(0, pitch, W, H, 0, 0)
    assert row_bytes(fmt, W) is not None and pitch >= row_bytes(fmt, W)
    return csr.pack([rec], grey_plane[None], extent(rec, fmt), seed, [fmt])


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
    """crop_source_ref.layout with the bins where the raw tests write them."""
    return csr.layout(rows, order, w, h, bins, start)


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
