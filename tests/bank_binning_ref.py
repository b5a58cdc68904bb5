"""Inputs and expected values of the binning tests (tests/test_bank_binning_ref.py, tests/test_bank_binning_abi.py,
tests/test_gpu_bank_binning.py): the layout tables of the binned crop of include/aof.h ("binned sensor pixels",
aof_set_bank_binning), one stream per layout x bin, and the twelve-tick case.  The binned crop as an integer numpy model,
the rule with a bin and the packer that spreads a WANTED binned crop over its footprint are crop_source_ref's.  Nothing
here touches the GPU or the library under test."""
import numpy as np

import bank_cases
import bank_pixels_ref as pref
import bank_rig
import crop_source_ref as csr

BINS, BAD_BINS = csr.BINS, csr.BAD_BINS
BIN_MAX = 4
T = 12
INTERVAL = 50_000           # the exposure gate opens several times in twelve ticks
RATE = 15
CASES = {"px4-64": 81, "opencv-128": 82}       # cfg: the seed of its nine-stream run
COMBOS = [(fmt, b) for fmt in pref.FORMATS for b in BINS]     # stream s: layout x bin
S = len(COMBOS)
ORDER = [4, 0, 7, 2, 5, 1, 3, 6, 8]    # the frames' order in the buffer; the last one (LUMA16_HI, bin 4) ends on the buffer's last byte


bin_plane, spread, footprint, crop, valid = csr.bin_plane, csr.spread, csr.footprint, csr.crop, csr.valid


def pack(recs, fmts, bins, frames, nbytes, seed):
    """crop_source_ref.pack with formats and bins where the binning tests write them."""
    return csr.pack(recs, frames, nbytes, seed, fmts, bins)


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
