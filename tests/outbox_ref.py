"""The stream bank's outbox on the host (include/aof.h, "the stream bank's outbox"): what aof_bank_collect_device must
leave, byte for byte, written in plain numpy from the header's rules -- independent of the package's own views.  Nothing
here touches the GPU."""
import numpy as np

from bank_rig import OFFSET

FILL = 0xEE
FRAME = 56
HEADER, ENTRY, EXPOSURE_ENTRY = 64, 128, 64


def _np(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)


def _rows(a, width):
    """[K, S, width] uint8 of an array of records: structured [S] / [K, S], or uint8 [S, width] / [K, S, width]."""
    a = _np(a)
    if a.dtype.names:
        assert a.dtype.itemsize == width
        a = a.view(np.uint8).reshape(a.shape + (width,))
    assert a.dtype == np.uint8 and a.shape[-1] == width and a.ndim in (2, 3), (a.dtype, a.shape)
    return a.reshape((1,) + a.shape) if a.ndim == 2 else a


def layout(cap_m, cap_e):
    """(total bytes, offset of the message entries, offset of the exposure entries)."""
    return HEADER + ENTRY * cap_m + EXPOSURE_ENTRY * cap_e, HEADER, HEADER + ENTRY * cap_m


def selected(records, exposure=None):
    """Indices o = round * S + stream of the published records and of the due exposure records."""
    rec = _rows(records, 48)
    q = rec.reshape(-1, 48)[:, :4].copy().view("<i4").reshape(-1)
    m = np.flatnonzero(q >= 0)
    if exposure is None:
        return m, np.zeros(0, np.int64)
    due = _rows(exposure, 48).reshape(-1, 48)[:, 44:48].copy().view("<u4").reshape(-1)
    return m, np.flatnonzero(due != 0)


def compact(records, mavlink, lengths, exposure, derotated, cap_m, cap_e, tag=1, fill=FILL):
    """The outbox bytes: uint8 [total_bytes], pre-filled with `fill`; only the header, the first min(found, cap_m)
    message entries and the first min(found, cap_e) exposure entries are written."""
    rec = _rows(records, 48)
    K, S = rec.shape[:2]
    n = K * S
    rec = rec.reshape(n, 48)
    total, off_m, off_e = layout(cap_m, cap_e)
    out = np.full(total, fill, np.uint8)
    sel_m, sel_e = selected(records, exposure)
    frames = lens = None
    if mavlink is not None and lengths is not None:
        frames = _np(mavlink).view(np.uint8).reshape(n, FRAME)
        lens = _np(lengths).view(np.uint8).reshape(n)
    der = None
    if derotated is not None:
        der = _np(derotated).view(np.uint8).reshape(n, 8)
    def who(sel):       # stream u32, round u16 of every selected record, as bytes
        return (sel % S).astype("<u4").view(np.uint8).reshape(-1, 4), (sel // S).astype("<u2").view(np.uint8).reshape(-1, 2)

    sm = sel_m[:cap_m]
    e = np.zeros((len(sm), ENTRY), np.uint8)
    e[:, 0:4], e[:, 4:6] = who(sm)
    if frames is not None:
        e[:, 6] = lens[sm]
        keep = np.arange(FRAME)[None, :] < np.minimum(lens[sm], FRAME)[:, None]
        e[:, 8:64] = np.where(keep, frames[sm], 0)
    e[:, 64:112] = rec[sm]
    if der is not None:
        e[:, 112:120] = der[sm]
    out[off_m:off_m + ENTRY * len(sm)] = e.reshape(-1)
    if exposure is not None:
        se = sel_e[:cap_e]
        e = np.zeros((len(se), EXPOSURE_ENTRY), np.uint8)
        e[:, 0:4], e[:, 4:6] = who(se)
        e[:, 8:56] = _rows(exposure, 48).reshape(n, 48)[se]
        out[off_e:off_e + EXPOSURE_ENTRY * len(se)] = e.reshape(-1)
    header = np.zeros(HEADER, np.uint8)
    header[0:8] = np.frombuffer(np.uint64(tag).tobytes(), np.uint8)
    header[8:24] = np.frombuffer(np.array([min(len(sel_m), cap_m), len(sel_m), min(len(sel_e), cap_e), len(sel_e)], "<u4").tobytes(), np.uint8)
    out[:HEADER] = header
    return out


# The test recipe of the outbox: bank_ref.make_run(synth, 64, 64, S=37, T=24, case_seed=11, wrap=True) on the PX4 64x64
# configuration.  Published records per tick of the oracle chain at 15 Hz (computed with the oracle on the CPU): an
# empty tick (10), ticks above a capacity of 8 (1-3, 6-8, 12, 20) and ticks below it.
RECIPE = dict(w=64, h=64, S=37, T=24, case_seed=11, wrap=True)
CENSUS_15HZ = [8, 9, 9, 9, 2, 3, 9, 9, 11, 5, 0, 1, 11, 7, 7, 7, 3, 2, 5, 6, 9, 5, 6, 4]
PUBLISHED_15HZ, PUBLISHED_RATE0, RECORDS = 147, 668, 888


def recipe_run(aof, orc, synth, rate=15, offset=OFFSET):
    """(run, records [T, S], wire [T][S], lengths u8 [T, S], frames u8 [T, S, 56]) of the recipe's oracle chain."""
    import bank_ref
    p = aof.px4flow_params(64, 64)
    run = bank_ref.make_run(synth, **RECIPE)
    recs, wire = bank_ref.expected(run, [bank_ref.oracle_chain(aof, orc, p, rate, offset, 0) for _ in range(run.S)])
    lens = np.array([[len(w) for w in row] for row in wire], np.uint8)
    frames = np.zeros((run.T, run.S, FRAME), np.uint8)
    for k, row in enumerate(wire):
        for s, w in enumerate(row):
            frames[k, s, :len(w)] = np.frombuffer(w, np.uint8)
    return run, recs, wire, lens, frames
