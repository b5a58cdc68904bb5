"""The reference side of the per-stream sensor tests (tests/bank_sensors_ref.py), checked on the CPU: the packer's crops
are the run's frames, the validity rule holds at every edge, and the inputs of the GPU tests meet the census on the
ORACLE's records (bank_rig.LIMITED, bank_rig.GATED) -- a bank that never publishes, holds, idles or gates cannot pass.
The grey layouts and buffers are pinned by sha256."""
import hashlib

import numpy as np
import pytest

import bank_ref as ref
import bank_sensors_ref as sref
from bank_rig import GATED, LIMITED


@pytest.mark.parametrize("cfg", sorted(sref.CASES))
def test_the_packers_crops_are_the_runs_frames(aof, synth, cfg):
    S, seed = sref.CASES[cfg]
    w = 64 if cfg == "px4-64" else 128
    table, order = sref.TABLES[cfg]
    recs, nbytes = sref.layout(table, order, w, w)
    assert len(recs) == S
    run = ref.make_run(synth, w, w, S, 4, seed)
    for k in range(4):
        buf = sref.pack(recs, run.frames[k], nbytes, seed + k)
        for s in range(S):
            assert np.array_equal(sref.crop(buf, recs[s], w, w), run.frames[k, s]), (k, s)
            assert sref.valid(recs[s], w, w, nbytes) and int(recs[s]["offset"]) % 16 == table[s][3]
    # the frames do not overlap, and the last one ends with the buffer: one byte less and its record is invalid
    spans = sorted((int(r["offset"]), int(r["offset"]) + sref.extent(r)) for r in recs)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == nbytes
    last = order[-1]
    assert not sref.valid(recs[last], w, w, nbytes - 1)
    # a second layout behind the first (the rotating-buffer test): same residues
    recs2, end2 = sref.layout(table, order, w, w, start=nbytes)
    assert all(int(a["offset"]) % 16 == int(b["offset"]) % 16 for a, b in zip(recs, recs2)) and end2 > nbytes


def test_stream_zero_is_what_the_centre_rule_gives():
    recs, _ = sref.layout(*sref.TABLES["px4-64"], 64, 64)
    assert tuple(recs[0]) == (0, 96, 96, 80, 16, 8, 0) and tuple(recs[4])[1:6] == (320, 320, 240, 128, 88)


def test_the_validity_rule_at_every_edge():
    """Each inequality at equality and one beyond; offset near 2^64 and (height - 1) * pitch near 2^62 (Python integers
    do not wrap: what a 64-bit implementation has to reproduce, tests/test_bank_sensors_abi.py)."""
    w = h = 64
    good = sref.record(100, 88, 80, 72, 16, 8)
    need = 100 + 71 * 88 + 80
    assert sref.valid(good, w, h, need) and not sref.valid(good, w, h, need - 1)
    assert sref.valid(good, w, h, need + 500, base=500) and not sref.valid(good, w, h, need + 499, base=500)
    edit = lambda **kw: sref.record(*[kw.get(n, int(good[n])) for n in ("offset", "pitch", "width", "height", "x0", "y0")])
    big = 1 << 40
    assert sref.valid(edit(pitch=80), w, h, big) and not sref.valid(edit(pitch=79), w, h, big)
    assert sref.valid(edit(x0=0, y0=0), w, h, big) and not sref.valid(edit(x0=-1), w, h, big) and not sref.valid(edit(y0=-1), w, h, big)
    assert sref.valid(edit(x0=16), w, h, big) and not sref.valid(edit(x0=17), w, h, big)
    assert sref.valid(edit(y0=8), w, h, big) and not sref.valid(edit(y0=9), w, h, big)
    assert sref.valid(sref.record(0, 64, 64, 64, 0, 0), w, h, 4096) and not sref.valid(sref.record(0, 64, 64, 64, 0, 0), w, h, 4095)
    assert not sref.valid(edit(width=0), w, h, big) and not sref.valid(edit(height=0), w, h, big)
    assert sref.valid(sref.record(0, 1, 1, 1, 0, 0), 1, 1, 1) and not sref.valid(sref.record(1, 1, 1, 1, 0, 0), 1, 1, 1)
    top = (1 << 64) - 1
    assert not sref.valid(edit(offset=top), w, h, top) and not sref.valid(edit(offset=top - 10), w, h, top)
    assert sref.valid(edit(offset=top - need + 100), w, h, top) and not sref.valid(edit(offset=top - need + 101), w, h, top)
    tall = sref.record(5, (1 << 31) - 1, 64, (1 << 31) - 1, 0, 0)
    ext = ((1 << 31) - 2) * ((1 << 31) - 1) + 64
    assert (1 << 61) < ext < (1 << 62) and sref.valid(tall, w, h, 5 + ext) and not sref.valid(tall, w, h, 4 + ext)
    assert not sref.valid(tall, w, h, top, base=top - ext - 4) and sref.valid(tall, w, h, top, base=top - ext - 5)


@pytest.mark.parametrize("cfg", sorted(sref.CASES))
def test_the_chosen_seeds_meet_the_census_on_the_oracle(aof, orc, synth, cfg):
    """Asserted inside bank_cases.prepare on the oracle chain's records; restated here per stream."""
    p, run, want, wire, due, after, derot = sref.case(aof, orc, synth, cfg)
    pub, held, idle = ref.census(want)
    assert pub.min() >= LIMITED[0] and held.min() >= LIMITED[1] and idle.min() >= LIMITED[2], (pub, held, idle)
    n_due, n_not = due.sum(0), ((run.active == 1) & (due == 0)).sum(0)
    assert n_due.min() >= GATED[0] and n_not.min() >= GATED[1], (n_due, n_not)
    assert run.T == 48 and any(any(w) for w in wire)


PINS = {
    # cfg: (bytes, sha256 of the records, sha256 of the packed buffer), recorded in front of the pixel format becoming an
    # argument of layout() and pack(): grey is what it was
    "px4-64": (104097, "ae0c9abd7440eebe5da015a39464aa483553098214b5dac60c38da23a5e43fa4",
               "dfe52d0826061f3be7cea473591e1d4cb5c49c9e799c5dfc69384a0a503ae43d"),
    "opencv-128": (70117, "32fb756cb5ac414093dec22e6b189405848803143b629e7198909d8578df06ea",
                   "c98e77ff909401b99360380ee0944340a72fbb660b77038b33aaee081ab736bc"),
}


@pytest.mark.parametrize("cfg", sorted(PINS))
def test_the_grey_layout_and_the_grey_buffer_are_pinned(cfg):
    w = 64 if cfg == "px4-64" else 128
    want_bytes, want_layout, want_buffer = PINS[cfg]
    recs, nbytes = sref.layout(*sref.TABLES[cfg], w, w)
    assert nbytes == want_bytes and hashlib.sha256(recs.tobytes()).hexdigest() == want_layout
    frames = np.random.default_rng(1).integers(0, 256, (len(recs), w, w), dtype=np.uint8)
    assert hashlib.sha256(sref.pack(recs, frames, nbytes, [5, 0]).tobytes()).hexdigest() == want_buffer
