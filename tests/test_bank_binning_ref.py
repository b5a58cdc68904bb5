"""The binning model and the inputs of the binning GPU tests, checked on the CPU (tests/bank_binning_ref.py): the model
against the level-1 image of npref.py and of the oracle, the hand-worked roundings, the packer against the model, and the
conditions the GPU tests' inputs have to meet, on the oracle's records."""
import numpy as np
import pytest

import bank_binning_ref as bref
import bank_pixels_ref as pref
import bank_sensors_ref as sref
import npref


def test_bin_2_is_the_level_1_image_of_npref_and_the_oracle(orc):
    rng = np.random.default_rng(3)
    for shape in ((64, 64), (128, 128), (6, 10)):
        plane = rng.integers(0, 256, shape, dtype=np.uint8)
        plane[:2, :4] = 255
        plane[2:4, :4] = 0
        got = bref.bin_plane(plane, 2)
        assert (got == npref.pyramid_down(plane)).all()
        assert (got == orc.pyramid_down(plane)).all()
    assert (bref.bin_plane(plane, 1) == plane).all()


def block(b, values):
    a = np.zeros(b * b, np.uint8)
    a[:len(values)] = values
    return a.reshape(b, b)


def test_hand_worked_roundings():
    for total, want in ((1, 0), (2, 1), (3, 1)):                 # (a + b + c + d + 2) >> 2
        assert bref.bin_plane(block(2, [1] * total), 2)[0, 0] == want
    assert bref.bin_plane(block(4, [1] * 7), 4)[0, 0] == 0       # (sum + 8) >> 4
    assert bref.bin_plane(block(4, [1] * 8), 4)[0, 0] == 1
    assert bref.bin_plane(np.full((4, 4), 255, np.uint8), 4)[0, 0] == 255 and 16 * 255 == 4080
    # quadrant sums 2, 2, 2, 1: one rounding of the sixteen-pixel sum gives 0, the 2 x 2 box applied twice gives 1
    quads = np.zeros((4, 4), np.uint8)
    quads[0, 0:2] = 1
    quads[0, 2:4] = 1
    quads[2, 0:2] = 1
    quads[2, 2] = 1
    assert [int(quads[y:y + 2, x:x + 2].sum()) for y in (0, 2) for x in (0, 2)] == [2, 2, 2, 1]
    assert bref.bin_plane(quads, 4)[0, 0] == 0
    assert bref.bin_plane(bref.bin_plane(quads, 2), 2)[0, 0] == 1


def test_the_rule_with_a_bin():
    w = h = 64
    for fmt, b in bref.COMBOS:
        bpp = pref.bpp_of(fmt)
        rec = sref.record(16, (5 + b * w) * bpp + 3, 5 + b * w, 3 + b * h, 5, 3)
        n = 16 + sref.extent(rec, fmt)
        assert bref.valid(rec, fmt, b, w, h, n) and not bref.valid(rec, fmt, b, w, h, n - 1)
        for bad in (0, 3, 8, 255):
            assert not bref.valid(rec, fmt, bad, w, h, n)
        for name in ("width", "height"):
            short = rec.copy()
            short[name] -= 1
            short["pitch"] = rec["pitch"]
            assert not bref.valid(short, fmt, b, w, h, n), (fmt, b, name)
        if b > 1:
            assert bref.valid(rec, fmt, b // 2, w, h, n) and not bref.valid(rec, fmt, 4, 2 * w, h, n)


@pytest.mark.parametrize("cfg,size", [("px4-64", 64), ("opencv-128", 128)])
def test_the_tables_hold_every_layout_and_bin_and_the_packer_gives_the_wanted_crops(cfg, size):
    rows, bins = bref.table(size, size)
    assert sorted(zip((r[5] for r in rows), bins.tolist())) == sorted(bref.COMBOS) and len(bref.COMBOS) == 9
    assert sorted(bref.ORDER) == list(range(bref.S)) and bref.COMBOS[bref.ORDER[-1]] == (pref.LUMA16_HI, 4)
    recs, fmts, nbytes = sref.layout(rows, bref.ORDER, size, size)
    for s in range(bref.S):
        assert bref.valid(recs[s], int(fmts[s]), int(bins[s]), size, size, nbytes), s
        assert recs[s]["pitch"] % 2 == 1 and recs[s]["x0"] % 2 == 1 and recs[s]["y0"] % 2 == 1
    last = bref.ORDER[-1]
    assert int(recs[last]["offset"]) + sref.extent(recs[last], int(fmts[last])) == nbytes, "a valid frame ends on the buffer's last byte"
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, (bref.S, size, size), dtype=np.uint8)
    frames[0, :8] = 255
    frames[1, :8] = 0
    buf = bref.pack(recs, fmts, bins, frames, nbytes, [1, 2])
    other = bref.pack(recs, fmts, bins, 255 - frames, nbytes, [1, 2])
    for s in range(bref.S):
        fmt, b = int(fmts[s]), int(bins[s])
        assert (bref.crop(buf, recs[s], fmt, b, size, size) == frames[s]).all(), s
        if b > 1:
            foot = bref.footprint(buf, recs[s], fmt, b, size, size).astype(int)
            blocks = foot.reshape(size, b, size, b)
            assert (blocks.max(axis=(1, 3)) != blocks.min(axis=(1, 3))).mean() > 0.9, "the pixels of a block differ"
            assert ((blocks.sum(axis=(1, 3)) - b * b * frames[s].astype(int)) != 0).mean() > 0.5, "sums off the exact multiple"
        if fmt != pref.GREY8:   # the other byte of each packed pixel is noise that does not depend on the frames
            start = int(recs[s]["offset"]) + int(recs[s]["y0"]) * int(recs[s]["pitch"]) + int(recs[s]["x0"]) * 2 + 1 - pref.phase_of(fmt)
            assert (buf[start:start + 2 * b * size:2] == other[start:start + 2 * b * size:2]).all()
    # the grey twin's sensors take the crops themselves
    grecs, gfmts, gbytes = sref.layout(bref.grey_table(size, size), list(range(bref.S)), size, size)
    assert all(sref.valid(grecs[s], size, size, gbytes) for s in range(bref.S)) and not gfmts.any()


@pytest.mark.parametrize("cfg", ["px4-64", "opencv-128"])
def test_every_stream_of_the_mixed_run_publishes_a_measured_flow(aof, orc, synth, cfg):
    """Conditions on the INPUT of the mixed-bank GPU tests, on the oracle's records: every stream publishes at least one
    record with quality > 0 and a non-zero pixel flow, and has due and not-due active frames; consecutive frames of a
    stream are whole-pixel translates of one texture (what sensor frames moving by bin times as many pixels bin to)."""
    p, run, want, wire, due, after, derot = bref.case(aof, orc, synth, cfg)
    assert (run.S, run.T) == (bref.S, bref.T)
    q = want["quality"]
    moved = (want["flow_x"] != 0) | (want["flow_y"] != 0)
    assert ((q > 0) & moved).any(axis=0).all(), ((q > 0) & moved).sum(axis=0)
    assert (q == aof.TICK_IDLE).any() and (q == aof.TICK_HELD).any()
    assert due.sum(0).min() >= 1 and ((run.active == 1) & (due == 0)).sum(0).min() >= 1, (due.sum(0),)
    assert all(len(w) > 0 for k in range(run.T) for s, w in enumerate(wire[k]) if q[k, s] >= 0)
