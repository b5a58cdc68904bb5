"""The reference side of the raw-mono-pixel tests (tests/bank_raw_ref.py), checked on the CPU: pack() followed by crop()
returns the plane for every format and bin and never depends on a bit that is no grey value, the tables carry the layouts
the GPU tests rely on, the library's rule -- the kernels' rule compiled for the host -- is the Python rule at every edge,
aof_bank_pixel_row_bytes and the centred helper answer as the header says, the tables and packed buffers are pinned by
sha256, and the oracle chain over the tables' crops publishes and holds within the ticks the GPU test runs."""
import numpy as np
import pytest

import bank_binning_ref as bref
import bank_pixels_ref as pref
import bank_raw_ref as rref
import bank_ref as ref
import bank_sensors_ref as sref

EINVAL = -22
FORMATS = sorted(rref.GROUPS)


@pytest.mark.parametrize("b", rref.BINS)
@pytest.mark.parametrize("fmt", FORMATS, ids=[rref.NAMES[f] for f in FORMATS])
def test_pack_then_crop_returns_the_plane(fmt, b):
    G, Bg, shift = rref.GROUPS[fmt]
    rng = np.random.default_rng([fmt, b])
    w, h, x0, y0 = 48, 20, 8, 3
    W, H = x0 + b * w + 4, y0 + b * h + 2
    plane = rng.integers(0, 256, (H, W), dtype=np.uint8)
    rb = rref.row_bytes(fmt, W)
    for pitch in (rb, rb + 7):
        buf = rref.pack(plane, fmt, pitch, 9)
        assert len(buf) == (H - 1) * pitch + rb
        rec = sref.record(0, pitch, W, H, x0, y0)
        assert rref.valid(rec, fmt, b, w, h, len(buf)) and not rref.valid(rec, fmt, b, w, h, len(buf) - 1)
        assert np.array_equal(rref.footprint(buf, rec, fmt, b, w, h), plane[y0:y0 + b * h, x0:x0 + b * w])
        assert np.array_equal(rref.crop(buf, rec, fmt, b, w, h), bref.bin_plane(plane[y0:y0 + b * h, x0:x0 + b * w], b))
        assert np.array_equal(rref.crop(buf, sref.record(0, pitch, W, H, 0, 0), fmt, 1, W, H), plane), "the whole sensor"
        # every bit that is no grey value is the seeded noise, whatever the plane holds: the same seed under another plane
        # differs in grey values only, and a buffer of the noise alone is restored by writing the plane into it
        noise = np.random.default_rng(9).integers(0, 256, len(buf), dtype=np.uint8)
        again = noise.copy()
        rref.put_grey(again, np.arange(H)[:, None] * pitch, fmt, np.arange(W)[None, :], plane)
        assert np.array_equal(again, buf)
        bits = np.zeros(len(buf), np.uint8)        # which bits of the buffer are grey values
        rref.put_grey(bits, np.arange(H)[:, None] * pitch, fmt, np.arange(W)[None, :], np.full((H, W), 255, np.uint8))
        assert int(np.unpackbits(bits).sum()) == 8 * H * W
        assert not ((buf ^ noise) & ~bits).any(), "no bit that is no grey value was written"
        assert (fmt == rref.GREY8 and pitch == rb) or (~bits).any(), "and there are such bits"
        if shift is not None:        # a 16-bit form read at any other shift is not the plane: the low bits and the bits above differ
            for other, (g2, b2, s2) in rref.GROUPS.items():
                if b2 == 2 and s2 != shift:
                    assert not np.array_equal(rref.crop(buf, rec, other, 1, w, h), plane[y0:y0 + h, x0:x0 + w]), (fmt, other)


def test_the_header_formulas_by_hand():
    """Four Y10P pixels in five bytes, two Y12P pixels in three, a Y10 / Y12 / Y14 word: the grey value is the top eight
    bits of the sample, truncated."""
    y10p = np.array([0x12, 0x34, 0x56, 0x78, 0xFF, 0x9A, 0xBC, 0xDE, 0xF0, 0xFF], np.uint8)
    assert rref.grey(y10p, 0, rref.Y10P, np.arange(8)).tolist() == [0x12, 0x34, 0x56, 0x78, 0x9A, 0xBC, 0xDE, 0xF0]
    y12p = np.array([0x12, 0x34, 0xFF, 0x56, 0x78, 0xFF], np.uint8)
    assert rref.grey(y12p, 0, rref.Y12P, np.arange(4)).tolist() == [0x12, 0x34, 0x56, 0x78]
    for fmt, bits in ((rref.Y10, 10), (rref.Y12, 12), (rref.Y14, 14)):
        for sample in (0, 1, (1 << bits) - 1, 0x2A5 << (bits - 10), 0x155 << (bits - 10)):
            word = sample | (0xFFFF << bits & 0xFFFF)                 # (bits above the sample set: never looked at)
            raw = np.array([word & 0xFF, word >> 8], np.uint8)
            assert int(rref.grey(raw, 0, fmt, 0)) == sample >> (bits - 8), (fmt, sample)
    word = np.array([0x34, 0x12], np.uint8)
    assert int(rref.grey(word, 0, rref.LUMA16_LO, 0)) == 0x34 and int(rref.grey(word, 0, rref.LUMA16_HI, 0)) == 0x12


@pytest.mark.parametrize("cfg", sorted(rref.SIZES))
def test_the_tables_carry_the_layouts_the_gpu_tests_rely_on(cfg):
    w, h = rref.SIZES[cfg]
    rows, bins, order = rref.table(cfg)
    recs, fmts, nbytes = rref.layout(rows, order, bins, w, h)
    assert len(rows) == rref.S and 8 <= rref.S <= 10 and sorted(order) == list(range(rref.S))
    assert set(rref.NEW) <= set(int(f) for f in fmts), "every new format"
    spans = sorted((int(r["offset"]), int(r["offset"]) + rref.extent(r, int(f))) for r, f in zip(recs, fmts))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == nbytes, "no overlap; the last frame ends the buffer"
    for s in range(rref.S):
        assert rref.valid(recs[s], int(fmts[s]), int(bins[s]), w, h, nbytes), s
    pitches = [(int(r["pitch"]), rref.row_bytes(int(f), int(r["width"]))) for r, f in zip(recs, fmts)]
    assert any(p == m for p, m in pitches) and any(p > m and p % 2 == 0 for p, m in pitches) and any(p % 2 == 1 for p, m in pitches), \
        "a tight, a padded and an odd pitch"
    assert {0, 1, 7, 8} <= set(int(r["offset"]) % 16 for r in recs)
    assert any(int(r["x0"]) + b * w == int(r["width"]) and int(r["y0"]) + b * h == int(r["height"]) and int(f) in rref.NEW and s != order[-1]
               for s, (r, f, b) in enumerate(zip(recs, fmts, bins))), "a crop touches the right and bottom edge"
    combos = set(zip(fmts.tolist(), bins.tolist()))
    assert {(rref.Y10P, 2), (rref.Y12, 2), (rref.Y10, 4)} <= combos
    last = order[-1]
    assert fmts[last] == rref.Y10P and bins[last] == 1 and (int(recs[last]["width"]), int(recs[last]["height"])) == (w, h)
    assert (int(recs[last]["x0"]), int(recs[last]["y0"])) == (0, 0) and int(recs[last]["pitch"]) == w // 4 * 5
    assert int(recs[last]["offset"]) + rref.extent(recs[last], rref.Y10P) == nbytes and not rref.valid(recs[last], rref.Y10P, 1, w, h, nbytes - 1), \
        "camera_bytes ends on the last frame's last low-bits byte"
    frames = np.random.default_rng(3).integers(0, 256, (rref.S, h, w), dtype=np.uint8)
    buf = rref.pack_buffer(recs, fmts, bins, frames, nbytes, [5, 0])
    for s in range(rref.S):
        assert np.array_equal(rref.crop(buf, recs[s], int(fmts[s]), int(bins[s]), w, h), frames[s]), s


def agree(aof, rec, fmt, b, w, h, nbytes, base=0):
    want = rref.valid(rec, fmt, b, w, h, nbytes, base)
    got = aof.bank_sensor_valid(rec, w, h, nbytes, base, format=fmt, bin=b)
    assert got == want, (rec, fmt, b, w, h, nbytes, base, got, want)
    if b == 1:
        assert aof.bank_sensor_valid(rec, w, h, nbytes, base, format=fmt) == want, "bin 1 decides as the call without a bin"
        if fmt in pref.FORMATS:
            assert want == pref.valid(rec, fmt, w, h, nbytes, base), "the older formats keep their rule"
    return want


def test_the_librarys_rule_is_the_python_rule_at_every_edge(aof):
    """The edge grid of test_bank_pixels_ref.py for formats 0..9 and 255."""
    top, big = (1 << 64) - 1, (1 << 31) - 1
    recs = [(100, 176, 80, 72, 16, 8), (100, 160, 80, 72, 16, 8), (100, 159, 80, 72, 16, 8), (100, 88, 80, 72, 16, 8), (100, 80, 80, 72, 16, 8),
            (100, 79, 80, 72, 16, 8), (100, 176, 80, 72, 17, 8), (100, 176, 80, 72, 16, 9), (100, 176, 80, 72, -1, 8), (100, 176, 80, 72, 16, -1),
            (100, 176, 0, 72, 0, 0), (100, 176, 80, 0, 0, 0), (0, 128, 64, 64, 0, 0), (0, 127, 64, 64, 0, 0),
            (top, 176, 80, 72, 16, 8), (top - 12656 + 100, 176, 80, 72, 16, 8), (top - 12656 + 101, 176, 80, 72, 16, 8),
            (5, big, 64, big, 0, 0), (5, big, big // 2, big, 0, 0), (5, big, big // 2 + 1, big, 0, 0), (100, big, big, 72, big - 63, 8),
            (100, 176, 80, 72, big, 8),
            # additions: pitch at Y10P's and Y12P's row_bytes of 80 pixels (100, 120) and one less; width and x0 one off a group
            (100, 100, 80, 72, 16, 8), (100, 99, 80, 72, 16, 8), (100, 120, 80, 72, 16, 8), (100, 119, 80, 72, 16, 8),
            (100, 176, 81, 72, 16, 8), (100, 176, 82, 72, 16, 8), (100, 176, 84, 72, 18, 8), (100, 176, 84, 72, 20, 8)]
    tall = (big - 1) * big
    # 71 * 176 + row_bytes + 100: 12756 (160), 12696 (100), 12716 (120), 12676 (80)
    sizes = [0, 1, 8191, 8192, 12755, 12756, 12757, 12695, 12696, 12715, 12716, 12675, 12676, 6427, 6428, 1 << 40, 4 + tall + 128, 5 + tall + 128,
             5 + tall + 64, 5 + tall + 2 * (big // 2), top - 1, top]
    bases = [0, 1, 500, top - 12756, top - 12755, top - tall - 133, top - tall - 134, top]
    checked = valid = 0
    for r in recs:
        rec = sref.record(*r)
        for fmt in list(range(10)) + [255]:
            for nbytes in sizes:
                for base in bases:
                    want = agree(aof, rec, fmt, 1, 64, 64, nbytes, base)
                    checked, valid = checked + 1, valid + want
    assert valid > 400 and checked - valid > 5000, (valid, checked)


@pytest.mark.parametrize("fmt", list(range(10)) + [255])
def test_the_rule_at_the_edges_the_groups_add(aof, fmt):
    """width % G and x0 % G at 0 and 1, pitch == row_bytes and one less, the extent equal to camera_bytes and one byte
    short -- for every bin byte the rule knows and one it does not."""
    w = h = 64
    G, Bg = rref.GROUPS[fmt][:2] if fmt in rref.GROUPS else (1, 1)
    known = fmt in rref.GROUPS
    for b in (1, 2, 4, 3):
        foot = (b if b != 3 else 1) * w
        width, height, x0, y0 = foot + 12, foot + 5, 8, 5
        rb = width // G * Bg
        for pitch in (rb, rb + 5):
            rec = sref.record(48, pitch, width, height, x0, y0)
            n = 48 + (height - 1) * pitch + rb
            assert agree(aof, rec, fmt, b, w, h, n) == (known and b in rref.BINS)
            assert not agree(aof, rec, fmt, b, w, h, n - 1)
            assert agree(aof, rec, fmt, b, w, h, n + 4096, base=4096) == (known and b in rref.BINS)
            assert not agree(aof, rec, fmt, b, w, h, n + 4095, base=4096)
            for name, value, still in (("x0", x0 + 1, G == 1), ("x0", x0 + 4, True), ("x0", x0 + 5, False), ("width", width + 1, G == 1),
                                       ("width", width + G, True), ("pitch", rb - 1, False), ("y0", y0 + 1, False)):
                edge = rec.copy()
                edge[name] = value
                got = agree(aof, edge, fmt, b, w, h, 1 << 40)
                assert got == (still and known and b in rref.BINS and (name != "width" or pitch >= (value // G) * Bg)), (fmt, b, name, value)


def test_row_bytes_of_the_tables_and_at_its_edges(aof):
    for cfg in rref.SIZES:
        rows, bins, order = rref.table(cfg)
        for width, height, pitch, mod, origin, fmt in rows:
            assert aof.bank_pixel_row_bytes(fmt, width) == rref.row_bytes(fmt, width) <= pitch
    top = 2 ** 31 - 1
    assert aof.bank_pixel_row_bytes(rref.Y10P, top - 3) == (top - 3) // 4 * 5 and aof.bank_pixel_row_bytes(rref.Y14, top) == 2 * top
    for fmt, width in ((rref.Y10P, top), (rref.Y10P, 2), (rref.Y12P, 1), (rref.Y10, 0), (3, 64), (9, 64), (255, 64)):
        with pytest.raises(aof.AofError):
            aof.bank_pixel_row_bytes(fmt, width)


def test_the_centred_helper_rounds_x0_down_to_a_group(aof):
    p = aof.px4flow_params(64, 64)
    for fmt in FORMATS:
        G = rref.GROUPS[fmt][0]
        for b in rref.BINS:
            for width in (328, 330, 332, 334):           # width / 2 - 32 b: 132, 133, 134, 135 (minus 0, 32, 96)
                if width % G:
                    with pytest.raises(aof.AofError):
                        aof.bank_sensor_centred(p, 4096, 2 * width, width, 267, format=fmt, bin=b)
                    continue
                pitch = rref.row_bytes(fmt, width) + 3
                rec = aof.bank_sensor_centred(p, 4096, pitch, width, 267, format=fmt, bin=b)
                centre = width // 2 - (b * 64) // 2
                assert int(rec["x0"]) == centre - centre % G and int(rec["y0"]) == 267 // 2 - (b * 64) // 2, (fmt, b, width)
                assert (int(rec["offset"]), int(rec["pitch"]), int(rec["width"]), int(rec["height"])) == (4096, pitch, width, 267)
                assert rref.valid(rec, fmt, b, 64, 64, 4096 + rref.extent(rec, fmt))
    assert any(((w // 2 - 32) % 4, (w // 2 - 32) % 2) == (3, 1) for w in (328, 330, 332, 334)), "an x0 that has to move for both packed forms"
    with pytest.raises(aof.AofError):
        aof.bank_sensor_centred(p, 0, rref.row_bytes(rref.Y10P, 328) - 1, 328, 267, format=rref.Y10P)


PINS = {
    # cfg: (bytes, sha256 of records + formats + bins, sha256 of the packed buffer of seeded frames)
    "px4-64": (260113, "e2b41ce8be6cb68be05af8bc0c33a8abdd9be2a8cee5790fb8077aa803576708",
               "16369c9627ed3304c7bf94c9d4e3e6d417a5d3525f5b52452bf9dc933d32b7b0"),
    "opencv-128": (980881, "b6c59243655684bd648e7611110ab920132080d6c783a2d2cb77ea5d2889a575",
                   "f6c0ff610e65bfd8008aca43bd2a210bce126b641396db15e9e067792540f1cb"),
}


@pytest.mark.parametrize("cfg", sorted(PINS))
def test_the_tables_and_the_packed_buffers_are_pinned(cfg):
    w, h = rref.SIZES[cfg]
    rows, bins, order = rref.table(cfg)
    recs, fmts, nbytes = rref.layout(rows, order, bins, w, h)
    frames = np.random.default_rng(1).integers(0, 256, (len(recs), h, w), dtype=np.uint8)
    got = (nbytes, rref.sha(recs.tobytes() + fmts.tobytes() + bins.tobytes()), rref.sha(rref.pack_buffer(recs, fmts, bins, frames, nbytes, [5, 0])))
    assert fmts.dtype == np.uint8 and bins.dtype == np.uint8
    assert got == PINS[cfg], got


@pytest.mark.parametrize("cfg", sorted(rref.SIZES))
def test_the_oracle_chain_publishes_and_holds_within_the_ticks_the_gpu_test_runs(aof, orc, synth, cfg):
    """A condition on the INPUT: every stream's chain over its crops has a record with quality > 0 and an AOF_TICK_HELD one
    within ticks 0..9 and the burst's ticks 12..14 -- a bank whose limiter never holds or never publishes cannot tell a
    wrong crop from a right one in the records."""
    p, run, want, wire = rref.case(aof, orc, synth, cfg)
    assert (run.S, run.T) == (rref.S, rref.T) and not run.active[rref.TICKS:rref.BURST * rref.K].any()
    ticks = list(range(rref.TICKS)) + list(range(rref.BURST * rref.K, rref.BURST * rref.K + rref.K))
    q = want["quality"][ticks]
    assert ((q > 0).sum(0) >= 1).all() and ((q == ref.TICK_HELD).sum(0) >= 1).all(), ((q > 0).sum(0), (q == ref.TICK_HELD).sum(0))
    assert any(len(f) for k in ticks for f in wire[k]), "wire frames are sent"
    burst = run.active[rref.BURST * rref.K:rref.BURST * rref.K + rref.K]
    assert burst.any() and (burst.cumprod(axis=0) == burst).all(), "the burst's frames are every stream's leading rounds"
