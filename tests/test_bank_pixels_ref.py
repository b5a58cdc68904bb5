"""The reference side of the packed-pixel tests (tests/bank_pixels_ref.py), checked on the CPU: the byte-by-byte crop is
plain numpy slicing, the packer's crops are the run's frames, the inputs can tell a wrong phase and a forgotten bpp from
the right crop, the tables carry the layouts the GPU tests rely on, the library's aof_bank_sensor_valid_format -- the
kernels' rule compiled for the host -- is the Python rule at every edge, and the packed layouts and buffers are pinned by
sha256."""
import hashlib

import numpy as np
import pytest

import bank_pixels_ref as pref
import bank_ref as ref
import bank_sensors_ref as sref

EINVAL = -22
SIZE = {"px4-64": 64, "opencv-128": 128}


def sliced(buf, rec, fmt, w, h):
    bpp, phase = pref.bpp_of(fmt), pref.phase_of(fmt)
    start, pitch, x0, y0 = (int(rec[n]) for n in ("offset", "pitch", "x0", "y0"))
    rows = [buf[start + (y0 + y) * pitch + x0 * bpp:start + (y0 + y) * pitch + (x0 + w) * bpp] for y in range(h)]
    return np.stack(rows) if bpp == 1 else np.stack([r[phase::2] for r in rows])


@pytest.mark.parametrize("cfg", sorted(pref.TABLES))
def test_the_model_is_numpy_slicing_and_the_packers_crops_are_the_runs_frames(synth, cfg):
    S, seed = sref.CASES[cfg]
    w = SIZE[cfg]
    table, order = pref.TABLES[cfg]
    recs, fmts, nbytes = pref.layout(table, order, w, w)
    run = ref.make_run(synth, w, w, S, 2, seed)
    for k in range(2):
        buf = pref.pack(recs, run.frames[k], nbytes, [seed, k], fmts)
        noise = np.random.default_rng([seed, k]).integers(0, 256, nbytes, dtype=np.uint8)
        for s in range(S):
            fmt = int(fmts[s])
            got = pref.crop(buf, recs[s], fmt, w, w)
            assert np.array_equal(got, sliced(buf, recs[s], fmt, w, w)), (k, s)
            assert np.array_equal(got, run.frames[k, s]), (k, s)
            assert pref.valid(recs[s], fmt, w, w, nbytes)
            if fmt != pref.GREY8:      # the other byte of every pixel of the crop is the seeded noise, whatever the frame holds
                other = pref.LUMA16_HI if fmt == pref.LUMA16_LO else pref.LUMA16_LO
                assert np.array_equal(pref.crop(buf, recs[s], other, w, w), pref.crop(noise, recs[s], other, w, w)), (k, s)


@pytest.mark.parametrize("cfg", sorted(pref.TABLES))
def test_the_inputs_tell_a_wrong_phase_and_a_forgotten_bpp_from_the_right_crop(synth, cfg):
    S, seed = sref.CASES[cfg]
    w = SIZE[cfg]
    recs, fmts, nbytes = pref.layout(*pref.TABLES[cfg], w, w)
    run = ref.make_run(synth, w, w, S, 1, seed)
    buf = np.concatenate([pref.pack(recs, run.frames[0], nbytes, seed, fmts), np.zeros(2 * w * w, np.uint8)])   # (room for the wrong reads)
    for s in range(S):
        fmt = int(fmts[s])
        right = pref.crop(buf, recs[s], fmt, w, w)
        for wrong in pref.FORMATS:
            if wrong == fmt:
                continue
            if wrong != pref.GREY8 and fmt == pref.GREY8 and not pref.valid(recs[s], wrong, w, w, len(buf)):
                continue       # (a grey record read as packed pixels would leave its rows: the rule refuses it)
            start = int(recs[s]["offset"]) + int(recs[s]["y0"]) * int(recs[s]["pitch"])
            x0, pitch, bpp, phase = int(recs[s]["x0"]), int(recs[s]["pitch"]), pref.bpp_of(wrong), pref.phase_of(wrong)
            got = np.stack([buf[start + y * pitch + x0 * bpp + phase:start + y * pitch + (x0 + w) * bpp + phase:bpp] for y in range(w)])
            assert not np.array_equal(got, right), (s, fmt, wrong)


def test_the_tables_carry_the_layouts_the_gpu_tests_rely_on():
    residues, packed_pitches = set(), []
    for cfg, (table, order) in pref.TABLES.items():
        w = SIZE[cfg]
        recs, fmts, nbytes = pref.layout(table, order, w, w)
        assert set(int(f) for f in fmts) == set(pref.FORMATS), cfg
        assert [t[:2] + t[3:5] for t in table] == [t[:2] + t[3:5] for t in sref.TABLES[cfg][0]], "bank_sensors_ref's cameras"
        spans = sorted((int(r["offset"]), int(r["offset"]) + pref.extent(r, int(f))) for r, f in zip(recs, fmts))
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == nbytes, "no overlap; the last frame ends the buffer"
        last = order[-1]
        assert fmts[last] != pref.GREY8 and not pref.valid(recs[last], int(fmts[last]), w, w, nbytes - 1)
        for s, t in enumerate(table):
            residues.add(int(recs[s]["offset"]) % 16)
            if t[5] != pref.GREY8:
                packed_pitches.append((t[2], 2 * t[0]))
        assert any(int(f) != pref.GREY8 and int(r["x0"]) + w == int(r["width"]) and int(r["y0"]) + w == int(r["height"])
                   for r, f in zip(recs, fmts)), "a packed crop touches the right and bottom edges"
        grey, grey_bytes = pref.grey_twin(table, order, w, w)
        for n in ("width", "height", "x0", "y0"):
            assert grey[n].tolist() == recs[n].tolist(), n
    assert {0, 1, 7, 8} <= residues
    assert any(p % 2 == 1 for p, _ in packed_pitches) and any(p > m and p % 2 == 0 for p, m in packed_pitches) \
        and any(p == m for p, m in packed_pitches), "an odd, a padded and a tight packed pitch"
    px4 = pref.layout(*pref.TABLES["px4-64"], 64, 64)
    last = pref.ORDER["px4-64"][-1]
    assert px4[1][last] == pref.LUMA16_HI and px4[0][last]["width"] == 64 and px4[0][last]["height"] == 64, \
        "the buffer's last byte is the grey byte of the last frame's last pixel"


def test_the_librarys_rule_with_a_format_is_the_python_rule_at_every_edge(aof):
    """aof_bank_sensor_valid_format against bank_pixels_ref.valid: every inequality at equality and one beyond, pitch ==
    2 * width and one less, the extent equal to camera_bytes and one byte short, format 3, width and height near 2^31,
    offsets near 2^64, bases that would wrap a careless sum."""
    top, big = (1 << 64) - 1, (1 << 31) - 1
    # the packed extent of (100, 176, 80, 72, ...): 71 * 176 + 160 = 12656
    recs = [(100, 176, 80, 72, 16, 8), (100, 160, 80, 72, 16, 8), (100, 159, 80, 72, 16, 8), (100, 88, 80, 72, 16, 8), (100, 80, 80, 72, 16, 8),
            (100, 79, 80, 72, 16, 8), (100, 176, 80, 72, 17, 8), (100, 176, 80, 72, 16, 9), (100, 176, 80, 72, -1, 8), (100, 176, 80, 72, 16, -1),
            (100, 176, 0, 72, 0, 0), (100, 176, 80, 0, 0, 0), (0, 128, 64, 64, 0, 0), (0, 127, 64, 64, 0, 0),
            (top, 176, 80, 72, 16, 8), (top - 12656 + 100, 176, 80, 72, 16, 8), (top - 12656 + 101, 176, 80, 72, 16, 8),
            (5, big, 64, big, 0, 0), (5, big, big // 2, big, 0, 0), (5, big, big // 2 + 1, big, 0, 0), (100, big, big, 72, big - 63, 8),
            (100, 176, 80, 72, big, 8)]
    tall = (big - 1) * big
    sizes = [0, 1, 8191, 8192, 12755, 12756, 12757, 6427, 6428, 1 << 40, 4 + tall + 128, 5 + tall + 128, 5 + tall + 64, 5 + tall + 2 * (big // 2),
             top - 1, top]
    bases = [0, 1, 500, top - 12756, top - 12755, top - tall - 133, top - tall - 134, top]
    checked = valid = 0
    for r in recs:
        rec = sref.record(*r)
        for fmt in (0, 1, 2, 3, 255):
            for nbytes in sizes:
                for base in bases:
                    want = pref.valid(rec, fmt, 64, 64, nbytes, base)
                    assert aof.bank_sensor_valid(rec, 64, 64, nbytes, base, format=fmt) == want, (r, fmt, nbytes, base)
                    if fmt == 0:
                        assert want == sref.valid(rec, 64, 64, nbytes, base), "format 0 is the rule without a format"
                    checked, valid = checked + 1, valid + want
    assert valid > 150 and checked - valid > 2000
    good = sref.record(100, 160, 80, 72, 16, 8)
    for fmt in (1, 2):
        assert pref.valid(good, fmt, 64, 64, 100 + 71 * 160 + 160) and not pref.valid(good, fmt, 64, 64, 100 + 71 * 160 + 159)
        assert not pref.valid(sref.record(100, 159, 80, 72, 16, 8), fmt, 64, 64, 1 << 40)
    assert not pref.valid(good, 3, 64, 64, 1 << 40) and pref.valid(good, 0, 64, 64, 1 << 40)
    assert aof.lib.aof_bank_sensor_valid_format(None, 1, 64, 64, 0, 1) == EINVAL


PINS = {
    # cfg: (bytes, sha256 of the records and the formats, sha256 of the packed buffer), recorded from bank_pixels_ref's own
    # layout() and pack() in front of their merge into bank_sensors_ref's
    "px4-64": (131441, "8a4bedbdba5247aa7db2d6e2da62c64d7b32f1d6cbf1a374548c3de83a4878a1",
               "fb2cc0069eebb6e409c7e10b39cfb63aa31f848f8c328f3324d28ae307f8516d"),
    "opencv-128": (119688, "66d3382ceb2f434bb4d045a9db8a08aa78cf9933d9f80078820c41045b1716f6",
                   "392ea56223742d73048b06af1e8e5b27be99aadf46f86ede820489f556915a5f"),
}


@pytest.mark.parametrize("cfg", sorted(PINS))
def test_the_packed_layout_and_the_packed_buffer_are_pinned(cfg):
    w = SIZE[cfg]
    want_bytes, want_layout, want_buffer = PINS[cfg]
    recs, fmts, nbytes = pref.layout(*pref.TABLES[cfg], w, w)
    assert fmts.dtype == np.uint8 and nbytes == want_bytes
    assert hashlib.sha256(recs.tobytes() + fmts.tobytes()).hexdigest() == want_layout
    frames = np.random.default_rng(1).integers(0, 256, (len(recs), w, w), dtype=np.uint8)
    assert hashlib.sha256(pref.pack(recs, frames, nbytes, [5, 0], fmts).tobytes()).hexdigest() == want_buffer
