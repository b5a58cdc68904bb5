"""The stream bank with raw mono pixels (include/aof.h "raw mono pixels": AOF_PIXEL_Y10, _Y12, _Y14, _Y10P, _Y12P): ten
streams whose sensor buffers hold 16-bit words and MIPI-packed groups full of noise around the grey values, against a twin
bank on grey sensors that hold the planes the numpy model reads out of those buffers -- by bytes, never by tolerance.  Ticks
and a burst, a mixed bank against banks of one, invalid records, a format rewritten between ticks, the stateless ingest on
its vector and its per-pixel path, and the facade.  The model, the tables and the packer: tests/bank_raw_ref.py (checked
on the CPU: tests/test_bank_raw_ref.py); the rigs: tests/bank_sensor_rig.py.  Every camera buffer
is allocated with more than 64 bytes of slack behind camera_bytes."""

import numpy as np
import pytest

import bank_camera_ref as cref
import bank_raw_ref as rref
import bank_ref as ref
import bank_sensors_ref as sref
import ingest_ref
from bank_ref import FX, FY
from bank_rig import EINVAL, OFFSET, Guarded, put, same, same_records, untouched, up
from bank_sensor_rig import SLACK, GreyTwin, RawRig, same_rigs, table_tensor
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

S = rref.S
assert SLACK >= 64


def setup(aof, synth, orc, cfg, path, n=2):
    p, run, want, wire = rref.case(aof, orc, synth, cfg)
    cam = aof.bank_camera_params(*sref.SCALARS[cfg], p.width, p.height, 0, rref.INTERVAL, cref.DEROTATE, FX, FY)   # (scalars no stream has)
    bp = aof.bank_params(run.S, FX, FY, rref.RATE, OFFSET, 1, 100, 0)
    engs = [aof.FlowEngine(p, 0) for _ in range(n)]
    for e in engs:
        e.set_bank_path(path)
    return p, run, cam, bp, engs


# ---- 1. contract (a): against the grey twin on the model's planes, ten ticks and a burst ----

@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("cfg", ["px4-64", "opencv-128"])
def test_a_raw_bank_leaves_the_bytes_of_a_grey_bank_on_the_models_planes(aof, orc, synth, gpu_device, cfg, path):
    """Records, wire frames and lengths, exposure records, de-rotated pairs (the rigs' outputs), the bank's frames and state
    regions and the gates, after every tick and after the burst of K = 3 on the same banks; the ticks' records and wire
    frames against the oracle chain as well."""
    p, run, want, wire = rref.case(aof, orc, synth, cfg)
    _, _, cam, bp, (ea, eb) = setup(aof, synth, orc, cfg, path)
    a = RawRig(aof, ea, run, bp, gpu_device, cam, cfg)
    b = GreyTwin(aof, eb, run, bp, gpu_device, cam, a)
    a.bind(), b.bind()
    assert a.alloc.numel() - 1 - a.camera_bytes >= 64, "slack behind camera_bytes"
    for k in range(rref.TICKS):
        a.load(k), a.enqueue()
        assert (a.crops[0] == run.frames[k]).all(), "the model reads the run's frames out of the buffer"
        b.load(k), b.enqueue()
        same_rigs(a, b, (cfg, path, "tick", k))
        got = a.read()
        same_records(got.recs, want[k], k, "oracle")
        assert got.wire == wire[k], ("oracle wire", k)
    K = rref.K
    ka = RawRig(aof, ea, run, bp, gpu_device, cam, cfg, K=K, pad=37, bank=a.bank)
    kb = GreyTwin(aof, eb, run, bp, gpu_device, cam, ka, K=K, pad=5, bank=b.bank)
    given = rref.burst_counts(run)
    assert given[rref.BURST].max() == K and len(set(given[rref.BURST].tolist())) > 1, "mixed counts"
    ka.bind(), kb.bind()
    ka.load(rref.BURST, given), ka.enqueue()
    kb.load(rref.BURST, given), kb.enqueue()
    same_rigs(ka, kb, (cfg, path, "burst"))
    rounds = ka.read()
    for r in range(K):
        same_records(rounds[r].recs, want[rref.BURST * K + r], r, "oracle, burst")
        assert rounds[r].wire == wire[rref.BURST * K + r], ("oracle wire, burst", r)
    ea.close(), eb.close()


# ---- 2. the mixed bank: every stream against its bank of one ----

def mixed_table(cfg):
    """Grey, LUMA16_LO, the five new formats and the three binned streams of the configuration's table in one buffer."""
    w, h = rref.SIZES[cfg]
    rows, bins, order = rref.table(cfg)
    rows = [(w + 9, h + 7, w + 11, 7, (5, 3), rref.GREY8), (w + 7, h + 4, 2 * (w + 7) + 1, 8, (7, 2), rref.LUMA16_LO)] + rows[:8]
    return rows, np.concatenate([[1, 1], bins[:8]]).astype(np.uint8), [2, 0, 7, 3, 9, 1, 4, 5, 8, 6]


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("cfg", ["px4-64", "opencv-128"])
def test_every_stream_of_a_mixed_bank_is_its_bank_of_one(aof, orc, synth, gpu_device, cfg, path):
    T = 6
    p, run, cam, bp, (ea,) = setup(aof, synth, orc, cfg, path, n=1)
    rows, bins, order = mixed_table(cfg)
    assert sorted(set(r[5] for r in rows)) == [0, 1, 4, 5, 6, 7, 8] and sorted(bins.tolist())[-3:] == [2, 2, 4]
    a = RawRig(aof, ea, run, bp, gpu_device, cam, cfg, table=(rows, bins, order))
    a.bind()
    bp1 = aof.bank_params(1, FX, FY, rref.RATE, OFFSET, 1, 100, 0)
    ones = []
    for s in range(S):
        e = aof.FlowEngine(p, 0)
        e.set_bank_path(path)
        one_run = ref.Run(run.frames[:, s:s + 1], run.times[:, s:s + 1], run.gyro[:, s:s + 1], run.active[:, s:s + 1])
        r = RawRig(aof, e, one_run, bp1, gpu_device, cam, cfg, table=([rows[s]], bins[s:s + 1], [0]), seed=40 + s)
        r.bind()
        ones.append(r)
    px = p.width * p.height
    served = 0
    for k in range(T):
        got = a.push(k)
        frames, state = a.bank.frames_bytes(), a.bank.state_bytes()
        for s, r in enumerate(ones):
            one = r.push(k)
            what = (cfg, path, k, s, rref.NAMES[rows[s][5]], int(bins[s]))
            assert got.recs[s:s + 1].tobytes() == one.recs.tobytes(), ("record",) + what
            assert got.wire[s] == one.wire[0], ("wire frame",) + what
            assert got.exposure[s:s + 1].tobytes() == one.exposure.tobytes(), ("exposure record",) + what
            assert got.derotated.reshape(S, -1)[s].tobytes() == one.derotated.reshape(-1).tobytes(), ("de-rotated pair",) + what
            assert frames[s * px:(s + 1) * px].tobytes() == r.bank.frames_bytes()[:px].tobytes(), ("stored frame",) + what
            assert state[s].tobytes() == r.bank.state_bytes()[0].tobytes(), ("state",) + what
            served += int(run.active[k, s])
    assert served > 3 * S
    for r in ones:
        r.eng.close()
    ea.close()


# ---- 3. invalid records, one per stream in one tick ----

def invalid_cases(rig):
    """(what, stream, record or None, format or None): seven streams, each with one thing wrong."""
    edit = lambda s, **kw: sref.record(*[kw.get(n, int(rig.recs[s][n])) for n in ("offset", "pitch", "width", "height", "x0", "y0")])
    fmt = lambda s: int(rig.layout_formats[0][s])
    assert (fmt(3), fmt(4), fmt(0), fmt(9)) == (rref.Y10P, rref.Y12P, rref.Y10, rref.Y10P)
    return [("x0 % G == 1", 3, edit(3, x0=int(rig.recs[3]["x0"]) - 3), None),
            ("width % G != 0", 4, edit(4, width=int(rig.recs[4]["width"]) + 1), None),
            ("pitch == row_bytes - 1", 0, edit(0, pitch=rref.row_bytes(rref.Y10, int(rig.recs[0]["width"])) - 1), None),
            ("a frame ending one byte behind camera_bytes", 9, edit(9, offset=int(rig.recs[9]["offset"]) + 1), None),
            ("format 3", 1, None, 3), ("format 9", 2, None, 9), ("format 255", 8, None, 255)]


@pytest.mark.parametrize("path", [1, 2])
def test_invalid_records_make_their_streams_idle_with_their_own_quality(aof, orc, synth, gpu_device, path):
    """Ticks 0..9 on twin banks: in one tick seven streams of A have an invalid record or format, in C those streams are
    inactive in that tick.  A's outputs are C's but for the quality of those records, the banks are equal after every tick
    -- the stored frames and states of the refused streams untouched --, and behind the repair the streams go on as ones
    that were idle meanwhile."""
    cfg = "px4-64"
    p, run, cam, bp, (ea, ec) = setup(aof, synth, orc, cfg, path)
    a, c = (RawRig(aof, e, run, bp, gpu_device, cam, cfg) for e in (ea, ec))
    a.bind(), c.bind()
    cases = invalid_cases(a)
    streams = [s for _, s, _, _ in cases]
    assert int(a.recs[9]["offset"]) + rref.extent(a.recs[9], rref.Y10P) == a.camera_bytes
    for what, s, bad, bad_fmt in cases:
        f, b = int(a.layout_formats[0][s]), int(a.host_bins[s])
        assert rref.valid(a.recs[s], f, b, 64, 64, a.camera_bytes), what
        assert not rref.valid(a.recs[s] if bad is None else bad, f if bad_fmt is None else bad_fmt, b, 64, 64, a.camera_bytes), what
    assert (int(cases[0][2]["x0"]) % 4, int(cases[1][2]["width"]) % 2) == (1, 1)
    kb = next(k for k in range(3, rref.TICKS - 1) if run.active[k, streams].all())
    assert all(run.active[:kb, s].any() and run.active[kb + 1:rref.TICKS, s].any() for s in streams), "frames in front of and behind the tick"
    px = p.width * p.height
    for k in range(rref.TICKS):
        if k == kb:
            for what, s, bad, bad_fmt in cases:
                if bad is not None:
                    put(a.table, s, bad)
                if bad_fmt is not None:
                    a.put_format(s, bad_fmt, host=False)
        a.load(k), c.load(k)
        if k == kb:
            for s in streams:
                c.select[s] = 0
            before_frames, before_state = a.bank.frames_bytes().copy(), a.bank.state_bytes().copy()
        a.enqueue(), c.enqueue()
        ga, gc = a.read(), c.read()
        if k == kb:
            for what, s, bad, bad_fmt in cases:
                assert ga.recs[s]["quality"] == aof.TICK_BAD_SENSOR and gc.recs[s]["quality"] == aof.TICK_IDLE, (what, ga.recs[s])
                idle = np.zeros((), ga.recs.dtype)
                idle["quality"] = aof.TICK_BAD_SENSOR
                assert ga.recs[s].tobytes() == idle.tobytes() and ga.wire[s] == b"", (what, "idle outputs")
                ga.recs[s]["quality"] = aof.TICK_IDLE
                assert a.bank.frames_bytes()[s * px:(s + 1) * px].tobytes() == before_frames[s * px:(s + 1) * px].tobytes(), (what, "the stored frame")
                assert a.bank.state_bytes()[s].tobytes() == before_state[s].tobytes(), (what, "the state")
                put(a.table, s, a.recs[s]), a.put_format(s, int(a.layout_formats[0][s]), host=False)
            others = [s for s in range(S) if s not in streams and run.active[k, s]]
            assert others and all(ga.recs[s]["quality"] != aof.TICK_BAD_SENSOR for s in others), "the other streams are served"
        same_records(ga.recs, gc.recs, k, "invalid records")
        assert ga.wire == gc.wire and ga.exposure.tobytes() == gc.exposure.tobytes(), k
        assert ga.derotated.tobytes() == gc.derotated.tobytes(), k
        assert a.bank_bytes() == c.bank_bytes() and a.gate_bytes().tolist() == c.gate_bytes().tolist(), k
    ea.close(), ec.close()


# ---- 4. the format array rewritten between two eager ticks ----

@pytest.mark.parametrize("path", [1, 2])
def test_a_format_rewritten_between_ticks_decodes_by_the_new_byte(aof, orc, synth, gpu_device, path):
    """Stream 0 delivers Y10 up to tick 3 and Y10P from tick 4 on, its buffer repacked (the same sensor: 96 pixels are 24
    groups, and a Y10P row fits the Y10 pitch); the byte is rewritten on the stream between the ticks.  Equal to the grey
    twin on the model's planes in every tick."""
    cfg, s, at = "px4-64", 0, 4
    p, run, cam, bp, (ea, eb) = setup(aof, synth, orc, cfg, path)
    a = RawRig(aof, ea, run, bp, gpu_device, cam, cfg)
    b = GreyTwin(aof, eb, run, bp, gpu_device, cam, a)
    a.bind(), b.bind()
    assert int(a.host_formats[s]) == rref.Y10 and rref.valid(a.recs[s], rref.Y10P, 1, 64, 64, a.camera_bytes)
    assert run.active[at - 2:at, s].all() and run.active[at:at + 2, s].all(), "a pair on either side of the rewrite"
    for k in range(8):
        if k == at:
            a.put_format(s, rref.Y10P)
        a.load(k), a.enqueue()
        if k in (at - 1, at):      # the two buffers differ where the stream's frame lies: the same bytes read by the other byte are another crop
            other = rref.Y10 if k == at else rref.Y10P
            assert not np.array_equal(rref.crop(a.frames[:a.layout_bytes].cpu().numpy(), a.recs[s], other, 1, 64, 64), a.crops[0][s])
        b.load(k), b.enqueue()
        same_rigs(a, b, (path, "tick", k))
    ea.close(), eb.close()


# ---- 5. the stateless ingest ----

def ingest_frames(w, h):
    """Every new format x bins 1, 2, 4 with the address of the footprint's first source byte at residues 0, 1, 7, 8, 15 mod
    16, at an odd pitch, the footprint a few groups inside a sensor just large enough."""
    combos = [(f, b) for f in rref.NEW for b in rref.BINS]
    res = (0, 1, 7, 8, 15)
    n = len(res) * len(combos)
    recs, fmts, bins, cursor = np.zeros(n, sref.SENSOR_DTYPE), np.zeros(n, np.uint8), np.zeros(n, np.uint8), 0
    for i in range(n):
        (fmt, b), r = combos[i // len(res)], res[i % len(res)]
        G, Bg, _ = rref.GROUPS[fmt]
        x0, y0 = 4 * ((5 * i) % 4), i % 5
        width, height = x0 + b * w + 4 * (i % 3), y0 + b * h + i % 2
        rb = rref.row_bytes(fmt, width)
        off = cursor + (r - x0 // G * Bg - cursor) % 16
        recs[i], fmts[i], bins[i] = sref.record(off, rb + 1 - rb % 2 + 2 * (i % 4), width, height, x0, y0), fmt, b
        assert (off + x0 // G * Bg) % 16 == r and int(recs[i]["pitch"]) % 2 == 1
        cursor = off + rref.extent(recs[i], fmt)
    return recs, fmts, bins, cursor


@pytest.mark.parametrize("w,h", [(64, 64), (60, 50)], ids=["vector-64x64", "per-pixel-60x50"])
def test_ingest_sensors_of_every_new_format_and_bin(aof, gpu_device, w, h):
    """aof_ingest_sensors_binned_device on a noise buffer of nbytes + SLACK bytes (the library is told nbytes), into dirty
    Guarded outputs: cropped, hist and ok against the numpy model.  One frame's x0 is off its group, one frame's format is
    no format: not read, nothing written."""
    import torch
    recs, fmts, bins, nbytes = ingest_frames(w, h)
    n = len(recs)
    bad = (47, 41, 66)
    recs[47]["x0"] += 1
    fmts[41] = 9
    fmts[66] = 3
    assert rref.GROUPS[int(fmts[47])][0] > 1
    assert [rref.valid(r, int(f), int(b), w, h, nbytes) for r, f, b in zip(recs, fmts, bins)] == [i not in bad for i in range(n)]
    buf = np.random.default_rng(n * 131 + w).integers(0, 256, nbytes + SLACK, dtype=np.uint8)
    buf[::7] = 255                                          # saturated bytes among the noise
    cam = up(gpu_device, buf)
    crops, hist, ok = Guarded(gpu_device, (n, h, w), skew=3 if w % 16 else 0), Guarded(gpu_device, (n, 40)), Guarded(gpu_device, (n,))
    lead = lambda a: up(gpu_device, np.concatenate([[0xEE], np.asarray(a, np.uint8)]).astype(np.uint8))[1:]
    aof.ingest_sensors(cam, table_tensor(gpu_device, recs), w, h, camera_bytes=nbytes, cropped=crops.tensor,
                       hist=hist.tensor.view(torch.int32), ok=ok.tensor, want_cropped=False, want_hist=False, formats=lead(fmts),
                       bins=lead(bins))
    torch.cuda.synchronize()
    assert ok.read().tolist() == [0 if i in bad else 1 for i in range(n)]
    got_c, got_h = crops.read(), hist.read().view("<u4")
    for i in range(n):
        if i in bad:
            continue
        want_c = rref.crop(buf, recs[i], int(fmts[i]), int(bins[i]), w, h)
        same(got_c[i], want_c, ("crop", i, rref.NAMES[int(fmts[i])], int(bins[i])))
        same(got_h[i], ingest_ref.ingest(want_c, w, h)[1], ("histogram", i))
    assert all(untouched(got_h[i]) and untouched(got_c[i]) for i in bad), "a refused frame: nothing is written"


# ---- 6. the facade ----

def test_the_facade_on_y10p_buffers_equals_an_object_fed_the_grey_planes(aof, orc, synth, gpu_device):
    """OpticalFlowBank, S = 10, 64 x 64: enableCameraPacked(96, 80, AOF_PIXEL_Y10P) fed MIPI-packed buffers against
    enableCamera(96, 80) fed the grey planes, the published entries entry by entry on raw bytes; stream 1 delivers Y12 from
    a 64 x 64 sensor inside its share of the bytes (setStreamSensor + setStreamPixelFormat).  The refusals leave the object
    as it was."""
    cfg = "px4-64"
    p, run, want, wire = rref.case(aof, orc, synth, cfg)
    cw, ch, w = 96, 80, 64
    rb = aof.bank_pixel_row_bytes(aof.PIXEL_Y10P, cw)
    assert rb == 120 == rref.row_bytes(rref.Y10P, cw)
    a, b = (aof.OpticalFlowBank(FX, FY, rref.RATE, w, w, S) for _ in range(2))
    for bank in (a, b):
        assert bank.engineOk(), bank.lastError()
        bank.setTimestampOffset(OFFSET)
    assert a.setStreamPixelFormat(0, aof.PIXEL_Y12) == EINVAL, "not before enabling"
    for bad in (3, 9, 255, 256, -1):
        assert a.enableCameraPacked(cw, ch, bad, 100, 4, rref.INTERVAL) == EINVAL and a.engineOk(), bad
    assert a.enableCameraPacked(cw + 2, ch, aof.PIXEL_Y10P, 100, 4, rref.INTERVAL) == EINVAL, "98 pixels are no whole groups of four"
    assert a.enableCameraPacked(cw + 1, ch, aof.PIXEL_Y12P, 100, 4, rref.INTERVAL) == EINVAL and a.engineOk()
    assert a.enableCameraPacked(cw, ch, aof.PIXEL_Y10P, 100, 4, rref.INTERVAL) == 0, a.lastError()
    assert b.enableCamera(cw, ch, 100, 4, rref.INTERVAL) == 0
    for bad in (3, 9, 255, 256, -1):
        assert a.setStreamPixelFormat(1, bad) == EINVAL and a.engineOk(), bad
    assert a.setStreamPixelFormat(S, aof.PIXEL_Y12) == EINVAL
    assert a.setStreamPixelFormat(1, aof.PIXEL_Y12) == EINVAL and a.engineOk(), "a Y12 row of 96 pixels does not fit the pitch of 120"
    share = ch * rb
    assert a.setStreamSensor(1, share, 2 * w, w, w, 0, 0) == 0, a.lastError()
    assert a.setStreamPixelFormat(1, aof.PIXEL_Y12) == 0, a.lastError()
    assert a.setStreamSensor(1, share, 2 * w, w + 20, w, 0, 0) == EINVAL, "checked with the stream's current format: 84 Y12 pixels need 168 bytes"
    x0, y0 = cw // 2 - w // 2, ch // 2 - w // 2
    assert x0 % 4 == 0
    rng = np.random.default_rng(17)
    entries_seen = 0
    for k in range(rref.TICKS):
        planes = rng.integers(0, 256, (S, ch, cw), dtype=np.uint8)
        planes[:, y0:y0 + w, x0:x0 + w] = run.frames[k]
        raw = np.stack([rref.pack(planes[s], rref.Y10P, rb, [k, s]) for s in range(S)])
        assert raw.shape == (S, share)
        raw[1] = rng.integers(0, 256, share, dtype=np.uint8)
        y12 = rref.pack(run.frames[k, 1], rref.Y12, 2 * w, [k, 99])
        raw[1, :len(y12)] = y12
        na, ea = a.pushCamera(raw, run.times[k], run.active[k], run.gyro[k])
        nb, eb = b.pushCamera(planes, run.times[k], run.active[k], run.gyro[k])
        assert na == nb >= 0, (k, a.lastError(), b.lastError())
        assert ea.tobytes() == eb.tobytes(), ("entries", k)
        assert a.exposureCommands().tobytes() == b.exposureCommands().tobytes(), ("exposure commands", k)
        entries_seen += na
    assert entries_seen > S
    a.close(), b.close()
