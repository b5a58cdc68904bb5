"""The stream bank with packed sensor pixels (AOF_PIXEL_*, aof_set_bank_pixel_formats, include/aof.h): YUYV-, UYVY- and
Y16-like buffers whose other byte per pixel is noise, against the grey sensor path fed the de-interleaved planes -- the
form tests/test_gpu_bank_sensors.py holds to the oracle -- and against the oracle itself, by bytes, never by tolerance.
The layouts, the packer and the rule in Python: tests/bank_pixels_ref.py (checked on the CPU: tests/test_bank_pixels_ref.py);
the rigs: tests/bank_rig.py and tests/bank_sensor_rig.py."""

import numpy as np
import pytest

import bank_camera_ref as cref
import bank_pixels_ref as pref
import bank_sensors_ref as sref
import ingest_ref
from bank_ref import FX, FY
from bank_rig import EINVAL, OFFSET, Guarded, counts_of, put, same, same_exposure, same_records, untouched, up
from bank_sensor_rig import SLACK, SensorRig, cameras, same_rigs, table_tensor
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

INTERVAL = sref.INTERVAL


def engines_and_cam(aof, synth, orc, cfg, path, n=2, K=None):
    p, run = sref.case(aof, orc, synth, cfg, K=K)[:2]
    cam = cameras(aof, cfg, p)[0]
    bp = aof.bank_params(run.S, FX, FY, 15, OFFSET, 1, 100, 0)
    engs = [aof.FlowEngine(p, 0) for _ in range(n)]
    for e in engs:
        e.set_bank_path(path)
    return p, run, cam, bp, engs


# ---- 1. twin banks: packed buffers against the grey sensor path on the de-interleaved planes ----

@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("cfg", ["px4-64", "opencv-128"])
def test_mixed_formats_leave_the_bytes_of_the_grey_sensor_path(aof, orc, synth, gpu_device, cfg, path):
    """48 ticks (first frames, due and not-due exposure ticks, idle streams: the census of bank_sensors_ref.case): every
    output buffer, the banks' frames and state and the gates equal after every tick."""
    p, run, cam, bp, (ea, eb) = engines_and_cam(aof, synth, orc, cfg, path)
    a, b = SensorRig(aof, ea, run, bp, gpu_device, cam, cfg, formats=True), SensorRig(aof, eb, run, bp, gpu_device, cam, cfg)
    a.bind(), b.bind()
    assert set(a.layout_formats[0].tolist()) == {0, 1, 2}
    for k in range(sref.T):
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, (cfg, path, "tick", k))
    ea.close(), eb.close()


# ---- 2. against the oracle directly ----

@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("cfg", ["px4-64", "opencv-128"])
def test_mixed_formats_equal_the_oracle_chain_per_stream(aof, orc, synth, gpu_device, cfg, path):
    p, run, want, wire, due, after, derot = sref.case(aof, orc, synth, cfg)
    S = run.S
    _, _, cam, bp, (eng,) = engines_and_cam(aof, synth, orc, cfg, path, n=1)
    a = SensorRig(aof, eng, run, bp, gpu_device, cam, cfg, formats=True)
    a.bind()
    uniform = cref.CameraRun(run, *sref.UNIFORM[cfg], 9)     # (the oracle crops at the centre: the same crops)
    for k in range(sref.T):
        got = a.push(k)
        same_records(got.recs, want[k], k, "oracle")
        assert got.wire == wire[k], ("oracle wire", k, [s for s in range(S) if got.wire[s] != wire[k][s]][:4])
        same_exposure(got.exposure, cref.expected_exposure(aof, orc, uniform.sensor(k), run, k, due[k]), k, "oracle exposure")
        assert got.derotated.tobytes() == derot[k].tobytes(), ("de-rotated", k)
        assert a.gate_bytes().tolist() == after[k].tolist(), ("gate", k)
    eng.close()


# ---- 3. all grey ----

@pytest.mark.parametrize("path", [1, 2])
def test_formats_that_are_all_grey_change_no_byte_against_sensors_bound_alone(aof, orc, synth, gpu_device, path):
    """Twin banks on the grey layouts, one with an array of AOF_PIXEL_GREY8 bound: twelve ticks, then two bursts of K = 3."""
    import torch
    cfg, K = "px4-64", 3
    p, run, cam, bp, (ea, eb) = engines_and_cam(aof, synth, orc, cfg, path, K=K)
    S = run.S
    a, b = (SensorRig(aof, e, run, bp, gpu_device, cam, cfg) for e in (ea, eb))
    ka, kb = (SensorRig(aof, r.eng, run, bp, gpu_device, cam, cfg, K=K, pad=5, bank=r.bank) for r in (a, b))
    grey = torch.zeros(S + 1, dtype=torch.uint8, device=gpu_device)[1:]
    ea.set_bank_pixel_formats(grey, S)
    given = counts_of(run, K, sref.T)
    for k in range(12):
        a.bind(), b.bind()
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, ("tick", k))
    for j in (4, 5):
        ka.bind(), kb.bind()
        ka.load(j, given), ka.enqueue()
        kb.load(j, given), kb.enqueue()
        same_rigs(ka, kb, ("burst", j))
    ea.close(), eb.close()


# ---- 4. bursts ----

@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("cfg,K", [("px4-64", 5), ("px4-64", 16), ("opencv-128", 5)])
def test_a_burst_equals_single_ticks_with_the_same_formats(aof, orc, synth, gpu_device, cfg, K, path):
    """K rounds with d_count and a padded round_stride against K single ticks on a twin bank: all outputs, all bank bytes."""
    T = sref.T - sref.T % K      # (every whole burst of the run: 9 of K = 5, 3 of K = 16)
    p, run, cam, bp, (ea, eb) = engines_and_cam(aof, synth, orc, cfg, path, K=K)
    S = run.S
    a = SensorRig(aof, ea, run, bp, gpu_device, cam, cfg, K=K, pad=37, formats=True)
    b = SensorRig(aof, eb, run, bp, gpu_device, cam, cfg, formats=True)
    a.bind(), b.bind()
    given = counts_of(run, K, sref.T)
    later = 0
    for k0 in range(0, T, K):
        got = a.push(k0 // K, given)
        for j in range(K):
            one = b.push(k0 + j)
            for name in ("recs", "exposure", "derotated"):
                assert getattr(got[j], name).tobytes() == getattr(one, name).tobytes(), (name, k0, j)
            assert got[j].wire == one.wire, ("wire", k0, j)
            later += int((got[j].recs["quality"] != aof.TICK_IDLE).sum()) if j else 0
        assert a.bank_bytes() == b.bank_bytes(), k0
    assert later > S, "frames in rounds behind the first"
    ea.close(), eb.close()


# ---- 5. formats and offsets rewritten before every tick ----

@pytest.mark.parametrize("path", [1, 2])
def test_formats_and_offsets_rewritten_every_tick_eager_and_through_a_replayed_graph(aof, orc, synth, gpu_device, path):
    """Every stream alternates between two places of the buffer AND two formats; records and formats are rewritten on the
    stream between the ticks.  Equal to the grey sensor path, eagerly and through a captured graph replayed 16 times."""
    import torch
    cfg, T = "px4-64", 16
    p, run, cam, bp, (ea, eb) = engines_and_cam(aof, synth, orc, cfg, path)
    S = run.S
    other = [(int(f) + 1) % 3 for f in pref.layout(*pref.TABLES[cfg], 64, 64)[1]]
    a = SensorRig(aof, ea, run, bp, gpu_device, cam, cfg, tables=[pref.TABLES[cfg], pref.retable(cfg, other)], formats=True)
    b = SensorRig(aof, eb, run, bp, gpu_device, cam, cfg)
    a.bind(), b.bind()
    assert all(a.layout_formats[0][s] != a.layout_formats[1][s] and int(a.layouts[0][s]["offset"]) != int(a.layouts[1][s]["offset"])
               for s in range(S))

    def rewrite(k):
        for s in range(S):
            put(a.table, s, a.layouts[k % 2][s])
            a.put_format(s, a.layout_formats[k % 2][s])

    outs = []
    for k in range(T):
        rewrite(k)
        a.load(k, which=k % 2), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, ("eager", k))
        outs.append(b.raw())
    final = b.bank_bytes()
    ea.bank_reset(a.bank)                        # (every kernel of the tick has run before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.enqueue()
    for k in range(T):
        rewrite(k)
        a.load(k, which=k % 2)
        g.replay()
        assert a.raw() == outs[k], ("replay", k)
    assert a.bank_bytes() == final
    ea.close(), eb.close()


# ---- 6. invalid records and formats are refused safely ----

def invalid_cases(rig, s):
    """(what, record, format) for stream s: a value that is no format, a packed pitch one byte short, a frame that ends one
    byte behind camera_bytes."""
    good, fmt = rig.recs[s], int(rig.layout_formats[0][s])
    edit = lambda **kw: sref.record(*[kw.get(n, int(good[n])) for n in ("offset", "pitch", "width", "height", "x0", "y0")])
    return [("format 3", good, 3), ("pitch = 2 * width - 1", edit(pitch=2 * int(good["width"]) - 1), fmt),
            ("one byte outside", edit(offset=rig.camera_bytes - pref.extent(good, fmt) + 1), fmt)]


@pytest.mark.parametrize("path", [1, 2])
def test_an_invalid_record_or_format_makes_the_stream_idle_with_its_own_quality(aof, orc, synth, gpu_device, path):
    """Per case: ticks 0..11 on twin banks, one packed stream invalid in one tick (A) against that stream inactive in that
    tick (C).  A's outputs are C's but for the quality of that record, the banks are equal after every tick (the stream's
    frame and state untouched, the other streams served as without it), and behind the repair the stream goes on."""
    cfg, T = "px4-64", 12
    p, run, cam, bp, (ea, ec) = engines_and_cam(aof, synth, orc, cfg, path)
    S = run.S
    a, c = (SensorRig(aof, e, run, bp, gpu_device, cam, cfg, formats=True) for e in (ea, ec))
    a.bind(), c.bind()
    packed = [s for s in range(S) if a.layout_formats[0][s] != pref.GREY8]
    for i in range(3):
        s = packed[i % len(packed)]
        what, bad, bad_fmt = invalid_cases(a, s)[i]
        fmt = int(a.layout_formats[0][s])
        assert not pref.valid(bad, bad_fmt, 64, 64, a.camera_bytes) and pref.valid(a.recs[s], fmt, 64, 64, a.camera_bytes), what
        kb = next(k for k in range(6, T) if run.active[k, s])
        assert run.active[:kb, s].any() and run.active[kb + 1:T, s].any(), "the stream has frames in front of and behind the tick"
        ea.bank_reset(a.bank), ec.bank_reset(c.bank)
        for k in range(T):
            if k == kb:
                put(a.table, s, bad), a.put_format(s, bad_fmt)
            a.load(k), c.load(k)
            if k == kb:
                c.select[s] = 0
                before = a.bank_bytes()
            a.enqueue(), c.enqueue()
            ga, gc = a.read(), c.read()
            if k == kb:
                assert ga.recs[s]["quality"] == aof.TICK_BAD_SENSOR and gc.recs[s]["quality"] == aof.TICK_IDLE, (what, ga.recs[s])
                ga.recs[s]["quality"] = aof.TICK_IDLE
                px = p.width * p.height
                assert a.bank_bytes()[s * px:(s + 1) * px] == before[s * px:(s + 1) * px], (what, "the stored frame")
                put(a.table, s, a.recs[s]), a.put_format(s, fmt)
            same_records(ga.recs, gc.recs, k, what)
            assert ga.wire == gc.wire and ga.exposure.tobytes() == gc.exposure.tobytes(), (what, k)
            assert ga.derotated.tobytes() == gc.derotated.tobytes(), (what, k)
            assert a.bank_bytes() == c.bank_bytes() and a.gate_bytes().tolist() == c.gate_bytes().tolist(), (what, k)
    ea.close(), ec.close()


@pytest.mark.parametrize("path", [1, 2])
def test_a_burst_whose_last_round_falls_outside_serves_the_rounds_before_it(aof, orc, synth, gpu_device, path):
    """K = 3, camera_bytes one byte short of round 2's last frame (a LUMA16_HI stream whose last grey byte is the buffer's
    last): rounds 0 and 1 are served, round 2 is AOF_TICK_BAD_SENSOR -- as a twin burst in which the stream has two frames."""
    cfg, K = "px4-64", 3
    p, run, cam, bp, (ea, ec) = engines_and_cam(aof, synth, orc, cfg, path, K=K)
    last = pref.TABLES[cfg][1][-1]
    a, c = (SensorRig(aof, e, run, bp, gpu_device, cam, cfg, K=K, pad=16, formats=True) for e in (ea, ec))
    a.bind(), c.bind()
    assert a.layout_formats[0][last] == pref.LUMA16_HI
    given = counts_of(run, K, sref.T)
    jb = next(j for j in range(1, len(given) - 1) if given[j, last] == K)
    for j in range(jb + 2):
        twin = given.copy()
        if j == jb:
            a.bind(a.camera_bytes - 1)
            twin[j, last] = K - 1
        ga, gc = a.push(j, given), c.push(j, twin)
        if j == jb:
            assert ga[K - 1].recs[last]["quality"] == aof.TICK_BAD_SENSOR and ga[K - 2].recs[last]["quality"] > aof.TICK_IDLE
            ga[K - 1].recs[last]["quality"] = aof.TICK_IDLE
            a.bind()
        for r in range(K):
            same_records(ga[r].recs, gc[r].recs, (j, r), "twin")
            assert ga[r].wire == gc[r].wire and ga[r].exposure.tobytes() == gc[r].exposure.tobytes(), (j, r)
            assert ga[r].derotated.tobytes() == gc[r].derotated.tobytes(), (j, r)
        assert a.bank_bytes() == c.bank_bytes(), j
    ea.close(), ec.close()


# ---- 7. the stateless ingest ----

def ingest_case(aof, gpu_device, recs, fmts, w, h, nbytes, bad=(), skew=0, no_formats=False):
    """aof_ingest_sensor_formats_device on a noise buffer of nbytes + SLACK bytes (the library is told nbytes), into dirty
    Guarded outputs, against crop() and ingest_ref's numpy histogram of every frame whose record is valid."""
    import torch
    n = len(recs)
    buf = np.random.default_rng(n * 131 + w).integers(0, 256, nbytes + SLACK, dtype=np.uint8)
    buf[::7] = 255                                          # values cv::calcHist drops
    cam = up(gpu_device, buf)
    crops, hist, ok = Guarded(gpu_device, (n, h, w), skew=skew), Guarded(gpu_device, (n, 40)), Guarded(gpu_device, (n,))
    d_fmts = None if no_formats else up(gpu_device, np.concatenate([[0xEE], np.asarray(fmts, np.uint8)]).astype(np.uint8))[1:]
    aof.ingest_sensors(cam, table_tensor(gpu_device, recs), w, h, camera_bytes=nbytes, cropped=crops.tensor,
                       hist=hist.tensor.view(torch.int32), ok=ok.tensor, want_cropped=False, want_hist=False, formats=d_fmts)
    torch.cuda.synchronize()
    flags = ok.read()
    assert [pref.valid(r, int(f), w, h, nbytes) for r, f in zip(recs, fmts)] == [i not in bad for i in range(n)]
    assert flags.tolist() == [0 if i in bad else 1 for i in range(n)], flags
    got_c, got_h = crops.read(), hist.read().view("<u4")
    for i in range(n):
        if i in bad:
            continue
        want_c = pref.crop(buf, recs[i], int(fmts[i]), w, h)
        same(got_c[i], want_c, ("crop", i))
        same(got_h[i], ingest_ref.ingest(want_c, w, h)[1], ("histogram", i))
    if h <= 128 and bad:
        assert all(untouched(got_h[i]) and untouched(got_c[i]) for i in bad), "a refused frame: nothing is written"


def test_ingest_with_formats_at_every_alignment_and_an_odd_pitch(aof, gpu_device):
    """48 frames of a 100 x 70 sensor: each format with the address of the crop's first source byte at every residue mod
    16, at an odd pitch; one record per format ends one byte behind the buffer, one frame has a value that is no format."""
    recs, fmts, cursor = np.zeros(48, sref.SENSOR_DTYPE), np.zeros(48, np.uint8), 0
    for i in range(48):
        fmt, res = i // 16, i % 16
        bpp = pref.bpp_of(fmt)
        x0, y0 = (5 * i) % 37, i % 7
        off = cursor + (res - x0 * bpp - cursor) % 16
        recs[i], fmts[i] = sref.record(off, 100 * bpp + 31, 100, 70, x0, y0), fmt
        assert (off + x0 * bpp) % 16 == res
        cursor = off + pref.extent(recs[i], fmt)
    for i in (5, 21, 37):
        recs[i]["offset"] = cursor - pref.extent(recs[i], int(fmts[i])) + 1
    fmts[40] = 3
    ingest_case(aof, gpu_device, recs, fmts, 64, 64, cursor, bad=(5, 21, 37, 40))
    ingest_case(aof, gpu_device, recs[:16], fmts[:16], 64, 64, cursor, bad=(5,), skew=3, no_formats=True)   # NULL: all grey


def test_ingest_with_formats_on_the_scalar_path_and_on_two_strips(aof, gpu_device):
    """A crop width that is no multiple of 16 (24 x 20); and a 160-row crop: two workgroups per frame."""
    recs = np.array([sref.record(3, 83, 70, 60, 11, 9), sref.record(6000, 141, 70, 50, 20, 10), sref.record(14003, 123, 61, 47, 0, 0),
                     sref.record(21000, 140, 70, 30, 46, 10), sref.record(26000, 139, 70, 30, 0, 0)])
    fmts = [0, 1, 2, 2, 1]
    ingest_case(aof, gpu_device, recs, fmts, 24, 20, 26000 + 29 * 139 + 140, bad=(4,))
    recs = np.array([sref.record(1, 166, 80, 200, 9, 5), sref.record(40000, 128, 64, 160, 0, 0), sref.record(70007, 263, 100, 161, 36, 1),
                     sref.record(70007, 263, 100, 161, 37, 1)])
    fmts = [1, 2, 1, 1]
    ingest_case(aof, gpu_device, recs, fmts, 64, 160, 70007 + 160 * 263 + 200, bad=(3,))


# ---- 8. the facade ----

def test_the_facade_with_packed_cameras_equals_an_object_fed_the_grey_planes(aof, orc, synth, gpu_device):
    """OpticalFlowBank, S = 5, 64 x 64: enableCameraPacked(96, 80, LUMA16_HI) fed packed frames against enableCamera(96, 80)
    fed their grey planes, entry by entry; and one stream of a GREY object made LUMA16_LO by setStreamSensor +
    setStreamPixelFormat against an object fed the frames themselves.  The refusals leave the objects as they were."""
    cfg, T = "px4-64", 24
    p, run = sref.case(aof, orc, synth, cfg)[:2]
    S, (cw, ch) = run.S, (96, 80)
    uniform = cref.CameraRun(run, cw, ch, 9)
    a, b, c = (aof.OpticalFlowBank(FX, FY, 15, 64, 64, S) for _ in range(3))
    for bank in (a, b, c):
        assert bank.engineOk(), bank.lastError()
        bank.setTimestampOffset(OFFSET)
    assert a.setStreamPixelFormat(0, aof.PIXEL_LUMA16_LO) == EINVAL, "not before enabling"
    assert a.enableCameraPacked(cw, ch, 3, 100, 4, INTERVAL) == EINVAL and a.engineOk(), "no such format"
    assert a.enableCameraPacked(cw, ch, aof.PIXEL_LUMA16_HI, 100, 4, INTERVAL) == 0, a.lastError()
    assert a.enableCameraPacked(cw, ch, aof.PIXEL_LUMA16_HI, 100, 4, INTERVAL) == EINVAL and a.enableCamera(cw, ch, 100, 4) == EINVAL
    assert b.enableCamera(cw, ch, 100, 4, INTERVAL) == 0 and c.enableCamera(128, 96, 100, 4, INTERVAL) == 0
    assert c.setStreamPixelFormat(1, aof.PIXEL_LUMA16_LO) == EINVAL and c.engineOk(), "stream 1's 128-pixel rows would need 256 bytes"
    assert c.setStreamPixelFormat(S, 1) == EINVAL and c.setStreamPixelFormat(-1, 1) == EINVAL and c.setStreamPixelFormat(1, 3) == EINVAL
    # a: a record is checked with the stream's CURRENT format: 96 pixels at pitch 96 do not fit LUMA16_HI rows
    assert a.setStreamSensor(0, 0, 96, 96, 80, 16, 8) == EINVAL and a.setStreamSensor(0, 0, 192, 96, 80, 16, 8) == 0
    rng = np.random.default_rng(11)
    entries_seen = 0
    for k in range(T):
        grey = uniform.sensor(k)                                   # [S, ch, cw]
        packed = rng.integers(0, 256, (S, ch, cw, 2), dtype=np.uint8)
        packed[..., 1] = grey
        na, ea = a.pushCamera(packed, run.times[k], run.active[k], run.gyro[k])
        nb, eb = b.pushCamera(grey, run.times[k], run.active[k], run.gyro[k])
        assert na == nb >= 0, (k, a.lastError(), b.lastError())
        assert ea.tobytes() == eb.tobytes(), ("entries", k)
        assert a.exposureCommands().tobytes() == b.exposureCommands().tobytes(), ("exposure commands", k)
        entries_seen += na
    assert entries_seen > 2 * S
    # c, a grey object of 128 x 96 bytes per stream: 64 x 64 frames (the crop is the sensor) at the start of each stream's
    # bytes -- stream 1 as LUMA16_LO pixels at pitch 128, the others grey at pitch 64
    w = 64
    offs = [s * 128 * 96 for s in range(S)]
    for s in range(S):
        assert c.setStreamSensor(s, offs[s], 128 if s == 1 else 64, w, w, 0, 0) == 0, c.lastError()
    assert c.setStreamPixelFormat(1, aof.PIXEL_LUMA16_LO) == 0, c.lastError()
    assert c.setStreamSensor(1, offs[1], 127, w, w, 0, 0) == EINVAL, "checked with the stream's current format"
    d = aof.OpticalFlowBank(FX, FY, 15, 64, 64, S)
    d.setTimestampOffset(OFFSET)
    assert d.enableCamera(64, 64, 100, 4, INTERVAL) == 0
    for k in range(12):
        buf = rng.integers(0, 256, S * 128 * 96, dtype=np.uint8)
        for s in range(S):
            if s == 1:
                buf[offs[s]:offs[s] + 2 * w * w:2] = run.frames[k, s].reshape(-1)
            else:
                buf[offs[s]:offs[s] + w * w] = run.frames[k, s].reshape(-1)
        nc, ec = c.pushCamera(buf, run.times[k], run.active[k], run.gyro[k])
        nd, ed = d.pushCamera(run.frames[k], run.times[k], run.active[k], run.gyro[k])
        assert nc == nd >= 0 and ec.tobytes() == ed.tobytes(), ("one packed stream", k, c.lastError())
    for bank in (a, b, c, d):
        bank.close()


# ---- bindings and refusals ----

def test_bindings_and_refusals(aof, orc, synth, gpu_device):
    """Every -EINVAL of aof_set_bank_pixel_formats with the binding left as it was; formats bound without sensors and a
    camera push of another stream count are refused and write nothing; the pushes of pre-cropped frames do not look at the
    binding; unbinding the formats leaves sensors bound alone."""
    import torch
    cfg = "px4-64"
    p, run, cam, bp, (ea, eb) = engines_and_cam(aof, synth, orc, cfg, 0)
    S = run.S
    a, b = SensorRig(aof, ea, run, bp, gpu_device, cam, cfg, formats=True), SensorRig(aof, eb, run, bp, gpu_device, cam, cfg)
    a.bind(), b.bind()
    setter = aof.lib.aof_set_bank_pixel_formats
    base = a.formats.data_ptr()
    assert setter(None, base, S) == EINVAL
    assert setter(ea._ctx, base, 0) == EINVAL and setter(ea._ctx, base, -1) == EINVAL and b"n_streams" in aof.lib.aof_last_error(ea._ctx)
    for k in range(3):                            # the binding is as it was: the packed layouts are served
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, ("after the refusals", k))

    def refused(text):
        snapshot = a.bank.buffer.clone()
        a.load(3)
        with pytest.raises(aof.AofError):
            a.enqueue()
        assert text in aof.lib.aof_last_error(ea._ctx), aof.lib.aof_last_error(ea._ctx)
        torch.cuda.synchronize()
        assert torch.equal(a.bank.buffer, snapshot) and all(untouched(g.read()) for g in (a.outputs[0], a.outputs[3], a.outputs[4]))

    assert setter(ea._ctx, base, S - 1) == 0      # an array for S - 1 streams
    refused(b"aof_set_bank_pixel_formats")
    assert setter(ea._ctx, base, S) == 0
    ea.set_bank_sensors(None)                     # formats without sensors
    refused(b"without sensor records")
    fresh = ea.bank_create(bp, gpu_device)
    plain = ea.bank_push(fresh, up(gpu_device, run.frames[3]), up(gpu_device, run.times[3]), up(gpu_device, run.active[3]))
    torch.cuda.synchronize()
    q = aof.ticks_view(plain)["quality"]
    assert (q == np.where(run.active[3] != 0, 0, aof.TICK_IDLE)).all(), "the plain push on pre-cropped frames, whatever is bound"
    # formats unbound, sensors bound alone: the grey layouts on the same engine and bank
    ea.set_bank_pixel_formats(None)
    g = SensorRig(aof, ea, run, bp, gpu_device, cam, cfg, bank=a.bank)
    g.bind()
    for k in (3, 4, 5):
        g.load(k), g.enqueue()
        b.load(k), b.enqueue()
        same_rigs(g, b, ("sensors alone", k))
    ea.close(), eb.close()
