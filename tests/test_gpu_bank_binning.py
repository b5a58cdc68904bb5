"""The stream bank with binned sensor pixels (aof_set_bank_binning, include/aof.h): nine streams, one per layout x bin, whose
sensor buffers hold noisy footprints, against a twin bank on grey sensors that hold the crops binned on the host by the
numpy model, and against the oracle chain -- by bytes, never by tolerance.  Bursts, invalid footprints and bins, bins
rewritten between ticks (eagerly and through a replayed graph), the stateless ingest and the facade.  The model, the tables
and the packer: tests/bank_binning_ref.py (checked on the CPU: tests/test_bank_binning_ref.py); the rigs:
tests/bank_sensor_rig.py."""

import numpy as np
import pytest

import bank_binning_ref as bref
import bank_camera_ref as cref
import bank_pixels_ref as pref
import bank_sensors_ref as sref
import ingest_ref
from bank_ref import FX, FY
from bank_rig import EINVAL, OFFSET, Guarded, counts_of, put, same, same_exposure, same_records, untouched, up
from bank_sensor_rig import SLACK, BinnedRig, GreyTwin, same_rigs, table_tensor
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

S = bref.S


def setup(aof, synth, orc, cfg, path, n=2, K=None):
    p, run = bref.case(aof, orc, synth, cfg, K=K)[:2]
    cam = aof.bank_camera_params(*sref.SCALARS[cfg], p.width, p.height, 0, bref.INTERVAL, cref.DEROTATE, FX, FY)   # (scalars no stream has)
    bp = aof.bank_params(run.S, FX, FY, bref.RATE, OFFSET, 1, 100, 0)
    engs = [aof.FlowEngine(p, 0) for _ in range(n)]
    for e in engs:
        e.set_bank_path(path)
    return p, run, cam, bp, engs


# ---- 1. the mixed bank: against the grey twin on the host-binned crops, and against the oracle ----

@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("cfg", ["px4-64", "opencv-128"])
def test_a_mixed_bank_leaves_the_bytes_of_a_grey_bank_on_the_host_binned_crops_and_of_the_oracle(aof, orc, synth, gpu_device, cfg, path):
    p, run, want, wire, due, after, derot = bref.case(aof, orc, synth, cfg)
    _, _, cam, bp, (ea, eb) = setup(aof, synth, orc, cfg, path)
    a = BinnedRig(aof, ea, run, bp, gpu_device, cam, p.width, p.height)
    b = GreyTwin(aof, eb, run, bp, gpu_device, cam, a)
    a.bind(), b.bind()
    assert sorted(zip(a.layout_formats[0].tolist(), a.host_bins.tolist())) == sorted(bref.COMBOS)
    uniform = cref.CameraRun(run, p.width + 32, p.height + 16, 9)     # (the oracle crops at the centre: the same crops)
    for k in range(bref.T):
        a.load(k), a.enqueue()
        assert (a.crops[0] == run.frames[k]).all(), "the model bins the buffer to the run's frames"
        b.load(k), b.enqueue()
        same_rigs(a, b, (cfg, path, "tick", k))
        got = a.read()
        same_records(got.recs, want[k], k, "oracle")
        assert got.wire == wire[k], ("oracle wire", k, [s for s in range(S) if got.wire[s] != wire[k][s]][:4])
        same_exposure(got.exposure, cref.expected_exposure(aof, orc, uniform.sensor(k), run, k, due[k]), k, "oracle exposure")
        assert got.derotated.tobytes() == derot[k].tobytes(), ("de-rotated", k)
        assert a.gate_bytes().tolist() == after[k].tolist(), ("gate", k)
    ea.close(), eb.close()


@pytest.mark.parametrize("path", [1, 2])
def test_bins_that_are_all_ones_change_no_byte_against_no_array(aof, orc, synth, gpu_device, path):
    """Twin banks on the same buffers (the table's sensors, every stream at bin 1), one with an array of ones bound, one with
    sensors and formats bound alone: twelve ticks, then the bursts of K = 3 on the same banks."""
    cfg, K = "px4-64", 3
    p, run, cam, bp, (ea, eb) = setup(aof, synth, orc, cfg, path, K=K)
    ones = np.ones(S, np.uint8)
    a, b = (BinnedRig(aof, e, run, bp, gpu_device, cam, 64, 64, bins=ones, bind_bins=e is ea) for e in (ea, eb))
    ka, kb = (BinnedRig(aof, r.eng, run, bp, gpu_device, cam, 64, 64, K=K, pad=5, bank=r.bank, bins=ones, bind_bins=r is a) for r in (a, b))
    given = counts_of(run, K, bref.T)
    for k in range(bref.T):
        a.bind(), b.bind()
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, ("tick", k))
    for j in (1, 2):
        ka.bind(), kb.bind()
        ka.load(j, given), ka.enqueue()
        kb.load(j, given), kb.enqueue()
        same_rigs(ka, kb, ("burst", j))
    ea.close(), eb.close()


# ---- 2. bursts ----

@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("cfg", ["px4-64", "opencv-128"])
def test_a_burst_equals_single_ticks_with_the_same_bins(aof, orc, synth, gpu_device, cfg, path):
    """K = 3 rounds with a mixed d_count and a padded round_stride against K single ticks on a twin bank."""
    K = 3
    p, run, cam, bp, (ea, eb) = setup(aof, synth, orc, cfg, path, K=K)
    a = BinnedRig(aof, ea, run, bp, gpu_device, cam, p.width, p.height, K=K, pad=37)
    b = BinnedRig(aof, eb, run, bp, gpu_device, cam, p.width, p.height)
    a.bind(), b.bind()
    given = counts_of(run, K, bref.T)
    assert len(set(given.reshape(-1).tolist())) > 2, "mixed counts"
    later = 0
    for k0 in range(0, bref.T, K):
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


# ---- 3. invalid footprints and bins ----

def invalid_cases(rig):
    """(what, stream, record or None, bin or None): a footprint one sensor pixel too wide or too high for a binned stream,
    and four bytes that are no bin."""
    w, h = rig.w, rig.h
    edit = lambda s, **kw: sref.record(*[kw.get(n, int(rig.recs[s][n])) for n in ("offset", "pitch", "width", "height", "x0", "y0")])
    wide, high = 4, 8     # (LUMA16_LO at bin 2, LUMA16_HI at bin 4: the buffer's last frame)
    out = [("one pixel too wide", wide, edit(wide, width=int(rig.recs[wide]["x0"]) + int(rig.host_bins[wide]) * w - 1), None),
           ("one pixel too high", high, edit(high, height=int(rig.recs[high]["y0"]) + int(rig.host_bins[high]) * h - 1), None)]
    return out + [("bin %d" % b, (1, 3, 5, 7)[i], None, b) for i, b in enumerate(bref.BAD_BINS)]


@pytest.mark.parametrize("path", [1, 2])
def test_an_invalid_footprint_or_bin_makes_the_stream_idle_with_its_own_quality(aof, orc, synth, gpu_device, path):
    """Per case: ticks 0..9 on twin banks, one stream invalid in one tick (A) against that stream inactive in that tick (C).
    A's outputs are C's but for the quality of that record, the banks are equal after every tick, and behind the repair the
    stream goes on.  The stream whose frame ends on the last byte of camera_bytes is served in every tick it has a frame."""
    cfg, T = "px4-64", 10
    p, run, cam, bp, (ea, ec) = setup(aof, synth, orc, cfg, path)
    a, c = (BinnedRig(aof, e, run, bp, gpu_device, cam, 64, 64) for e in (ea, ec))
    a.bind(), c.bind()
    last = bref.ORDER[-1]
    assert int(a.recs[last]["offset"]) + sref.extent(a.recs[last], int(a.layout_formats[0][last])) == a.camera_bytes
    for what, s, bad, bad_bin in invalid_cases(a):
        fmt, b = int(a.layout_formats[0][s]), int(a.host_bins[s])
        assert bref.valid(a.recs[s], fmt, b, 64, 64, a.camera_bytes), what
        assert not bref.valid(a.recs[s] if bad is None else bad, fmt, b if bad_bin is None else bad_bin, 64, 64, a.camera_bytes), what
        kb = next(k for k in range(5, T) if run.active[k, s])
        assert run.active[:kb, s].any() and run.active[kb + 1:T, s].any(), "the stream has frames in front of and behind the tick"
        ea.bank_reset(a.bank), ec.bank_reset(c.bank)
        for k in range(T):
            if k == kb:
                if bad is not None:
                    put(a.table, s, bad)
                if bad_bin is not None:
                    a.put_bin(s, bad_bin, host=False)
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
                put(a.table, s, a.recs[s]), a.put_bin(s, b)
            if run.active[k, last] and not (k == kb and s == last):
                assert ga.recs[last]["quality"] != aof.TICK_BAD_SENSOR, "the frame that ends on the buffer's last byte"
            same_records(ga.recs, gc.recs, k, what)
            assert ga.wire == gc.wire and ga.exposure.tobytes() == gc.exposure.tobytes(), (what, k)
            assert ga.derotated.tobytes() == gc.derotated.tobytes(), (what, k)
            assert a.bank_bytes() == c.bank_bytes() and a.gate_bytes().tolist() == c.gate_bytes().tolist(), (what, k)
    ea.close(), ec.close()


# ---- 4. a bin rewritten between ticks ----

@pytest.mark.parametrize("path", [1, 2])
def test_a_bin_rewritten_between_ticks_eager_and_through_a_replayed_graph(aof, orc, synth, gpu_device, path):
    """Stream 5 (LUMA16_LO, a sensor laid out for bin 4) runs at bin 1 in ticks 0..3, bin 2 in ticks 4..7, bin 4 from tick 8
    on; the byte is rewritten on the stream between the ticks, with a masked reset of that stream.  Equal to the grey twin on
    the host-binned crops, eagerly and through a captured graph replayed twelve times."""
    import torch
    cfg, s = "px4-64", 5
    p, run, cam, bp, (ea, eb) = setup(aof, synth, orc, cfg, path)
    assert bref.COMBOS[s] == (pref.LUMA16_LO, 4)
    a = BinnedRig(aof, ea, run, bp, gpu_device, cam, 64, 64)
    b = GreyTwin(aof, eb, run, bp, gpu_device, cam, a)
    a.bind(), b.bind()
    mask = torch.zeros(S, dtype=torch.uint8, device=gpu_device)
    mask[s] = 1
    assert sum(int(run.active[k0:k0 + 4, s].sum()) >= 2 for k0 in (0, 4, 8)) == 3, "a pair at every bin"

    def rewrite(k):
        if k % 4 == 0:
            a.put_bin(s, (1, 2, 4)[k // 4])
            ea.bank_reset(a.bank, mask)

    outs = []
    for k in range(bref.T):
        rewrite(k)
        if k % 4 == 0:
            eb.bank_reset(b.bank, mask)
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, ("eager", k))
        outs.append(b.raw())
    final = b.bank_bytes()
    ea.bank_reset(a.bank)                        # (every kernel of the tick has run before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.enqueue()
    for k in range(bref.T):
        rewrite(k)
        a.load(k)
        g.replay()
        assert a.raw() == outs[k], ("replay", k)
    assert a.bank_bytes() == final
    ea.close(), eb.close()


# ---- 5. the stateless ingest ----

def ingest_case(aof, gpu_device, recs, fmts, bins, w, h, nbytes, bad=(), skew=0, no_bins=False):
    """aof_ingest_sensors_binned_device on a noise buffer of nbytes + SLACK bytes (the library is told nbytes), into dirty
    Guarded outputs, against the numpy model's crop and ingest_ref's histogram of every frame whose record is valid."""
    import torch
    n = len(recs)
    buf = np.random.default_rng(n * 131 + w).integers(0, 256, nbytes + SLACK, dtype=np.uint8)
    buf[::7] = 255                                          # saturated pixels among the noise
    cam = up(gpu_device, buf)
    crops, hist, ok = Guarded(gpu_device, (n, h, w), skew=skew), Guarded(gpu_device, (n, 40)), Guarded(gpu_device, (n,))
    lead = lambda a: up(gpu_device, np.concatenate([[0xEE], np.asarray(a, np.uint8)]).astype(np.uint8))[1:]
    aof.ingest_sensors(cam, table_tensor(gpu_device, recs), w, h, camera_bytes=nbytes, cropped=crops.tensor,
                       hist=hist.tensor.view(torch.int32), ok=ok.tensor, want_cropped=False, want_hist=False, formats=lead(fmts),
                       bins=None if no_bins else lead(bins))
    torch.cuda.synchronize()
    flags = ok.read()
    assert [bref.valid(r, int(f), int(b), w, h, nbytes) for r, f, b in zip(recs, fmts, bins)] == [i not in bad for i in range(n)]
    assert flags.tolist() == [0 if i in bad else 1 for i in range(n)], flags
    got_c, got_h = crops.read(), hist.read().view("<u4")
    for i in range(n):
        if i in bad:
            continue
        want_c = bref.crop(buf, recs[i], int(fmts[i]), int(bins[i]), w, h)
        same(got_c[i], want_c, ("crop", i, int(fmts[i]), int(bins[i])))
        same(got_h[i], ingest_ref.ingest(want_c, w, h)[1], ("histogram", i))
    if bad:
        assert all(untouched(got_h[i]) and untouched(got_c[i]) for i in bad), "a refused frame: nothing is written"


def ingest_frames(w, h):
    """144 frames: every layout x bin with the address of the footprint's first source byte at every residue mod 16, at an
    odd pitch, the footprint a few pixels inside a sensor just large enough."""
    n = 16 * len(bref.COMBOS)
    recs, fmts, bins, cursor = np.zeros(n, sref.SENSOR_DTYPE), np.zeros(n, np.uint8), np.zeros(n, np.uint8), 0
    for i in range(n):
        (fmt, b), res = bref.COMBOS[i // 16], i % 16
        bpp = pref.bpp_of(fmt)
        x0, y0 = (5 * i) % 13, i % 5
        width, height = x0 + b * w + i % 3, y0 + b * h + i % 2
        off = cursor + (res - x0 * bpp - cursor) % 16
        recs[i], fmts[i], bins[i] = sref.record(off, width * bpp + 1 - (width * bpp) % 2 + 2 * (i % 4), width, height, x0, y0), fmt, b
        assert (off + x0 * bpp) % 16 == res
        cursor = off + pref.extent(recs[i], fmt)
    return recs, fmts, bins, cursor


@pytest.mark.parametrize("w,h", [(64, 32), (40, 20)], ids=["vector-64", "scalar-40"])
def test_ingest_with_bins_at_every_alignment(aof, gpu_device, w, h):
    """Crop widths 64 (16-byte pieces) and 40 (the scalar path): one frame's bin is no bin, one binned frame is one sensor
    pixel too narrow; NULL bins against ones on the frames of bin 1."""
    recs, fmts, bins, nbytes = ingest_frames(w, h)
    bins[70] = 3
    recs[120]["width"] = int(recs[120]["x0"]) + int(bins[120]) * w - 1
    assert bins[120] > 1
    ingest_case(aof, gpu_device, recs, fmts, bins, w, h, nbytes, bad=(70, 120))
    one = [i for i in range(len(recs)) if bins[i] == 1]
    ingest_case(aof, gpu_device, recs[one], fmts[one], bins[one], w, h, nbytes, skew=3 if w % 16 else 0, no_bins=True)   # NULL: ones


# ---- 6. the facade ----

def test_the_facade_with_binned_streams_equals_an_object_fed_the_binned_crops(aof, orc, synth, gpu_device):
    """OpticalFlowBank, S = 9, 64 x 64: enableCamera(272, 264) with streams at bins 1, 2, 4 (setStreamSensor +
    setStreamBinning) fed noisy footprints against enableCamera(64, 64) fed the host-binned crops, entry by entry.  The
    refusals leave the object as it was."""
    cfg = "px4-64"
    p, run = bref.case(aof, orc, synth, cfg)[:2]
    cw, ch, w = 272, 264, 64
    a, b = (aof.OpticalFlowBank(FX, FY, bref.RATE, w, w, S) for _ in range(2))
    for bank in (a, b):
        assert bank.engineOk(), bank.lastError()
        bank.setTimestampOffset(OFFSET)
    assert a.setStreamBinning(0, 2) == EINVAL, "not before enabling"
    assert a.enableCamera(cw, ch, 100, 4, bref.INTERVAL) == 0 and b.enableCamera(w, w, 100, 4, bref.INTERVAL) == 0
    bins = [(1, 2, 4)[s % 3] for s in range(S)]
    origin = {1: (cw // 2 - w // 2, ch // 2 - w // 2), 2: (cw // 2 - w // 2, ch // 2 - w // 2), 4: (3, 5)}
    assert a.setStreamBinning(S, 2) == EINVAL and a.setStreamBinning(-1, 2) == EINVAL
    for bad in (0, 3, 8, 255, -1):
        assert a.setStreamBinning(1, bad) == EINVAL and a.engineOk()
    assert a.setStreamBinning(2, 4) == EINVAL and a.engineOk(), "the centred record leaves no room for 256 x 256"
    for s in range(S):
        if bins[s] == 4:
            assert a.setStreamSensor(s, s * cw * ch, cw, cw, ch, *origin[4]) == 0, a.lastError()
        if bins[s] != 1:
            assert a.setStreamBinning(s, bins[s]) == 0, a.lastError()
    assert a.setStreamSensor(2, 2 * cw * ch, cw, cw, ch, 17, 5) == EINVAL, "checked with the stream's current bin: 17 + 256 > 272"
    assert a.setStreamPixelFormat(2, aof.PIXEL_LUMA16_LO) == EINVAL and a.engineOk()
    assert a.setStreamBinning(2, 2) == 0 and a.setStreamBinning(2, 4) == 0, "a bin may change, and change back"
    rng = np.random.default_rng(13)
    entries_seen = 0
    for k in range(bref.T):
        sensor = rng.integers(0, 256, (S, ch, cw), dtype=np.uint8)
        for s in range(S):
            x0, y0 = origin[bins[s]]
            foot = bref.spread(run.frames[k, s], bins[s], rng)
            sensor[s, y0:y0 + foot.shape[0], x0:x0 + foot.shape[1]] = foot
            assert (bref.bin_plane(sensor[s, y0:y0 + foot.shape[0], x0:x0 + foot.shape[1]], bins[s]) == run.frames[k, s]).all()
        na, ea = a.pushCamera(sensor, run.times[k], run.active[k], run.gyro[k])
        nb, eb = b.pushCamera(run.frames[k], run.times[k], run.active[k], run.gyro[k])
        assert na == nb >= 0, (k, a.lastError(), b.lastError())
        assert ea.tobytes() == eb.tobytes(), ("entries", k)
        assert a.exposureCommands().tobytes() == b.exposureCommands().tobytes(), ("exposure commands", k)
        entries_seen += na
    assert entries_seen > S
    a.close(), b.close()


# ---- bindings and refusals ----

def test_bindings_and_refusals(aof, orc, synth, gpu_device):
    """The -EINVAL of aof_set_bank_binning with the binding left as it was; a binning bound without sensors and a camera push
    of another stream count are refused and write nothing; the pushes of pre-cropped frames do not look at the binding."""
    import torch
    cfg = "px4-64"
    p, run, cam, bp, (ea, eb) = setup(aof, synth, orc, cfg, 0)
    a = BinnedRig(aof, ea, run, bp, gpu_device, cam, 64, 64)
    b = GreyTwin(aof, eb, run, bp, gpu_device, cam, a)
    a.bind(), b.bind()
    setter = aof.lib.aof_set_bank_binning
    base = a.bins.data_ptr()
    assert setter(None, base, S) == EINVAL
    assert setter(ea._ctx, base, 0) == EINVAL and setter(ea._ctx, base, -1) == EINVAL and b"n_streams" in aof.lib.aof_last_error(ea._ctx)
    for k in range(3):                            # the binding is as it was: the binned streams are served
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
    refused(b"aof_set_bank_binning")
    assert setter(ea._ctx, base, S) == 0
    ea.set_bank_pixel_formats(None)
    ea.set_bank_sensors(None)                     # a binning without sensors
    refused(b"without sensor records")
    fresh = ea.bank_create(bp, gpu_device)
    plain = ea.bank_push(fresh, up(gpu_device, run.frames[3]), up(gpu_device, run.times[3]), up(gpu_device, run.active[3]))
    torch.cuda.synchronize()
    q = aof.ticks_view(plain)["quality"]
    assert (q == np.where(run.active[3] != 0, 0, aof.TICK_IDLE)).all(), "the plain push on pre-cropped frames, whatever is bound"
    a.bind()                                      # bound again: the run goes on
    for k in (3, 4, 5):
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, ("bound again", k))
    ea.set_bank_binning(None)
    ea.close(), eb.close()
