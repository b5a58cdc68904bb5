"""The stream bank with per-stream sensors (aof_bank_sensor / aof_set_bank_sensors, include/aof.h): S cameras of different
sizes, row pitches, alignments and crop origins in one camera buffer, against the form that is already held to the
oracle (uniform sensor frames, nothing bound) and against the oracle itself -- by bytes, never by tolerance.  The scalars
of aof_bank_camera hold a sensor size no stream has: a kernel that still reads them cannot pass.  The layouts, the packer
and the validity rule in Python: tests/bank_sensors_ref.py (its census: tests/test_bank_sensors_ref.py); the rig:
tests/bank_rig.py and tests/bank_sensor_rig.py."""

import numpy as np
import pytest

import bank_camera_ref as cref
import bank_sensors_ref as sref
import ingest_ref
from bank_ref import FX, FY
from bank_rig import EINVAL, OFFSET, BankRig, Guarded, counts_of, put, same, same_exposure, same_records, untouched, up
from bank_sensor_rig import SLACK, SensorRig, cameras, same_rigs, table_tensor
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

INTERVAL = sref.INTERVAL


def pair_of_rigs(aof, synth, orc, gpu_device, cfg, path, **kw):
    """(engines, rig A: records bound, mixed layouts; rig B: nothing bound, uniform sensors) on one run."""
    p, run = sref.case(aof, orc, synth, cfg)[:2]
    S = run.S
    cam_a, cam_b = cameras(aof, cfg, p)
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    ea, eb = aof.FlowEngine(p, 0), aof.FlowEngine(p, 0)
    ea.set_bank_path(path), eb.set_bank_path(path)
    a = SensorRig(aof, ea, run, bp, gpu_device, cam_a, cfg, **kw)
    a.bind()
    b = BankRig(aof, eb, run, bp, gpu_device, camera=(cam_b, cref.CameraRun(run, *sref.UNIFORM[cfg], 9)))
    return (ea, eb), a, b


# ---- 1. a bank of one, against the form that is held to the oracle ----

@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("cfg", ["px4-64", "opencv-128"])
def test_mixed_sensors_leave_the_bytes_of_uniform_sensors_with_the_same_crops(aof, orc, synth, gpu_device, cfg, path):
    """48 ticks: every output buffer, the banks' frames and state and the gates equal after every tick."""
    engines, a, b = pair_of_rigs(aof, synth, orc, gpu_device, cfg, path)
    for k in range(sref.T):
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, (cfg, path, "tick", k))
    for e in engines:
        e.close()


# ---- 2. against the oracle directly ----

@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("cfg", ["px4-64", "opencv-128"])
def test_mixed_sensors_equal_the_oracle_chain_per_stream(aof, orc, synth, gpu_device, cfg, path):
    p, run, want, wire, due, after, derot = sref.case(aof, orc, synth, cfg)
    S = run.S
    cam_a, cam_b = cameras(aof, cfg, p)
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    a = SensorRig(aof, eng, run, aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0), gpu_device, cam_a, cfg)
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


# ---- 3. identity ----

@pytest.mark.parametrize("path", [1, 2])
def test_records_from_the_cameras_scalars_change_no_byte(aof, orc, synth, gpu_device, path):
    """S records of aof_bank_sensor_from_camera bound against nothing bound, on twin banks: six ticks, then two bursts of
    K = 3."""
    cfg, K = "px4-64", 3
    p, run = sref.case(aof, orc, synth, cfg, K=K)
    S, (cw, ch) = run.S, sref.UNIFORM[cfg]
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    cam = cameras(aof, cfg, p)[1]
    cam_run = cref.CameraRun(run, cw, ch, 9)
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    a, b = (BankRig(aof, eng, run, bp, gpu_device, camera=(cam, cam_run)) for _ in range(2))
    bursts = {rig: BankRig(aof, eng, run, bp, gpu_device, K=K, camera=(cam, cam_run), bank=rig.bank) for rig in (a, b)}
    table = table_tensor(gpu_device, aof.bank_sensor_from_camera(p, cam, n=S))
    given = counts_of(run, K, sref.T)
    published = 0
    for step in [("tick", k) for k in range(6)] + [("burst", 6), ("burst", 9)]:
        raws = []
        for rig, bound in ((a, True), (b, False)):
            used = rig if step[0] == "tick" else bursts[rig]
            eng.set_bank_sensors(table if bound else None, S, (used.K or 1) * S * cw * ch)
            ticks = [used.push(step[1])] if step[0] == "tick" else used.push(step[1] // K, given)
            raws.append(used.raw())
            published += sum(int((t.recs["quality"] >= 0).sum()) for t in ticks)
        assert raws[0] == raws[1], step
        assert a.bank_bytes() == b.bank_bytes(), step
    assert published > 2 * S
    eng.close()


# ---- 4. bursts ----

@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("cfg", ["px4-64", "opencv-128"])
def test_a_burst_equals_single_ticks_with_the_same_records(aof, orc, synth, gpu_device, cfg, path):
    """K = 3 with d_count and a padded round_stride against K single ticks on a twin bank: all outputs, all bank bytes."""
    K, T = 3, 24
    p, run = sref.case(aof, orc, synth, cfg, K=K)
    S = run.S
    cam_a = cameras(aof, cfg, p)[0]
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    ea, eb = aof.FlowEngine(p, 0), aof.FlowEngine(p, 0)
    ea.set_bank_path(path), eb.set_bank_path(path)
    a = SensorRig(aof, ea, run, bp, gpu_device, cam_a, cfg, K=K, pad=37)
    b = SensorRig(aof, eb, run, bp, gpu_device, cam_a, cfg)
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


# ---- 5. rotating buffers ----

@pytest.mark.parametrize("path", [1, 2])
def test_offsets_rewritten_every_tick_eager_and_through_a_replayed_graph(aof, orc, synth, gpu_device, path):
    """Every stream's frame alternates between two places of the buffer; the records are rewritten on the stream between
    the ticks.  Equal to rig B, eagerly and through a captured (linear) graph of the push replayed 16 times."""
    import torch
    cfg, T = "px4-64", 16
    engines, a, b = pair_of_rigs(aof, synth, orc, gpu_device, cfg, path, copies=2)
    S = a.run.S
    assert all(int(a.layouts[0][s]["offset"]) != int(a.layouts[1][s]["offset"]) for s in range(S))
    outs = []
    for k in range(T):
        for s in range(S):
            put(a.table, s, a.layouts[k % 2][s])
        a.load(k, which=k % 2), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, ("eager", k))
        outs.append(b.raw())
    final = b.bank_bytes()
    a.eng.bank_reset(a.bank)                     # (every kernel of the tick has run before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.enqueue()
    for k in range(T):
        for s in range(S):
            put(a.table, s, a.layouts[k % 2][s])
        a.load(k, which=k % 2)
        g.replay()
        assert a.raw() == outs[k], ("replay", k)
    assert a.bank_bytes() == final
    for e in engines:
        e.close()


# ---- 6. invalid records are refused safely ----

def invalid_records(good, camera_bytes):
    """One record per inequality of the rule, each at most a few bytes outside of what `good` describes.  (The test gives
    "offset > camera_bytes" to stream 2, whose whole frame fits the SLACK bytes behind the buffer.)"""
    edit = lambda **kw: sref.record(*[kw.get(n, int(good[n])) for n in ("offset", "pitch", "width", "height", "x0", "y0")])
    w, h = 64, 64
    return {"width < 1": edit(width=0), "height < 1": edit(height=0), "pitch < width": edit(pitch=int(good["width"]) - 1),
            "x0 < 0": edit(x0=-1), "y0 < 0": edit(y0=-1), "x0 + w > width": edit(x0=int(good["width"]) - w + 1),
            "y0 + h > height": edit(y0=int(good["height"]) - h + 1),
            "offset > camera_bytes": edit(offset=camera_bytes + 1), "extent": edit(offset=camera_bytes - sref.extent(good) + 1)}


@pytest.mark.parametrize("path", [1, 2])
def test_an_invalid_record_makes_the_stream_idle_with_its_own_quality(aof, orc, synth, gpu_device, path):
    """Per inequality: ticks 0..11 on twin banks, one stream's record invalid in one tick (A) against that stream inactive
    in that tick (C).  A's outputs are C's but for the quality of that record, the banks are equal after every tick (the
    stream's frame and state untouched), and behind the repair the stream goes on as one that was idle meanwhile."""
    cfg, T = "px4-64", 12
    p, run = sref.case(aof, orc, synth, cfg)[:2]
    S = run.S
    cam_a = cameras(aof, cfg, p)[0]
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    ea, ec = aof.FlowEngine(p, 0), aof.FlowEngine(p, 0)
    ea.set_bank_path(path), ec.set_bank_path(path)
    a, c = SensorRig(aof, ea, run, bp, gpu_device, cam_a, cfg), SensorRig(aof, ec, run, bp, gpu_device, cam_a, cfg)
    a.bind(), c.bind()
    for i, (what, _) in enumerate(invalid_records(a.recs[0], a.camera_bytes).items()):
        s = i % S
        assert what != "offset > camera_bytes" or sref.extent(a.recs[s]) + 1 <= SLACK + 64   # (what SensorRig allocates behind camera_bytes)
        bad = invalid_records(a.recs[s], a.camera_bytes)[what]
        assert not sref.valid(bad, 64, 64, a.camera_bytes) and sref.valid(a.recs[s], 64, 64, a.camera_bytes), what
        kb = next(k for k in range(6, T) if run.active[k, s])
        assert run.active[:kb, s].any() and run.active[kb + 1:T, s].any(), "the stream has frames in front of and behind the tick"
        ea.bank_reset(a.bank), ec.bank_reset(c.bank)
        for k in range(T):
            if k == kb:
                put(a.table, s, bad)
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
                put(a.table, s, a.recs[s])
            same_records(ga.recs, gc.recs, k, what)
            assert ga.wire == gc.wire and ga.exposure.tobytes() == gc.exposure.tobytes(), (what, k)
            assert ga.derotated.tobytes() == gc.derotated.tobytes(), (what, k)
            assert a.bank_bytes() == c.bank_bytes() and a.gate_bytes().tolist() == c.gate_bytes().tolist(), (what, k)
    ea.close(), ec.close()


@pytest.mark.parametrize("path", [1, 2])
def test_a_burst_whose_last_round_falls_outside_serves_the_rounds_before_it(aof, orc, synth, gpu_device, path):
    """K = 3, camera_bytes one byte short of round 2's last frame (stream 2's, the last in the buffer): rounds 0 and 1 are
    served, round 2 is AOF_TICK_BAD_SENSOR -- as a twin burst in which the stream has two frames.  The next burst, with
    the full size, equals the twin's."""
    cfg, K = "px4-64", 3
    p, run = sref.case(aof, orc, synth, cfg, K=K)
    S, last = run.S, sref.TABLES[cfg][1][-1]
    cam_a = cameras(aof, cfg, p)[0]
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    ea, ec = aof.FlowEngine(p, 0), aof.FlowEngine(p, 0)
    ea.set_bank_path(path), ec.set_bank_path(path)
    a, c = (SensorRig(aof, e, run, bp, gpu_device, cam_a, cfg, K=K, pad=16) for e in (ea, ec))
    a.bind(), c.bind()
    given = counts_of(run, K, sref.T)
    jb = next(j for j in range(1, len(given) - 1) if given[j, last] == K)
    for j in range(jb + 2):
        twin = given.copy()
        if j == jb:
            a.bind(a.camera_bytes - 1)
            twin[j, last] = K - 1
        ga, gc = a.push(j, given), c.push(j, twin)
        if j == jb:
            assert [int(t.recs[last]["quality"]) for t in gc][K - 1] == aof.TICK_IDLE
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

def ingest_case(aof, gpu_device, recs, w, h, nbytes, bad=(), want_cropped=True, want_hist=True, skew=0):
    """aof_ingest_sensors_device on a noise buffer of nbytes + SLACK bytes (the library is told nbytes), into dirty
    Guarded outputs, against crop() and ingest_ref's numpy histogram of every frame whose record is valid."""
    import torch
    n = len(recs)
    buf = np.random.default_rng(n * 131 + w).integers(0, 256, nbytes + SLACK, dtype=np.uint8)
    buf[::7] = 255                                          # values cv::calcHist drops
    cam = up(gpu_device, buf)
    crops = Guarded(gpu_device, (n, h, w), skew=skew) if want_cropped else None
    hist = Guarded(gpu_device, (n, 40)) if want_hist else None
    ok = Guarded(gpu_device, (n,))
    aof.ingest_sensors(cam, table_tensor(gpu_device, recs), w, h, camera_bytes=nbytes, cropped=crops.tensor if crops else None,
                       hist=hist.tensor.view(torch.int32) if hist else None, ok=ok.tensor, want_cropped=False, want_hist=False)
    torch.cuda.synchronize()
    flags = ok.read()
    assert flags.tolist() == [0 if i in bad else 1 for i in range(n)], flags
    assert [sref.valid(r, w, h, nbytes) for r in recs] == [i not in bad for i in range(n)]
    got_c = crops.read() if crops else None
    got_h = hist.read().view("<u4") if hist else None
    for i in range(n):
        if i in bad:
            continue
        want_c = sref.crop(buf, recs[i], w, h)
        if crops:
            same(got_c[i], want_c, ("crop", i))
        if hist:
            same(got_h[i], ingest_ref.ingest(want_c, w, h)[1], ("histogram", i))
    if hist and h <= 128 and bad:
        assert all(untouched(got_h[i]) for i in bad), "one workgroup per frame: a refused frame's histogram is not written"


def test_ingest_by_records_at_every_alignment_and_an_odd_pitch(aof, gpu_device):
    """16 frames of a 100 x 70 sensor at pitch 131 whose offset + x0 covers every residue mod 16; frame 5's record ends
    one byte behind the buffer."""
    recs, cursor = np.zeros(16, sref.SENSOR_DTYPE), 0
    for i in range(16):
        x0, y0 = (5 * i) % 37, i % 7
        off = cursor + (i - x0 - cursor) % 16
        recs[i] = sref.record(off, 131, 100, 70, x0, y0)
        assert (off + x0) % 16 == i
        cursor = off + sref.extent(recs[i])
    recs[5]["offset"] = cursor - sref.extent(recs[5]) + 1
    for kw in (dict(), dict(want_cropped=False), dict(want_hist=False), dict(skew=3)):
        ingest_case(aof, gpu_device, recs, 64, 64, cursor, bad=(5,), **kw)


def test_ingest_by_records_on_the_scalar_path_and_on_two_strips(aof, gpu_device):
    """A crop width that is no multiple of 16; and a 192-row crop: two workgroups per frame, the histogram through the
    zeroing pass (a refused frame's is then zero)."""
    recs = np.array([sref.record(3, 83, 70, 60, 11, 9), sref.record(6000, 70, 70, 50, 20, 10), sref.record(11003, 97, 61, 47, 0, 0)])
    ingest_case(aof, gpu_device, recs, 50, 40, 11003 + 46 * 97 + 61)
    recs = np.array([sref.record(1, 83, 80, 200, 9, 5), sref.record(17000, 64, 64, 192, 0, 0), sref.record(30007, 131, 100, 193, 36, 1),
                     sref.record(30007, 131, 100, 193, 37, 1)])
    ingest_case(aof, gpu_device, recs, 64, 192, 30007 + 192 * 131 + 100, bad=(3,))


# ---- 8. the facade ----

def test_the_facade_with_stream_sensors_equals_an_object_fed_uniform_frames(aof, orc, synth, gpu_device):
    """OpticalFlowBank, S = 5, 64 x 64, enableCamera(320, 240): one object with setStreamSensor on the table's layouts and
    the mixed buffer, one without, fed uniform frames with the same crops: entries by raw bytes, exposure commands."""
    cfg, T = "px4-64", 24
    p, run = sref.case(aof, orc, synth, cfg)[:2]
    S, (cw, ch) = run.S, (320, 240)
    recs, nbytes = sref.layout(*sref.TABLES[cfg], 64, 64)
    staging = S * cw * ch
    assert nbytes <= staging
    uniform = cref.CameraRun(run, cw, ch, 9)
    a, b = (aof.OpticalFlowBank(FX, FY, 15, 64, 64, S) for _ in range(2))
    for bank in (a, b):
        assert bank.engineOk(), bank.lastError()
        bank.setTimestampOffset(OFFSET)
    args = lambda r: [int(r[n]) for n in ("offset", "pitch", "width", "height", "x0", "y0")]
    assert a.setStreamSensor(0, *args(recs[0])) == EINVAL, "not before enableCamera()"
    for bank in (a, b):
        assert bank.enableCamera(cw, ch, 100, 4, INTERVAL) == 0, bank.lastError()
    for s in range(S):
        assert a.setStreamSensor(s, *args(recs[s])) == 0, a.lastError()
    assert a.setStreamSensor(-1, *args(recs[0])) == EINVAL and a.setStreamSensor(S, *args(recs[0])) == EINVAL
    entries_seen = commands_seen = 0
    for k in range(T):
        if k == 7:     # refused: one byte behind the staging buffer, a crop outside the sensor; the object is as it was
            assert a.setStreamSensor(1, staging - sref.extent(recs[1]) + 1, *args(recs[1])[1:]) == EINVAL
            assert a.setStreamSensor(2, *(args(recs[2])[:4] + [1, 0])) == EINVAL and a.engineOk()
        buf = np.zeros(staging, np.uint8)
        buf[:nbytes] = sref.pack(recs, run.frames[k], nbytes, [3, k])
        na, ea = a.pushCamera(buf, run.times[k], run.active[k], run.gyro[k])
        nb, eb = b.pushCamera(uniform.sensor(k), run.times[k], run.active[k], run.gyro[k])
        assert na == nb >= 0, (k, a.lastError(), b.lastError())
        assert ea.tobytes() == eb.tobytes(), ("entries", k)
        ca, cb = a.exposureCommands(), b.exposureCommands()
        assert ca.tobytes() == cb.tobytes(), ("exposure commands", k)
        entries_seen += na
        commands_seen += int((cb["flags"] != 0).sum())
    assert entries_seen > 2 * S and commands_seen > S
    a.close(), b.close()


def test_the_facade_takes_a_sensor_record_set_between_ticks_from_that_tick(aof, synth, gpu_device):
    """OpticalFlowBank, S = 2, 64 x 64, rate 0, four ticks: object A with enableCamera(80, 80) and no setter before the
    first tick; setStreamSensor() before tick 2 -- the first copy of the shadow records and their binding, between two
    ticks -- moves stream 1's crop from the centre to the corner.  Object B with enableCamera(64, 64) is fed the crops
    the host cuts: entries and exposure commands by raw bytes at every tick."""
    S, T, w, cw = 2, 4, 64, 80
    seqs = [synth.make_sequence(cw, cw, T, 4, seed=181000 + s, max_step=3)[0] for s in range(S)]
    a, b = (aof.OpticalFlowBank(FX, FY, 0, w, w, S) for _ in range(2))
    for bank, size in ((a, cw), (b, w)):
        assert bank.engineOk(), bank.lastError()
        bank.setTimestampOffset(OFFSET)
        assert bank.enableCamera(size, size, 100, 4, INTERVAL) == 0, bank.lastError()
    centre = (cw - w) // 2
    entries_seen = 0
    for k in range(T):
        if k == 2:
            assert a.setStreamSensor(1, 1 * cw * cw, cw, cw, cw, 0, 0) == 0, a.lastError()
        sensor = np.stack([q[k] for q in seqs])
        origin = [centre, centre if k < 2 else 0]
        crops = np.stack([sensor[s, o:o + w, o:o + w] for s, o in enumerate(origin)])
        times = np.full(S, 12_000 * (k + 1), np.uint64)
        na, ea = a.pushCamera(sensor, times)
        nb, eb = b.pushCamera(crops, times)
        assert na == nb >= 0, (k, a.lastError(), b.lastError())
        assert ea.tobytes() == eb.tobytes(), ("entries", k)
        assert a.exposureCommands().tobytes() == b.exposureCommands().tobytes(), ("exposure commands", k)
        entries_seen += na
    assert entries_seen >= 2 * (T - 1)
    a.close(), b.close()


# ---- bindings and refusals ----

def test_bindings_and_refusals(aof, orc, synth, gpu_device):
    """Every -EINVAL of aof_set_bank_sensors with the binding left as it was; a camera push of another stream count is
    refused and writes nothing; the pushes of pre-cropped frames do not look at the binding; unbinding restores the
    scalars."""
    import torch
    cfg = "px4-64"
    p, run = sref.case(aof, orc, synth, cfg)[:2]
    S = run.S
    cam_a, cam_b = cameras(aof, cfg, p)
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    eng, eb = aof.FlowEngine(p, 0), aof.FlowEngine(p, 0)
    a = SensorRig(aof, eng, run, bp, gpu_device, cam_a, cfg)
    b = BankRig(aof, eb, run, bp, gpu_device, camera=(cam_b, cref.CameraRun(run, *sref.UNIFORM[cfg], 9)))
    a.bind()
    setter = aof.lib.aof_set_bank_sensors
    base = a.table.data_ptr()
    assert setter(None, base, S, a.camera_bytes) == EINVAL
    assert setter(eng._ctx, base + 8, S, a.camera_bytes) == EINVAL and b"16-byte" in aof.lib.aof_last_error(eng._ctx)
    assert setter(eng._ctx, base, 0, a.camera_bytes) == EINVAL and setter(eng._ctx, base, -1, a.camera_bytes) == EINVAL
    assert setter(eng._ctx, base, S, 0) == EINVAL and b"camera_bytes" in aof.lib.aof_last_error(eng._ctx)
    for k in range(3):                            # the binding is as it was: the mixed layouts are served
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, ("after the refusals", k))
    # an array for S - 1 streams: the camera push is refused and writes nothing, the plain push does not look at it
    assert setter(eng._ctx, base, S - 1, a.camera_bytes) == 0
    snapshot = a.bank.buffer.clone()
    a.load(3)
    with pytest.raises(aof.AofError) as e:
        a.enqueue()
    assert e.value is not None
    assert b"aof_set_bank_sensors" in aof.lib.aof_last_error(eng._ctx)
    torch.cuda.synchronize()
    assert torch.equal(a.bank.buffer, snapshot) and all(untouched(g.read()) for g in (a.outputs[0], a.outputs[3], a.outputs[4]))
    fresh = eng.bank_create(bp, gpu_device)
    plain = eng.bank_push(fresh, up(gpu_device, run.frames[3]), up(gpu_device, run.times[3]), up(gpu_device, run.active[3]))
    torch.cuda.synchronize()
    q = aof.ticks_view(plain)["quality"]
    assert (q == np.where(run.active[3] != 0, 0, aof.TICK_IDLE)).all(), "the plain push on pre-cropped frames, whatever is bound"
    # unbound: the scalars again -- a rig with uniform frames on the same engine and bank
    eng.set_bank_sensors(None)
    u = BankRig(aof, eng, run, bp, gpu_device, camera=(cam_b, cref.CameraRun(run, *sref.UNIFORM[cfg], 9)), bank=a.bank)
    a.bank.camera = cam_b
    for k in (4, 5):
        u.load(k), u.enqueue()
        b.load(k), b.enqueue()
        same_rigs(u, b, ("unbound", k))
    eng.close(), eb.close()
