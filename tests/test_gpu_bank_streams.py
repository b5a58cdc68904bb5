"""The stream bank with per-stream cameras (aof_bank_stream / aof_set_bank_streams, include/aof.h): S streams with their
own focal lengths, output rate, vehicle-time offset and MAVLink identity, against one oracle chain per stream built with
that stream's values (tests/bank_streams_ref.py) -- records and wire frames by bytes, never by tolerance.  The scalars of
aof_bank_params hold values no stream has: a kernel that still reads them cannot pass.  The rig: tests/bank_rig.py."""
import ctypes as C
from functools import partial

import numpy as np
import pytest

import bank_ref as ref
import bank_streams_ref as sref
from bank_ref import FX, FY
from bank_rig import EINVAL, BankRig, burstable, counts_of, params_of, put, same_records, untouched, up
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

# what bp carries while an array is bound: checked as ever (focal lengths > 0), used by nobody
UNUSED = dict(focal_x=51.5, focal_y=49.25, output_rate=7, offset_timestamp_usec=31337, system_id=77, component_id=78, first_seq=79)
SENSOR = (96, 80)   # sensor frames of the camera forms: centre-cropped to 64 x 64


def bind(aof, eng, dev, recs, n_streams=None):
    """Binds the BANK_STREAM_DTYPE array `recs`; returns the device tensor [n, 32] (rewrite it with put())."""
    t = up(dev, recs.view(np.uint8).reshape(len(recs), 32))
    assert t.data_ptr() % 16 == 0
    eng.set_bank_streams(t, n_streams)
    return t


def sensors_of(frames, seed):
    """Sensor frames [.., 80, 96] of noise whose centre crop is frames [.., 64, 64]."""
    cw, ch = SENSOR
    out = np.random.default_rng(seed).integers(0, 256, frames.shape[:-2] + (ch, cw), dtype=np.uint8)
    h, w = frames.shape[-2:]
    y0, x0 = ch // 2 - h // 2, cw // 2 - w // 2
    out[..., y0:y0 + h, x0:x0 + w] = frames
    return out


class NoiseSensors:
    """The sensor frames of a run for BankRig: tick k's are sensors_of(run.frames[k], seed + k)."""
    cam_w, cam_h = SENSOR

    def __init__(self, run, seed):
        self.run, self.seed = run, seed

    def sensor(self, k):
        return sensors_of(self.run.frames[k], self.seed + k)


_expected = {}


def expected(aof, orc, synth, cfg, S, T, seed, K=None, rows=None):
    """The run and the oracle's records and wire frames, computed once per case and left unchanged."""
    key = (cfg, S, T, seed, K)
    if key not in _expected:
        p = params_of(aof, cfg)
        run = ref.make_run(synth, p.width, p.height, S, T, seed)
        if K:
            run = burstable(run, K)
        _expected[key] = (p, run) + sref.expected(aof, orc, p, run, rows)
    return _expected[key]


def check_tick(got, want, wire, k, what):
    same_records(got.recs, want[k], k, what)
    assert got.wire == wire[k], (what, "wire", k, [s for s in range(len(wire[k])) if got.wire[s] != wire[k][s]][:4])


# ---- 1. oracle parity ----

@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("cfg,seed", [("px4-64", 71), ("opencv-128", 72)])
def test_six_different_cameras_equal_one_oracle_chain_each(aof, orc, synth, gpu_device, cfg, seed, path):
    """S = 6, T = 48, the table of the issue: records and wire frames byte for byte, the stored frames, idle streams
    untouched.  (The census on this input: tests/test_bank_streams_ref.py.)"""
    S, T = 6, 48
    p, run, want, wire = expected(aof, orc, synth, cfg, S, T, seed)
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    rig = BankRig(aof, eng, run, aof.bank_params(S, **UNUSED), gpu_device)
    bind(aof, eng, gpu_device, sref.records(aof, S))
    px = p.width * p.height
    for k in range(T):
        before_frames, before_state = rig.bank.frames_bytes(), rig.bank.state_bytes()
        check_tick(rig.push(k), want, wire, k, "oracle")
        after_frames, after_state = rig.bank.frames_bytes(), rig.bank.state_bytes()
        for s in range(S):
            slot = slice(s * px, (s + 1) * px)
            if run.active[k, s]:
                assert after_frames[slot].tobytes() == run.frames[k, s].tobytes(), ("stored frame", k, s)
            else:
                assert after_frames[slot].tobytes() == before_frames[slot].tobytes(), ("idle frame", k, s)
                assert after_state[s].tobytes() == before_state[s].tobytes(), ("idle state", k, s)
    assert not any(w[3] for w in wire) and any(w[1] for w in wire), "stream 3 (offset 0) never sends, stream 1 does"
    eng.close()


# ---- 2. the all-equal twin ----

@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("camera", [False, True], ids=["frames", "sensor"])
def test_an_array_of_from_params_records_changes_no_byte(aof, synth, gpu_device, camera, path):
    """S = 5: six ticks and two bursts of K = 3 with S copies of aof_bank_stream_from_params(bp) bound, against the
    unbound calls on a twin bank: every output and the banks' frames and state regions identical."""
    S, K, T = 5, 3, 12
    p = params_of(aof, "px4-64")
    run = burstable(ref.make_run(synth, 64, 64, S, T, 81), K)
    bp = aof.bank_params(S, 180.5, 222.25, 15, 5_000_000, 3, 42, 251)
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    cam = (aof.bank_camera_params(SENSOR[0], SENSOR[1], 64, 64, exposure_interval_us=30000), NoiseSensors(run, 7)) if camera else None
    a, b = BankRig(aof, eng, run, bp, gpu_device, camera=cam), BankRig(aof, eng, run, bp, gpu_device, camera=cam)
    bursts = {rig: BankRig(aof, eng, run, bp, gpu_device, K=K, camera=cam, bank=rig.bank) for rig in (a, b)}
    given = counts_of(run, K)
    table = up(gpu_device, aof.bank_stream_from_params(bp, S).view(np.uint8).reshape(S, 32))
    published = held = 0
    for step in [("tick", k) for k in range(6)] + [("burst", 6), ("burst", 9)]:
        outs = []
        for rig, bound in ((a, True), (b, False)):
            eng.set_bank_streams(table if bound else None)
            used = rig if step[0] == "tick" else bursts[rig]
            ticks = [used.push(step[1])] if step[0] == "tick" else used.push(step[1] // K, given)
            outs.append((ticks, used.raw()))                  # (raw: the lengths and the exposure records among them)
        (ga, raw_a), (gb, raw_b) = outs
        recs = np.stack([t.recs for t in ga])
        assert recs.tobytes() == np.stack([t.recs for t in gb]).tobytes(), step
        assert [t.wire for t in ga] == [t.wire for t in gb] and raw_a == raw_b, step
        assert all(untouched(t.exposure) != camera for t in ga), step
        assert a.bank_bytes() == b.bank_bytes(), step
        published += int((recs["quality"] >= 0).sum())
        held += int((recs["quality"] == aof.TICK_HELD).sum())
        assert sum(1 for t in ga for w in t.wire if w) == int((recs["quality"] >= 0).sum()), "every published record is sent"
    assert published > S and held > S, (published, held)
    eng.close()


# ---- 3. a burst indexes the array by the stream ----

@pytest.mark.parametrize("path", [1, 2])
def test_a_burst_reads_the_record_of_the_stream_not_of_the_round(aof, orc, synth, gpu_device, path):
    """K = 3, S = 5, five different cameras; the device array has K * S records, the first S real, the others a decoy:
    a kernel that indexed by round * S + stream would produce the decoy's bytes, not fault.  Against three single
    ticks on a twin bank and against the oracle chains."""
    S, K, T = 5, 3, 12
    p, run, want, wire = expected(aof, orc, synth, "px4-64", S, T, 91, K=K)
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    a, b = BankRig(aof, eng, run, aof.bank_params(S, **UNUSED), gpu_device, K=K), BankRig(aof, eng, run, aof.bank_params(S, **UNUSED), gpu_device)
    given = counts_of(run, K)
    recs = sref.records(aof, K * S, [sref.TABLE[s] for s in range(S)] + [sref.DECOY] * ((K - 1) * S))
    bind(aof, eng, gpu_device, recs, n_streams=S)
    later = 0
    for k0 in range(0, T, K):
        got = a.push(k0 // K, given)
        for j in range(K):
            one = b.push(k0 + j)
            assert got[j].recs.tobytes() == one.recs.tobytes(), ("twin", k0, j)
            assert got[j].wire == one.wire, ("twin wire", k0, j)
            same_records(got[j].recs, want[k0 + j], k0 + j, "oracle")
            assert got[j].wire == wire[k0 + j], ("oracle wire", k0, j)
            if j:
                later += int((got[j].recs["quality"] >= 0).sum())
        assert a.bank_bytes() == b.bank_bytes(), k0
    assert later > S, "records published in rounds behind the first: where a round-indexed read would go wrong"
    eng.close()


# ---- 4. more than one wave of streams ----

@pytest.mark.parametrize("path", [1, 2])
def test_seventy_streams_cycle_through_the_table(aof, orc, synth, gpu_device, path):
    S, T = 70, 8
    p, run, want, wire = expected(aof, orc, synth, "px4-64", S, T, 101)
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    rig = BankRig(aof, eng, run, aof.bank_params(S, **UNUSED), gpu_device)
    bind(aof, eng, gpu_device, sref.records(aof, S))
    for k in range(T):
        check_tick(rig.push(k), want, wire, k, "oracle")
    pub, held, _ = ref.census(want)
    assert held.sum() > 0 and (pub > 1).any() and sum(1 for w in wire[T - 1] if w) > 6
    eng.close()


# ---- 5. records rewritten between ticks ----

@pytest.mark.parametrize("path", [1, 2])
def test_a_record_rewritten_between_ticks_applies_from_that_tick(aof, orc, synth, gpu_device, path):
    """Behind tick 10 stream 2 gets other focal lengths, another identity and another offset; its rate stays.  The limiter
    sums pixels, so two oracle chains fed the same frames -- old values, new values -- hold and publish alike: the
    stream equals the old chain before the change and the new chain from it on.  The new chain has counted its
    messages from the start, like the bank: the sequence number runs on from the new first_seq, here through 255."""
    S, T, CHANGE = 6, 30, 10
    p, run, want, wire = expected(aof, orc, synth, "px4-64", S, T, 111)
    old = sref.TABLE[2]
    before = int((want[:CHANGE, 2]["quality"] >= 0).sum())          # messages of stream 2 when its record changes
    new = (150.0, 90.5, old[2], 1 << 33, 42, 7, (250 - before) & 0xFF)   # (the first frame behind the change is number 250)
    chain_b = sref.chain(aof, orc, p, new)
    want_b, wire_b = ref.expected(ref.Run(run.frames[:, 2:3], run.times[:, 2:3], run.gyro[:, 2:3], run.active[:, 2:3]), [chain_b])
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    rig = BankRig(aof, eng, run, aof.bank_params(S, **UNUSED), gpu_device)
    table = bind(aof, eng, gpu_device, sref.records(aof, S))
    seqs = []
    for k in range(T):
        if k == CHANGE:
            put(table, 2, sref.records(aof, 1, [new])[0])
        w_k, x_k = want[k].copy(), list(wire[k])
        if k >= CHANGE:
            w_k[2], x_k[2] = want_b[k, 0], wire_b[k][0]
        got = rig.push(k)
        same_records(got.recs, w_k, k, "oracle")
        assert got.wire == x_k, (k, [s for s in range(S) if got.wire[s] != x_k[s]])
        if k >= CHANGE and got.wire[2]:
            assert got.wire[2][5:7] == bytes([42, 7])
            seqs.append(got.wire[2][4])
    assert (want[CHANGE:, 2]["flow_x"] != want_b[CHANGE:, 0]["flow_x"]).any(), "the two focal lengths give other angles"
    assert before > 0 and len(seqs) > 8 and seqs[:8] == [250, 251, 252, 253, 254, 255, 0, 1]
    assert 255 in seqs and 0 in seqs, seqs
    eng.close()


# ---- 6. a captured tick reads the array at replay ----

def test_a_captured_tick_uses_what_the_array_holds_at_replay(aof, synth, gpu_device):
    """Path 1, S = 5: one tick captured with an array bound, replayed for 14 ticks; behind replay 6 every record is
    rewritten (the table turned round).  Equal to the eager run with the same rewrite, and the frames carry the new
    identities from replay 7 on."""
    import torch
    S, T, CHANGE = 5, 14, 7
    p = params_of(aof, "px4-64")
    run = ref.make_run(synth, 64, 64, S, T, 121)
    first, second = sref.records(aof, S), sref.records(aof, S, [sref.TABLE[(4 - s)] for s in range(S)])
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(1)
    table = bind(aof, eng, gpu_device, first)
    rewrite = lambda recs: table.copy_(up(gpu_device, recs.view(np.uint8).reshape(S, 32)))
    eager = BankRig(aof, eng, run, aof.bank_params(S, **UNUSED), gpu_device)
    outs = []
    for k in range(T):
        if k == CHANGE:
            rewrite(second)
        outs.append(eager.push(k))
    rewrite(first)
    rig = BankRig(aof, eng, run, aof.bank_params(S, **UNUSED), gpu_device)
    rig.push(0)                                  # (the tick kernel has run once before the capture)
    eng.bank_reset(rig.bank)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rig.enqueue()
    new_ids = 0
    for k in range(T):
        if k == CHANGE:
            rewrite(second)
        rig.load(k)
        g.replay()
        got = rig.read()
        assert got.recs.tobytes() == outs[k].recs.tobytes(), k
        sent = got.wire
        assert sent == outs[k].wire, k
        for s, f in enumerate(sent):
            if f:
                want_id = bytes((second if k >= CHANGE else first)[s].tobytes()[12:14])
                assert f[5:7] == want_id, (k, s)
                new_ids += k >= CHANGE
    assert new_ids > S
    assert rig.bank_bytes() == eager.bank_bytes()
    eng.close()


# ---- 7. the IMU call takes the identity from the array ----

def test_the_imu_call_sends_with_each_stream_s_identity(aof, synth, gpu_device):
    """Records-only bursts (K = 2) and aof_bank_imu_device with an array bound, S = 5, M = 4, against aof_bank_imu_host
    called once per stream with n_streams = 1, that stream's triple and that stream's samples repacked to [K][M][1]."""
    import torch
    S, K, M, T = 5, 2, 4, 8
    p = params_of(aof, "px4-64")
    run = burstable(ref.make_run(synth, 64, 64, S, T, 131), K)
    eng = aof.FlowEngine(p, 0)
    bank = eng.bank_create(aof.bank_params(S, **UNUSED), gpu_device)
    bind(aof, eng, gpu_device, sref.records(aof, S))
    state = torch.zeros((S, 64), dtype=torch.uint8, device=gpu_device)
    eng.bank_imu_reset(state, offset0=0)
    states = np.zeros(S, aof.IMU_STATE_DTYPE)
    rng = np.random.default_rng(7)
    clock = np.full(S, 10 ** 9, np.int64)
    sent = 0
    for k0 in range(0, T, K):
        rounds = slice(k0, k0 + K)
        samples = np.zeros((K, M, S), aof.IMU_SAMPLE_DTYPE)
        counts = rng.integers(1, M + 1, (K, S)).astype(np.uint8)
        for k in range(K):
            for s in range(S):
                for j in range(counts[k, s]):
                    clock[s] += int(rng.integers(2000, 3000))
                    samples[k, j, s] = (clock[s], *rng.normal(0, 0.8, 3).astype(np.float32), 0)
        count = run.active[rounds].sum(axis=0).astype(np.uint8)
        times = up(gpu_device, run.times[rounds])
        records = eng.bank_push_burst(bank, K, up(gpu_device, run.frames[rounds]), times, up(gpu_device, count), None)
        pushed = records.cpu().numpy().view(aof.TICK_DTYPE).reshape(K, S).copy()
        out, frames, lens = eng.bank_imu(up(gpu_device, samples.view(np.uint8).reshape(K, M, S, 24)), times, records, state,
                                         up(gpu_device, counts), system_id=UNUSED["system_id"], component_id=UNUSED["component_id"],
                                         first_seq=UNUSED["first_seq"])
        torch.cuda.synchronize()
        got_r = out.cpu().numpy().view(aof.TICK_DTYPE).reshape(K, S)
        got_f, got_n, got_s = frames.cpu().numpy(), lens.cpu().numpy(), aof.imu_states_view(state)
        for s in range(S):
            sysid, compid, seq = sref.TABLE[s][4:7]
            st = states[s:s + 1].copy()
            wr, wf, wn = aof.bank_imu_host(samples[:, :, s:s + 1], counts[:, s:s + 1], run.times[rounds][:, s:s + 1].astype(np.uint64),
                                           np.ascontiguousarray(pushed[:, s:s + 1]), st, sysid, compid, seq)
            states[s] = st[0]
            assert got_r[:, s].tobytes() == wr[:, 0].tobytes(), (k0, s)
            assert got_n[:, s].tobytes() == wn[:, 0].tobytes(), (k0, s)
            for k in range(K):
                n = int(wn[k, 0])
                assert got_f[k, s, :n].tobytes() == wf[k, 0, :n].tobytes(), (k0, k, s)
                if n:
                    assert got_f[k, s, 5:7].tobytes() == bytes([sysid, compid])
                    sent += 1
            assert got_s[s].tobytes() == states[s].tobytes(), (k0, s)
    assert sent >= 2 * S, sent
    eng.close()


# ---- 8. arguments ----

def test_a_binding_of_another_stream_count_is_refused_and_unbinding_restores_the_scalars(aof, synth, gpu_device):
    import torch
    S = 5
    p = params_of(aof, "px4-64")
    run = ref.make_run(synth, 64, 64, S, 6, 141)
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000, 1, 100, 3)
    eng = aof.FlowEngine(p, 0)
    a, b = BankRig(aof, eng, run, bp, gpu_device), BankRig(aof, eng, run, bp, gpu_device)     # b: never sees a binding
    for k in range(3):
        a.push(k), b.push(k)
    big = torch.zeros((S + 2) * 32 + 16, dtype=torch.uint8, device=gpu_device)
    base = big.data_ptr()
    assert base % 16 == 0
    set_streams = aof.lib.aof_set_bank_streams
    assert set_streams(eng._ctx, base + 8, S) == EINVAL and b"16-byte" in aof.lib.aof_last_error(eng._ctx), "a misaligned array"
    assert set_streams(eng._ctx, base, 0) == EINVAL and set_streams(eng._ctx, base, -1) == EINVAL
    # (nothing is bound yet: the refused calls left the context as it was)
    assert a.push(3).recs.tobytes() == b.push(3).recs.tobytes()
    assert set_streams(eng._ctx, base, S + 1) == 0                          # an array for six streams
    snapshot = a.bank.buffer.clone()
    stream = torch.cuda.current_stream().cuda_stream
    d = gpu_device
    recs = torch.full((S, 48), 0xEE, dtype=torch.uint8, device=d)
    wire, lens = torch.full((S, 56), 0xEE, dtype=torch.uint8, device=d), torch.full((S,), 0xEE, dtype=torch.uint8, device=d)
    frames, times = up(d, run.frames[4]), up(d, run.times[4])
    rc = aof.lib.aof_bank_push_device(eng._ctx, C.byref(bp), frames.data_ptr(), times.data_ptr(), None, None, a.bank.buffer.data_ptr(),
                                      a.bank.buffer.numel(), recs.data_ptr(), wire.data_ptr(), lens.data_ptr(), stream)
    assert rc == EINVAL and b"aof_set_bank_streams" in aof.lib.aof_last_error(eng._ctx)
    burst = aof.bank_burst_params(1)
    rc = aof.lib.aof_bank_push_burst_device(eng._ctx, C.byref(bp), C.byref(burst), frames.data_ptr(), times.data_ptr(), None, None,
                                            a.bank.buffer.data_ptr(), a.bank.buffer.numel(), recs.data_ptr(), wire.data_ptr(),
                                            lens.data_ptr(), stream)
    assert rc == EINVAL
    ip = aof.imu_params(S, 1, 2)
    samples, state = torch.zeros((2, S, 24), dtype=torch.uint8, device=d), torch.full((S, 64), 0xEE, dtype=torch.uint8, device=d)
    rin = torch.zeros((S, 48), dtype=torch.uint8, device=d)
    rc = aof.lib.aof_bank_imu_device(eng._ctx, C.byref(ip), samples.data_ptr(), None, times.data_ptr(), rin.data_ptr(), state.data_ptr(),
                                     recs.data_ptr(), wire.data_ptr(), lens.data_ptr(), stream)
    assert rc == EINVAL and b"aof_set_bank_streams" in aof.lib.aof_last_error(eng._ctx)
    torch.cuda.synchronize()
    assert torch.equal(a.bank.buffer, snapshot), "a refused push leaves the bank untouched"
    for t in (recs, wire, lens, state):
        assert bool((t == 0xEE).all()), "a refused call writes nothing"
    # an array of the right count is accepted: one heterogeneous tick on a bank of its own carries the table's identities
    c = BankRig(aof, eng, run, bp, gpu_device)
    bind(aof, eng, gpu_device, sref.records(aof, S))
    first = c.push(4)                                                       # (every stream's first frame: published)
    for s in range(S):
        if run.active[4, s]:
            assert (first.wire[s][5:7] == bytes(sref.TABLE[s][4:6])) if sref.TABLE[s][3] else first.wire[s] == b"", s
    assert sum(1 for w in first.wire if w) >= 2
    # unbound again: the scalars, byte for byte what the bank without a binding gives
    eng.set_bank_streams(None)
    for k in (4, 5):
        ga, gb = a.push(k), b.push(k)
        assert ga.recs.tobytes() == gb.recs.tobytes() and ga.wire == gb.wire, k
    assert a.bank_bytes() == b.bank_bytes()
    eng.close()


# ---- 9. the facade ----

def test_the_facade_with_setters_equals_one_opencv_object_per_camera(aof, synth, gpu_device):
    """OpticalFlowBank, S = 4, T = 48, every stream given its table row through the setters: per stream its entries are
    the non-negative calcFlow returns of one OpticalFlowOpenCV(fx_s, fy_s, rate_s) object, with gyro sums and whole
    frames from the identity-aware Python packer.  A second object, no setter called, gives what it always gave."""
    S, T, w = 4, 48, 128
    run = ref.make_run(synth, w, w, S, T, 151)
    bank = aof.OpticalFlowBank(FX, FY, 15, w, w, S)
    assert bank.engineOk(), bank.lastError()
    for bad in (-1, S):
        assert bank.setStreamFocalLength(bad, 1.0, 1.0) == EINVAL and bank.setStreamOutputRate(bad, 5) == EINVAL
        assert bank.setStreamIdentity(bad, 1, 2, 3) == EINVAL and bank.setStreamTimestampOffset(bad, 9) == EINVAL
    assert bank.setStreamFocalLength(0, 0.0, 1.0) == EINVAL
    bank.setTimestampOffset(sref.TABLE[0][3])
    singles, chains = [], []
    for s in range(S):
        fx, fy, rate, offset, sysid, compid, seq = sref.TABLE[s]
        if s:                              # (stream 0 keeps the constructor's values: its row is the repository's default)
            assert bank.setStreamFocalLength(s, fx, fy) == 0 and bank.setStreamOutputRate(s, rate) == 0
            assert bank.setStreamIdentity(s, sysid, compid, seq) == 0 and bank.setStreamTimestampOffset(s, offset) == 0
        f = aof.OpticalFlowOpenCV(fx, fy, rate, w, w)
        singles.append(f)
        chains.append(ref.Chain(aof.TICK_DTYPE, f.calcFlow, partial(sref.py_frame_id, system_id=sysid, component_id=compid), offset, seq))
    want, wire = ref.expected(run, chains)
    plain = aof.OpticalFlowBank(FX, FY, 15, w, w, S)
    plain.setTimestampOffset(5_000_000)
    plain_singles = [aof.OpticalFlowOpenCV(FX, FY, 15, w, w) for _ in range(S)]
    plain_want, plain_wire = ref.expected(run, [ref.Chain(aof.TICK_DTYPE, f.calcFlow, sref.py_frame_id, 5_000_000, 0) for f in plain_singles])
    entries_seen = 0
    for k in range(T):
        n, entries = bank.push(run.frames[k], run.times[k], run.active[k], run.gyro[k])
        assert n == len(entries) >= 0, bank.lastError()
        assert list(entries["stream"]) == list(np.flatnonzero(want[k]["quality"] >= 0)), k
        for e in entries:
            s = int(e["stream"])
            for name in ("quality", "dt_us", "flow_x", "flow_y", "gyro_x", "gyro_y", "gyro_z"):
                assert e["record"][name].tobytes() == want[k, s][name].tobytes(), (k, s, name)
            ln = int(e["mavlink_len"])
            assert bytes(e["mavlink"][:ln]) == wire[k][s], (k, s)
        entries_seen += n
        # the object without a setter: what it always gave, every stream, every field, whole frames with identity 1 / 100
        n, entries = plain.push(run.frames[k], run.times[k], run.active[k], run.gyro[k])
        assert n == len(entries) and list(entries["stream"]) == list(np.flatnonzero(plain_want[k]["quality"] >= 0)), k
        for e in entries:
            s = int(e["stream"])
            for name in ("quality", "dt_us", "flow_x", "flow_y", "gyro_x", "gyro_y", "gyro_z"):
                assert e["record"][name].tobytes() == plain_want[k, s][name].tobytes(), ("plain", k, s, name)
            f = bytes(e["mavlink"][:int(e["mavlink_len"])])
            assert f == plain_wire[k][s] and f[5:7] == bytes([1, 100]), ("plain", k, s)
    pub, held, _ = ref.census(want)
    assert entries_seen == pub.sum() and pub[2] == run.active[:, 2].sum() and held[0] >= 10 and held[1] >= 10
    assert not any(w[3] for w in wire) and pub[3] >= 3, "stream 3 publishes entries without frames"
    assert ref.census(plain_want)[0].min() >= 3
    for f in singles + plain_singles:
        f.close()
    bank.close()
    plain.close()


def test_the_facade_takes_an_identity_set_between_ticks_from_that_tick(aof, synth, gpu_device):
    """OpticalFlowBank, S = 2, 64 x 64, rate 0 (every frame publishes), six ticks with every stream active and no setter
    before the first: setStreamIdentity(1, ...) before tick 2 is the first copy of the shadow records and their binding,
    the one before tick 4 a second copy of an array that is already bound.  Each applies from its own tick, to stream 1
    alone."""
    S, T, w = 2, 6, 64
    seqs = [synth.make_sequence(w, w, T, 4, seed=171000 + s, max_step=3)[0] for s in range(S)]
    bank = aof.OpticalFlowBank(FX, FY, 0, w, w, S)
    assert bank.engineOk(), bank.lastError()
    bank.setTimestampOffset(5_000_000)
    want = [(1, 100), (1, 100), (42, 43), (42, 43), (52, 53), (52, 53)]
    for k in range(T):
        if k == 2:
            assert bank.setStreamIdentity(1, 42, 43, 7) == 0
        if k == 4:
            assert bank.setStreamIdentity(1, 52, 53, 9) == 0
        n, entries = bank.push(np.stack([q[k] for q in seqs]), np.full(S, 12_000 * (k + 1), np.uint64))
        assert n == len(entries) == 2, (k, n, bank.lastError())
        assert list(entries["stream"]) == [0, 1], k
        ids = [tuple(bytes(e["mavlink"][5:7])) for e in entries]
        assert all(int(e["mavlink_len"]) > 0 for e in entries) and ids == [(1, 100), want[k]], (k, ids)
    bank.close()


def test_the_facade_with_imu_sends_with_each_stream_s_identity(aof, synth, gpu_device):
    """OpticalFlowBank with enableImu(), S = 3, 14 ticks: the IMU call packs the frames, with the identity and the
    sequence numbers setStreamIdentity() gave each stream; setStreamTimestampOffset() is ignored, as setTimestampOffset()
    is (every frame carries offset0 + t)."""
    import struct
    S, T, M, OFFSET0 = 3, 14, 2, 1_650_000_000_000_000
    run = ref.make_run(synth, 128, 128, S, T, 161, density=0.9, black=False)
    bank = aof.OpticalFlowBank(FX, FY, 0, 128, 128, S)               # (rate 0: every frame publishes)
    assert bank.engineOk(), bank.lastError()
    assert bank.enableImu(M, OFFSET0) == 0, bank.lastError()
    ids = [(11, 21, 250), (12, 22, 0), (13, 23, 100)]
    for s, (sysid, compid, seq) in enumerate(ids):
        assert bank.setStreamIdentity(s, sysid, compid, seq) == 0 and bank.setStreamTimestampOffset(s, 4242 + s) == 0
    clock, sent = 10 ** 9, [0] * S
    for k in range(T):
        for s in range(S):
            clock += 2500
            assert bank.pushImu(s, clock, 0.1, -0.2, 0.05) == 0
        n, entries = bank.push(run.frames[k], run.times[k], run.active[k], None)
        assert n == len(entries) >= 0, bank.lastError()
        for e in entries:
            s, ln = int(e["stream"]), int(e["mavlink_len"])
            f = bytes(e["mavlink"][:ln])
            assert ln > 0 and f[5:7] == bytes(ids[s][:2]) and f[4] == (ids[s][2] + sent[s]) & 0xFF, (k, s, f[:8])
            assert struct.unpack_from("<Q", f, 10)[0] == OFFSET0 + int(run.times[k, s]), (k, s)
            sent[s] += 1
    assert min(sent) >= 8, sent                                      # stream 0's sequence number has passed 255
    bank.close()
