"""The stream bank's MAVLink receive on the device (aof_bank_mavlink_rx_device / aof_bank_mavlink_rx_reset_device,
include/aof.h) and the facade's receive path (OpticalFlowBank::enableMavlinkRx / pushMavlink): samples up to their
counts, the counts and all 128 state bytes must equal aof_bank_mavlink_rx_host byte for byte, the public 32 bytes the
plain-Python model of tests/mavlink_rx_ref.py.  Sample buffers are pre-filled with the model's sentinel, so slots at
and behind a count are compared as well; every buffer has guard bytes behind it.  No tolerance anywhere."""
import numpy as np
import pytest

import mavlink_rx_ref as ref
import outbox_ref as ob
from bank_ref import FX, FY, make_run
from bank_rig import EINVAL, ENOBUFS, Guarded, engine, same, time_limit   # (engine, time_limit: this module's fixtures too)

pytestmark = pytest.mark.gpu



class Rx:
    """The buffers of receive calls of at most K rounds for S streams on the device, each with guard bytes."""

    def __init__(self, aof, eng, gpu_device, S, K, B, M):
        import torch
        self.aof, self.eng, self.torch, self.dev = aof, eng, torch, gpu_device
        self.S, self.K, self.B, self.M = S, K, B, M
        self.state_buf, self.counts_buf = Guarded(gpu_device, (S, 128)), Guarded(gpu_device, (K * S,))
        self.samples_buf = Guarded(gpu_device, (24 * K * M * S,), fill=ref.SENTINEL)
        self.state = self.state_buf.tensor
        eng.bank_mavlink_rx_reset(self.state)

    def run(self, data, lengths):
        """One call -> (samples [K, M, S], counts [K, S]) on the host; slots nobody wrote hold the sentinel."""
        torch, S, M = self.torch, self.S, self.M
        K = data.shape[0]
        self.samples_buf.refill(), self.counts_buf.refill()
        d = torch.from_numpy(np.ascontiguousarray(data)).to(self.dev)
        ln = None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths).view(np.int16)).to(self.dev)
        self.eng.bank_mavlink_rx(d, self.state, M, ln, self.samples_buf.tensor[:24 * K * M * S].view(K, M, S, 24),
                                 self.counts_buf.tensor[:K * S].view(K, S))
        torch.cuda.synchronize()
        self.state_buf.read()       # (the guard behind the states)
        return (self.samples_buf.read(24 * K * M * S).view(self.aof.IMU_SAMPLE_DTYPE).reshape(K, M, S),
                self.counts_buf.read(K * S).reshape(K, S))

    def states(self):
        return self.aof.mavlink_rx_states_view(self.state)


def host_run(aof, calls, M, S, states=None):
    """aof_bank_mavlink_rx_host over the calls -> ([(samples, counts)], states), sentinel-filled as Rx.run's."""
    states = np.zeros(S, aof.MAVLINK_RX_STATE_DTYPE) if states is None else states.copy()
    out = []
    for data, lengths in calls:
        K = data.shape[0]
        samples = np.full((K, M, S, 24), ref.SENTINEL, np.uint8).view(aof.IMU_SAMPLE_DTYPE).reshape(K, M, S)
        counts = np.zeros((K, S), np.uint8)
        aof.bank_mavlink_rx_host(data, lengths, states, M, samples, counts)
        out.append((samples, counts))
    return out, states


_families = {}


def family(aof, S, K, B, M, calls):
    """The coverage family of these sizes with what the host function and the model make of it: computed once."""
    key = (S, K, B, M, calls)
    if key not in _families:
        fam = ref.coverage_family(1000 * S + K, S, K, B, calls)
        want, states = host_run(aof, fam, M, S)
        parsers = [ref.Parser() for _ in range(S)]
        for data, lengths in fam:
            ref.run(data, lengths, M, parsers)
        _families[key] = dict(calls=fam, want=want, states=states, public=ref.publics(parsers))
    return _families[key]


def check_family(aof, engine, gpu_device, S, K, B, M, calls):
    f = family(aof, S, K, B, M, calls)
    rx = Rx(aof, engine, gpu_device, S, K, B, M)
    for c, (data, lengths) in enumerate(f["calls"]):
        samples, counts = rx.run(data, lengths)
        same(counts, f["want"][c][1], ("counts", c))
        same(samples, f["want"][c][0], ("samples up to the counts, the sentinel behind them", c))
    st = rx.states()
    same(st, f["states"], "all 128 state bytes against the host function")
    for n in ref.COUNTERS:
        assert np.array_equal(st[n], f["public"][n]), ("the public bytes against the model", n)
    return f, st


@pytest.mark.parametrize("K,B,M,calls", [(1, 16, 1, 24), (5, 272, 4, 2), (16, 4096, 16, 1)])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 257])
def test_the_device_equals_the_host_function_and_the_model_on_the_coverage_family(aof, engine, gpu_device, S, K, B, M, calls):
    f, st = check_family(aof, engine, gpu_device, S, K, B, M, calls)
    if S >= 63:
        lens = np.concatenate([l.ravel() for _, l in f["calls"]]).astype(np.int64)
        assert {min(e, B) for e in ref.edge_lengths(B)} <= set(np.minimum(lens, B)) and (lens > B).any(), "every staging edge"
        for n in ref.COUNTERS:
            assert st[n].sum() > 0, n
        assert st["in_progress"].any(axis=1).sum() > 0, "streams left inside a frame"


def test_null_lengths_mean_every_byte_of_the_slot(aof, engine, gpu_device):
    S, K, B, M = 65, 3, 272, 4
    calls = [(data, None) for data, _ in ref.coverage_family(8, S, K, B)]
    want, states = host_run(aof, calls, M, S)
    rx = Rx(aof, engine, gpu_device, S, K, B, M)
    samples, counts = rx.run(*calls[0])
    same(counts, want[0][1], "counts")
    same(samples, want[0][0], "samples")
    same(rx.states(), states, "states")
    assert (states["bytes"] == K * B).all()


def test_one_call_of_k_rounds_equals_k_calls_of_one(aof, engine, gpu_device):
    S, K, B, M = 65, 5, 272, 4
    f = family(aof, S, K, B, M, 2)
    (data, lengths), _ = f["calls"]
    rx = Rx(aof, engine, gpu_device, S, K, B, M)
    for k in range(K):
        samples, counts = rx.run(data[k:k + 1], lengths[k:k + 1])
        same(counts[0], f["want"][0][1][k], ("counts", k))
        same(samples[0], f["want"][0][0][k], ("samples", k))
    want_states = host_run(aof, f["calls"][:1], M, S)[1]
    same(rx.states(), want_states, "states behind K calls of one round")


def test_a_masked_reset_in_mid_frame_restarts_the_masked_streams_and_keeps_the_others(aof, engine, gpu_device):
    import torch
    S, K, B, M = 65, 5, 272, 4
    f = family(aof, S, K, B, M, 2)
    rx = Rx(aof, engine, gpu_device, S, K, B, M)
    rx.run(*f["calls"][0])
    before = rx.states().copy()
    mid = before["in_progress"].any(axis=1)
    assert mid.sum() >= 8, "the family leaves streams inside a frame"
    mask = np.zeros(S, np.uint8)
    mask[np.flatnonzero(mid)[::2]] = 1          # every other stream that is inside a frame
    mask[np.flatnonzero(~mid)[:3]] = 1
    engine.bank_mavlink_rx_reset(rx.state, torch.from_numpy(mask).to(gpu_device))
    torch.cuda.synchronize()
    after = rx.states().copy()
    assert not after[mask == 1].view(np.uint8).any(), "a reset stream is idle with every counter 0"
    same(after[mask == 0], before[mask == 0], "the others")
    rx.state_buf.read()         # (the guard behind the states)
    want, states = host_run(aof, f["calls"][1:], M, S, after)
    samples, counts = rx.run(*f["calls"][1])
    same(counts, want[0][1], "counts behind the reset")
    same(samples, want[0][0], "samples behind the reset")
    same(rx.states(), states, "states behind the reset")


def test_refused_calls_write_nothing(aof, engine, gpu_device):
    import ctypes as C
    import torch
    S, K, B, M = 63, 5, 272, 4
    f = family(aof, S, K, B, M, 2)
    rx = Rx(aof, engine, gpu_device, S, K, B, M)
    data = torch.from_numpy(f["calls"][0][0]).to(gpu_device)
    lens = torch.from_numpy(f["calls"][0][1].view(np.int16)).to(gpu_device)
    samples = torch.full((K, M, S, 24), 0xEE, dtype=torch.uint8, device=gpu_device)
    counts = torch.full((K, S), 0xEE, dtype=torch.uint8, device=gpu_device)
    stream = torch.cuda.current_stream().cuda_stream
    call, reset = aof.lib.aof_bank_mavlink_rx_device, aof.lib.aof_bank_mavlink_rx_reset_device

    def args(**kw):
        rp = aof.mavlink_rx_params(kw.get("S", S), kw.get("K", K), kw.get("B", B), kw.get("M", M))
        return [kw.get("ctx", engine._ctx), None if kw.get("rp", 1) is None else C.byref(rp), kw.get("data", data.data_ptr()),
                kw.get("lens", lens.data_ptr()), kw.get("state", rx.state.data_ptr()), kw.get("samples", samples.data_ptr()),
                kw.get("counts", counts.data_ptr()), stream]

    refused = [dict(ctx=None), dict(rp=None), dict(data=None), dict(state=None), dict(samples=None), dict(counts=None),
               dict(S=0), dict(S=-1), dict(K=0), dict(K=17), dict(B=0), dict(B=8), dict(B=264), dict(B=4112), dict(M=0), dict(M=17),
               dict(data=data.data_ptr() + 8), dict(state=rx.state.data_ptr() + 4), dict(samples=samples.data_ptr() + 4),
               dict(lens=lens.data_ptr() + 1)]
    for kw in refused:
        assert call(*args(**kw)) == EINVAL, kw
    assert b"mavlink rx" in aof.lib.aof_last_error(engine._ctx)
    assert reset(None, S, None, rx.state.data_ptr(), stream) == EINVAL
    assert reset(engine._ctx, 0, None, rx.state.data_ptr(), stream) == EINVAL
    assert reset(engine._ctx, S, None, None, stream) == EINVAL
    assert reset(engine._ctx, S, None, rx.state.data_ptr() + 4, stream) == EINVAL
    torch.cuda.synchronize()
    assert not rx.states().view(np.uint8).any(), "a refused call must leave the states untouched"
    for t in (samples, counts):
        assert (t.cpu().numpy() == 0xEE).all(), "a refused call must write nothing"
    assert call(*args()) == 0, "the context is still usable"
    torch.cuda.synchronize()
    same(counts.cpu().numpy(), f["want"][0][1], "counts")


# ---- in front of real pushes -----------------------------------------------------------------------------------------

S_REAL, T_REAL, K_REAL, M_REAL, B_REAL = 5, 8, 5, 4, 272
FIRST_SEQ = 253


class Wire:
    """What S autopilots send: per stream a byte stream of HIGHRES_IMU frames at about 400 Hz in all their forms, with
    other frames and junk between them, handed out in reads of any length (a read ends wherever it ends)."""

    def __init__(self, seed, S):
        self.rng, self.S = np.random.default_rng(seed), S
        self.clock = np.full(S, 10 ** 9, np.int64)
        self.pending = [b""] * S
        self.i = 0

    def round(self, B):
        """(data uint8 [S, B], lengths uint16 [S]) of one round."""
        rng = self.rng
        data = rng.integers(0, 256, (self.S, B), dtype=np.uint8)        # (behind the length: garbage)
        lengths = np.zeros(self.S, np.uint16)
        for s in range(self.S):
            buf = self.pending[s]
            for _ in range(int(rng.integers(0, 4))):
                self.i += 1
                self.clock[s] += int(rng.integers(2000, 3000)) if rng.random() < 0.95 else 60000
                p = ref.imu_payload(int(self.clock[s]), *(float(v) for v in rng.normal(0, 0.8, 3).astype(np.float32)), rest=9.81)
                form = self.i % 4
                buf += (ref.frame_v1(105, p, seq=self.i & 255) if form == 0 else
                        ref.frame_v2(105, p, seq=self.i & 255, signature=bytes(13)) if form == 1 else
                        ref.frame_v2(105, p, seq=self.i & 255))
                if rng.random() < 0.5:
                    buf += ref.frame_v2(30, rng.integers(0, 256, 28, dtype=np.uint8).tobytes(), seq=self.i & 255)
                if rng.random() < 0.2:
                    buf += ref.junk(rng, int(rng.integers(1, 9)))
            n = min(len(buf), B) if rng.random() < 0.5 else int(rng.integers(0, min(len(buf), B) + 1))
            data[s, :n] = np.frombuffer(buf[:n], np.uint8)
            lengths[s] = n
            self.pending[s] = buf[n:]
        return data, lengths


@pytest.fixture(scope="module")
def real_run(synth):
    return make_run(synth, 64, 64, S_REAL, T_REAL + K_REAL, 21, density=0.9, black=False)


def test_receive_push_imu_collect_equals_the_models_samples_fed_to_the_imu_call(aof, gpu_device, real_run):
    """64x64, S = 5: 8 ticks, then one K = 5 burst.  Chain A: receive -> records-only push -> IMU call -> collect.  Chain B,
    on a twin bank: the samples the model decodes from the same bytes, uploaded, -> the same push -> IMU call -> collect.
    The two outboxes must hold the same bytes."""
    import torch
    run, S, M, B = real_run, S_REAL, M_REAL, B_REAL
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    banks = [eng.bank_create(aof.bank_params(S, FX, FY, 15, 0, 1, 100, 0), gpu_device) for _ in range(2)]
    imu_states = [torch.zeros((S, 64), dtype=torch.uint8, device=gpu_device) for _ in range(2)]
    for st in imu_states:
        eng.bank_imu_reset(st, offset0=1_700_000_000_000_000)
    rx_state = torch.zeros((S, 128), dtype=torch.uint8, device=gpu_device)
    eng.bank_mavlink_rx_reset(rx_state)
    parsers = [ref.Parser() for _ in range(S)]
    wire = Wire(7, S)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    sent = delivered = 0

    def step(K, frames, times, select, burst, tag):
        nonlocal sent, delivered
        rounds = [wire.round(B) for _ in range(K)]
        data, lengths = np.stack([r[0] for r in rounds]), np.stack([r[1] for r in rounds])
        m_samples, m_counts = ref.run(data, lengths, M, parsers)
        delivered += int(m_counts.sum())
        boxes = []
        for chain in range(2):
            if chain == 0:
                samples, counts = eng.bank_mavlink_rx(up(data), rx_state, M, up(lengths.view(np.int16)))
            else:
                samples, counts = up(m_samples.view(np.uint8).reshape(K, M, S, 24)), up(m_counts)
            if burst:
                records = eng.bank_push_burst(banks[chain], K, up(frames), up(times), up(select), None)
            else:
                records = eng.bank_push(banks[chain], up(frames[0]), up(times[0]), up(select), None).view(1, S, 48)
            _, frames_out, lens = eng.bank_imu(samples, up(times), records, imu_states[chain], counts, records_out=records,
                                               first_seq=FIRST_SEQ)
            box = torch.full((aof.outbox_layout(K * S, 0).total_bytes,), ob.FILL, dtype=torch.uint8, device=gpu_device)
            eng.bank_collect(records, frames_out, lens, capacity_messages=K * S, outbox=box, tag=tag)
            torch.cuda.synchronize()
            boxes.append(box.cpu().numpy())
        assert boxes[0].tobytes() == boxes[1].tobytes(), ("the outbox", "burst" if burst else "tick", tag)
        assert imu_states[0].cpu().numpy().tobytes() == imu_states[1].cpu().numpy().tobytes()
        sent += int(aof.outbox_view(boxes[0], K * S)[0]["n_messages"])

    for k in range(T_REAL):
        step(1, run.frames[k:k + 1], run.times[k:k + 1], run.active[k], False, 100 + k)
    rounds = slice(T_REAL, T_REAL + K_REAL)
    count = run.active[rounds].cumprod(axis=0).sum(axis=0).astype(np.uint8)
    step(K_REAL, run.frames[rounds], run.times[rounds], count, True, 200)
    st = aof.mavlink_rx_states_view(rx_state)
    pub = ref.publics(parsers)
    for n in ref.COUNTERS:
        assert np.array_equal(st[n], pub[n]), n
    assert sent >= S and delivered >= 4 * S and st["frames"].sum() > st["imu_samples"].sum() and st["skipped"].sum() > 0, (sent, delivered)
    eng.close()


def test_a_captured_receive_push_imu_collect_chain_replayed_twice_equals_eager_execution(aof, gpu_device, real_run):
    """One linear graph on one stream (no parallel branches): receive -> records-only push -> IMU call -> collect with
    d_tag; fresh frames and bytes are copied into the same tensors between the replays."""
    import torch
    run, S, M, B = real_run, S_REAL, M_REAL, B_REAL
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    bp = aof.bank_params(S, FX, FY, 0, 0, 1, 100, 0)               # rate 0: every frame publishes
    wire = Wire(9, S)
    ticks = [wire.round(B) for _ in range(3)]
    total = aof.outbox_layout(S, 0).total_bytes

    class Chain:
        def __init__(self):
            z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=gpu_device)
            self.bank = eng.bank_create(bp, gpu_device)
            self.frames, self.times = z(S, 64, 64), torch.zeros(S, dtype=torch.int64, device=gpu_device)
            self.data, self.lengths = z(S, B), torch.zeros(S, dtype=torch.int16, device=gpu_device)
            self.samples, self.counts = z(M, S, 24), z(S)
            self.records, self.wire, self.lens = z(S, 48), z(S, 56), z(S)
            self.state, self.rx_state, self.box = z(S, 64), z(S, 128), z(total)
            self.tag = torch.zeros(1, dtype=torch.int64, device=gpu_device)
            self.start()

        def start(self):
            eng.bank_reset(self.bank)
            eng.bank_imu_reset(self.state, offset0=123456)
            eng.bank_mavlink_rx_reset(self.rx_state)

        def load(self, k):
            self.frames.copy_(torch.from_numpy(run.frames[k]))
            self.times.copy_(torch.from_numpy(run.times[k]))
            self.data.copy_(torch.from_numpy(ticks[k][0]))
            self.lengths.copy_(torch.from_numpy(ticks[k][1].view(np.int16)))
            self.tag.fill_(700 + k)
            self.box.fill_(ob.FILL)

        def enqueue(self):
            eng.bank_mavlink_rx(self.data, self.rx_state, M, self.lengths, self.samples, self.counts)
            eng.bank_push(self.bank, self.frames, self.times, None, None, records=self.records)
            eng.bank_imu(self.samples, self.times, self.records, self.state, self.counts, records_out=self.records,
                         out_frames=self.wire, out_lengths=self.lens, first_seq=FIRST_SEQ)
            eng.bank_collect(self.records, self.wire, self.lens, capacity_messages=S, outbox=self.box, tag=0, tag_tensor=self.tag)

        def read(self):
            torch.cuda.synchronize()
            return [t.cpu().numpy().tobytes() for t in (self.box, self.state, self.rx_state, self.counts)]

    eager = Chain()
    outs = []
    for k in range(3):
        eager.load(k)
        eager.enqueue()
        outs.append(eager.read())
    assert sum(int(aof.outbox_view(np.frombuffer(o[0], np.uint8), S)[0]["n_messages"]) for o in outs) >= S
    assert sum(np.frombuffer(o[3], np.uint8).sum() for o in outs) >= S, "samples were delivered"
    c = Chain()
    c.load(0)
    c.enqueue()                                       # (every kernel has run once before the capture)
    c.read()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.enqueue()
    c.start()
    for k in range(3):
        c.load(k)
        g.replay()
        got = c.read()
        for name, a, b in zip(("outbox", "imu states", "receive states", "counts"), got, outs[k]):
            assert a == b, ("replayed", name, k)
    eng.close()


# ---- the facade --------------------------------------------------------------------------------------------------------

def test_the_facade_fed_bytes_equals_a_twin_fed_the_decoded_samples(aof, synth, gpu_device):
    """OpticalFlowBank with enableMavlinkRx over 3 streams and 16 ticks, fed pushMavlink in reads of any length, against
    a twin object with enableImu only, fed pushImu with what the model decodes from each tick's bytes."""
    S, T, M, B = 3, 16, 4, 272
    OFFSET0 = 1_650_000_000_000_000
    run = make_run(synth, 128, 128, S, T, 14, density=0.85, black=False)
    bank, twin = (aof.OpticalFlowBank(FX, FY, 15, 128, 128, S) for _ in range(2))
    assert bank.engineOk() and twin.engineOk()
    assert bank.enableMavlinkRx(B) == EINVAL and "enableImu" in bank.lastError() and bank.engineOk(), "no enableImu yet"
    assert bank.pushMavlink(0, b"\x00") == EINVAL
    assert bank.enableImu(M, OFFSET0) == 0 and twin.enableImu(M, OFFSET0) == 0
    for bad in (0, 8, 264, 4112):
        assert bank.enableMavlinkRx(bad) == EINVAL and bank.engineOk(), bad
    assert bank.enableMavlinkRx(B) == 0, bank.lastError()
    assert bank.enableMavlinkRx(B) == EINVAL and "already" in bank.lastError() and bank.engineOk()
    assert bank.pushImu(0, 1, 0.0, 0.0, 0.0) == EINVAL, "with the receive path the device counts the samples"
    assert bank.pushMavlink(-1, b"\x00") == EINVAL and bank.pushMavlink(S, b"\x00") == EINVAL
    wire = Wire(3, S)
    parsers = [ref.Parser() for _ in range(S)]
    sent = samples_fed = 0
    for k in range(T):
        data, lengths = wire.round(B)
        for s in range(S):
            n = int(lengths[s])
            cut = n // 3                                            # two reads per tick
            assert bank.pushMavlink(s, data[s, :cut].tobytes()) == 0 and bank.pushMavlink(s, data[s, cut:n].tobytes()) == 0
            if k == 2 and s == 1:                                   # a full slot refuses and takes nothing
                assert bank.pushMavlink(s, bytes(B - n + 1)) == ENOBUFS and bank.engineOk()
                assert bank.pushMavlink(s, b"") == 0
            out = []
            parsers[s].feed(data[s, :n].tobytes(), M, out)
            for t, x, y, z in out:
                fx, fy, fz = np.array([x, y, z], np.uint32).view(np.float32)
                assert twin.pushImu(s, t, fx, fy, fz) == 0
            samples_fed += len(out)
        n1, e1 = bank.push(run.frames[k], run.times[k], run.active[k], None)
        n2, e2 = twin.push(run.frames[k], run.times[k], run.active[k], None)
        assert n1 == n2 >= 0, (k, n1, n2, bank.lastError(), twin.lastError())
        assert e1.tobytes() == e2.tobytes(), ("the published entries", k)
        sent += n1
    assert sent >= S and samples_fed >= 4 * S, (sent, samples_fed)
    # a reset drops a half-received frame and the queued bytes: the rest of the frame is junk to the restarted stream
    frame = ref.frame_v2(105, ref.imu_payload(int(wire.clock[0]) + 2500, 0.1, 0.1, 0.1))
    for s in range(S):
        assert bank.pushMavlink(s, wire.pending[s] + frame[:20]) in (0, ENOBUFS)
    assert bank.reset(None) == 0 and twin.reset(None) == 0
    t0 = np.full(S, 1_000_000, np.int64)
    later = ref.frame_v2(105, ref.imu_payload(int(wire.clock[0]) + 5000, 0.2, 0.2, 0.2))
    fresh = [(frame[20:] + frame, int(wire.clock[0]) + 2500, 0.1), (later, int(wire.clock[0]) + 5000, 0.2)]
    assert len(ref.decode(fresh[0][0])) == 1, "the tail of the dropped frame starts no frame of its own"
    for k, (data, t, v) in enumerate(fresh):
        for s in range(S):
            assert bank.pushMavlink(s, data) == 0 and twin.pushImu(s, t, v, v, v) == 0
        n1, e1 = bank.push(run.frames[k], t0 + 100000 * k, None, None)
        n2, e2 = twin.push(run.frames[k], t0 + 100000 * k, None, None)
        assert n1 == n2 and e1.tobytes() == e2.tobytes(), k
    assert n1 == S, "published again behind the reset, with a fresh sample: sent"
    bank.close()
    twin.close()
