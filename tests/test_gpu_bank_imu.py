"""The stream bank's IMU on the device (aof_bank_imu_device / aof_bank_imu_reset_device, include/aof.h) and the facade's
IMU form (OpticalFlowBank::enableImu / pushImu): records, frames up to their lengths, lengths and the whole 64-byte
states must equal, byte for byte, the plain-Python model of tests/imu_ref.py -- on synthetic records (no flow engine:
the coverage family and random families at the wave and workgroup edges) and behind real pushes on every bank path.
Frame buffers are pre-filled with the model's sentinel, so bytes behind a frame's length are compared as well; every
buffer has guard bytes behind it.  No tolerance anywhere."""
import numpy as np
import pytest

import imu_ref as ref
import outbox_ref as ob
from bank_ref import FX, FY, make_run
from bank_rig import EINVAL, ENOBUFS, Guarded, engine, time_limit   # (engine, time_limit: this module's fixtures too)
from bank_rig import same as same_bytes

pytestmark = pytest.mark.gpu


def same(got, want, what):
    for name in ("records", "lengths", "frames", "states"):
        if got.get(name) is not None and want.get(name) is not None:
            same_bytes(got[name], want[name], (what, name))


def model(f, k0=0, k1=None, states=None, pack=True):
    k1 = f["samples"].shape[0] if k1 is None else k1
    return ref.run(f["samples"][k0:k1], None if f["counts"] is None else f["counts"][k0:k1], f["times"][k0:k1],
                   f["records"][k0:k1], f["states"] if states is None else states, first_seq=f["first_seq"], pack=pack)


class Imu:
    """The buffers of one IMU call for [K][M][S] samples on the device, each with guard bytes; the states are written
    directly (their layout is public)."""

    def __init__(self, aof, eng, gpu_device, f):
        import torch
        self.aof, self.eng, self.torch, self.dev, self.f = aof, eng, torch, gpu_device, f
        self.K, self.M, self.S = f["samples"].shape
        K, M, S = self.K, self.M, self.S
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(gpu_device)
        self.samples = up(f["samples"]).view(K, M, S, 24)
        self.counts = None if f["counts"] is None else up(f["counts"]).view(K, S)
        self.times = torch.from_numpy(np.ascontiguousarray(f["times"]).view(np.int64)).to(gpu_device)
        self.records_in = up(f["records"]).view(K, S, 48)
        self.state_buf, self.out_buf = Guarded(gpu_device, (S, 64)), Guarded(gpu_device, (48 * K * S,))
        self.wire_buf, self.lens_buf = Guarded(gpu_device, (56 * K * S,), fill=ref.SENTINEL), Guarded(gpu_device, (K * S,))
        self.state = self.state_buf.tensor
        self.set_states(f["states"])

    def set_states(self, states):
        self.state.copy_(self.torch.from_numpy(np.ascontiguousarray(states).view(np.uint8).reshape(self.S, 64)))

    def run(self, k0=0, k1=None, in_place=False, mavlink=True):
        """Rounds k0 .. k1-1 in one call -> dict(records, frames, lengths, states) on the host."""
        k1 = self.K if k1 is None else k1
        n, S = k1 - k0, self.S
        for b in (self.out_buf, self.wire_buf, self.lens_buf):
            b.refill()
        out = self.out_buf.tensor[:48 * n * S].view(n, S, 48)
        wire = self.wire_buf.tensor[:56 * n * S].view(n, S, 56)
        lens = self.lens_buf.tensor[:n * S].view(n, S)
        rin = self.records_in[k0:k1]
        if in_place:
            out.copy_(rin)
            rin = out
        self.eng.bank_imu(self.samples[k0:k1], self.times[k0:k1], rin, self.state, None if self.counts is None else self.counts[k0:k1],
                          mavlink=mavlink, records_out=out, out_frames=wire if mavlink else None,
                          out_lengths=lens if mavlink else None, first_seq=self.f["first_seq"])
        self.torch.cuda.synchronize()
        got = dict(records=self.out_buf.read(48 * n * S).view(self.aof.TICK_DTYPE).reshape(n, S),
                   states=self.state_buf.read().reshape(-1).view(self.aof.IMU_STATE_DTYPE))
        if mavlink:
            got.update(frames=self.wire_buf.read(56 * n * S).reshape(n, S, 56), lengths=self.lens_buf.read(n * S).reshape(n, S))
        else:       # without d_mavlink no frame byte and no length is written
            self.wire_buf.read(0), self.lens_buf.read(0)
        return got


_families = {}


def cached(key, make):
    if key not in _families:
        f = make()
        f["want"] = model(f)
        _families[key] = f
    return _families[key]


# ---- synthetic records, no flow engine ----

def test_the_device_equals_the_model_on_the_coverage_family(aof, engine, gpu_device):
    f = cached("family", ref.family)
    assert all(f["want"]["tally"][o] >= 1 for o in ref.OUTCOMES)
    imu = Imu(aof, engine, gpu_device, f)
    same(imu.run(), f["want"], "out of place")
    imu.set_states(f["states"])
    same(imu.run(in_place=True), f["want"], "in place")
    imu.set_states(f["states"])
    same(imu.run(mavlink=False), f["want"], "without frames: the same decisions and counters")
    same(dict(zip(("records", "frames", "lengths"), aof.bank_imu_host(f["samples"], f["counts"], f["times"], f["records"],
                                                                        f["states"].copy(), first_seq=f["first_seq"], fill=ref.SENTINEL))),
         f["want"], "the host function")


@pytest.mark.parametrize("K,M", [(1, 1), (5, 4), (16, 16)])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 257])
def test_the_device_equals_the_model_on_random_families(aof, engine, gpu_device, S, K, M):
    """A lone lane, the wave edge, two workgroups with a ragged last one; mixed counts (0 .. M and above); one call of K
    rounds against K calls of one round on a twin state; in place against out of place."""
    f = cached((S, K, M), lambda: ref.random_family(seed=1000 * S + 16 * K + M, S=S, K=K, M=M))
    imu = Imu(aof, engine, gpu_device, f)
    got = imu.run()
    same(got, f["want"], "one call")
    imu.set_states(f["states"])
    same(imu.run(in_place=True), got, "in place")
    if K > 1:
        imu.set_states(f["states"])
        parts = [imu.run(k, k + 1) for k in range(K)]
        twin = dict(records=np.concatenate([p["records"] for p in parts]), frames=np.concatenate([p["frames"] for p in parts]),
                    lengths=np.concatenate([p["lengths"] for p in parts]), states=parts[-1]["states"])
        same(twin, got, "K calls of one round")


def test_a_null_count_means_every_slot(aof, engine, gpu_device):
    f = cached("full", lambda: ref.random_family(seed=77, S=65, K=5, M=4, counts="full"))
    assert f["counts"] is None
    same(Imu(aof, engine, gpu_device, f).run(), f["want"], "counts NULL")


def test_a_masked_reset_restarts_the_masked_streams_and_keeps_the_others(aof, engine, gpu_device):
    import torch
    f = cached((257, 5, 4), lambda: ref.random_family(seed=1000 * 257 + 16 * 5 + 4, S=257, K=5, M=4))
    imu = Imu(aof, engine, gpu_device, f)
    engine.bank_imu_reset(imu.state, offset0=0)
    fresh = np.zeros(257, ref.STATE_DTYPE)
    torch.cuda.synchronize()
    assert aof.imu_states_view(imu.state).tobytes() == fresh.tobytes(), "reset of all streams, offset learned later"
    imu.set_states(f["states"])
    got = imu.run()
    same(got, f["want"], "before the reset")
    mask = (np.arange(257) % 3 == 1).astype(np.uint8)
    engine.bank_imu_reset(imu.state, torch.from_numpy(mask).to(gpu_device), offset0=(1 << 45) + 5)
    want = f["want"]["states"].copy()
    fresh["offset_timestamp_usec"] = (1 << 45) + 5
    want[mask == 1] = fresh[mask == 1]
    assert (f["want"]["states"]["samples_integrated"][mask == 1] > 0).any()
    torch.cuda.synchronize()
    assert imu.state_buf.read().tobytes() == want.tobytes(), "masked reset"
    # the streams go on from there
    same(imu.run(), model(f, states=want), "behind the reset")


def test_refused_calls_write_nothing(aof, engine, gpu_device):
    import ctypes as C
    import torch
    f = cached((63, 5, 4), lambda: ref.random_family(seed=1000 * 63 + 16 * 5 + 4, S=63, K=5, M=4))
    imu = Imu(aof, engine, gpu_device, f)
    out = torch.full((5, 63, 48), 0xEE, dtype=torch.uint8, device=gpu_device)
    wire = torch.full((5, 63, 56), 0xEE, dtype=torch.uint8, device=gpu_device)
    lens = torch.full((5, 63), 0xEE, dtype=torch.uint8, device=gpu_device)
    stream = torch.cuda.current_stream().cuda_stream
    call, reset = aof.lib.aof_bank_imu_device, aof.lib.aof_bank_imu_reset_device

    def args(**kw):
        ip = aof.imu_params(kw.get("S", 63), kw.get("K", 5), kw.get("M", 4))
        return [kw.get("ctx", engine._ctx), None if kw.get("ip", 1) is None else C.byref(ip), kw.get("samples", imu.samples.data_ptr()),
                imu.counts.data_ptr(), kw.get("times", imu.times.data_ptr()), kw.get("rin", imu.records_in.data_ptr()),
                kw.get("state", imu.state.data_ptr()), kw.get("out", out.data_ptr()), kw.get("wire", wire.data_ptr()),
                kw.get("lens", lens.data_ptr()), stream]

    refused = [dict(ctx=None), dict(ip=None), dict(samples=None), dict(times=None), dict(rin=None), dict(state=None), dict(out=None),
               dict(S=0), dict(K=0), dict(K=17), dict(M=0), dict(M=17), dict(wire=None), dict(lens=None),
               dict(samples=imu.samples.data_ptr() + 4), dict(state=imu.state.data_ptr() + 4), dict(times=imu.times.data_ptr() + 4),
               dict(rin=imu.records_in.data_ptr() + 2), dict(out=out.data_ptr() + 2)]
    for kw in refused:
        assert call(*args(**kw)) == EINVAL, kw
    assert b"imu" in aof.lib.aof_last_error(engine._ctx)
    assert reset(None, 63, None, 0, imu.state.data_ptr(), stream) == EINVAL
    assert reset(engine._ctx, 0, None, 0, imu.state.data_ptr(), stream) == EINVAL
    assert reset(engine._ctx, 63, None, 0, None, stream) == EINVAL
    assert reset(engine._ctx, 63, None, 0, imu.state.data_ptr() + 4, stream) == EINVAL
    torch.cuda.synchronize()
    assert aof.imu_states_view(imu.state).tobytes() == f["states"].tobytes(), "a refused call must leave the states untouched"
    for t in (out, wire, lens):
        assert (t.cpu().numpy() == 0xEE).all(), "a refused call must write nothing"
    # the context is still usable
    assert call(*args()) == 0
    torch.cuda.synchronize()
    same(dict(states=aof.imu_states_view(imu.state), records=out.cpu().numpy().view(aof.TICK_DTYPE).reshape(5, 63)), f["want"], "after")


# ---- behind real pushes ----

S_REAL, T_REAL, K_REAL, M_REAL = 5, 12, 5, 4
FIRST_SEQ = 253
FLOW_FIELDS = ("dt_us", "flow_x", "flow_y", "frame", "pixel")


def real_samples(rng, K, S, clock):
    """[K, M, S] samples, 0 .. M per round at about 400 Hz with a few gaps; stream 0 hears nothing in round 1 (a stale
    take if it publishes there).  clock [S] runs on across calls."""
    a = np.zeros((K, M_REAL, S), ref.SAMPLE_DTYPE)
    a["time_usec"] = ref.GARBAGE[0]
    counts = rng.integers(0, M_REAL + 1, (K, S)).astype(np.uint8)
    if K > 1:
        counts[1, 0] = 0
    for k in range(K):
        for s in range(S):
            for j in range(counts[k, s]):
                clock[s] += int(rng.integers(2000, 3000)) if rng.random() < 0.95 else 60000
                a[k, j, s] = (clock[s], *rng.normal(0, 0.8, 3).astype(np.float32), 0)
    return a, counts


@pytest.fixture(scope="module")
def real_run(synth):
    return make_run(synth, 64, 64, S_REAL, T_REAL + K_REAL, 21, density=0.9, black=False)


def check_flow_fields(got, with_gyro, what):
    """The IMU call's records against those of the existing push with d_gyro: only gyro and quality codes differ."""
    for n in FLOW_FIELDS:
        assert got[n].tobytes() == with_gyro[n].tobytes(), (what, n)
    dropped = (got["quality"] == ref.STALE_GYRO) | (got["quality"] == ref.NO_OFFSET)
    assert (got["quality"][~dropped] == with_gyro["quality"][~dropped]).all() and (with_gyro["quality"][dropped] >= 0).all(), what


@pytest.mark.parametrize("path", [1, 2])
def test_ticks_and_a_burst_behind_the_records_only_push_equal_the_model_on_that_pushs_records(aof, gpu_device, real_run, path):
    """64x64, S = 5: 12 ticks, then one K = 5 burst, on one bank and one IMU state; the model is applied to the records
    the push itself wrote.  A twin bank pushed with d_gyro and frames gives the flow fields."""
    import torch
    run, S = real_run, S_REAL
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    eng.set_bank_path(path)
    bank = eng.bank_create(aof.bank_params(S, FX, FY, 15, 0, 1, 100, 0), gpu_device)
    twin = eng.bank_create(aof.bank_params(S, FX, FY, 15, ob.OFFSET, 1, 100, 0), gpu_device)
    rng = np.random.default_rng(5)
    clock = np.full(S, 10 ** 9, np.int64)
    states = np.zeros(S, ref.STATE_DTYPE)
    states["offset_timestamp_usec"][1::2] = 1_700_000_000_000_000          # every other stream learns its offset
    state = torch.from_numpy(states.view(np.uint8).reshape(S, 64).copy()).to(gpu_device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    tally = {}

    def step(K, frames, times, select, gyro, burst):
        nonlocal states
        samples, counts = real_samples(rng, K, S, clock)
        d_samples = up(samples.view(np.uint8).reshape(K, M_REAL, S, 24))
        if burst:
            records = eng.bank_push_burst(bank, K, up(frames), up(times), up(select), None)
            r2, _, _ = eng.bank_push_burst(twin, K, up(frames), up(times), up(select), up(gyro), mavlink=True)
        else:
            records = eng.bank_push(bank, up(frames[0]), up(times[0]), up(select), None).view(1, S, 48)
            r2, _, _ = eng.bank_push(twin, up(frames[0]), up(times[0]), up(select), up(gyro[0]), mavlink=True)
        wire = torch.full((K, S, 56), ref.SENTINEL, dtype=torch.uint8, device=gpu_device)
        lens = torch.full((K, S), 0xEE, dtype=torch.uint8, device=gpu_device)
        raw = records.clone()
        eng.bank_imu(d_samples, up(times), records, state, up(counts), records_out=records, out_frames=wire, out_lengths=lens,
                     first_seq=FIRST_SEQ)
        torch.cuda.synchronize()
        pushed = raw.cpu().numpy().view(aof.TICK_DTYPE).reshape(K, S)
        assert not pushed["gyro_x"].any() and not pushed["gyro_z"].any(), "a push without d_gyro leaves zero sums"
        want = ref.run(samples, counts, times.astype(np.uint64), pushed, states, first_seq=FIRST_SEQ)
        got = dict(records=records.cpu().numpy().view(aof.TICK_DTYPE).reshape(K, S), frames=wire.cpu().numpy(),
                   lengths=lens.cpu().numpy(), states=aof.imu_states_view(state))
        same(got, want, ("burst" if burst else "tick"))
        check_flow_fields(got["records"], r2.cpu().numpy().view(aof.TICK_DTYPE).reshape(K, S), burst)
        states = want["states"]
        for name, n in want["tally"].items():
            tally[name] = tally.get(name, 0) + n

    for k in range(T_REAL):
        step(1, run.frames[k:k + 1], run.times[k:k + 1], run.active[k], run.gyro[k:k + 1], False)
    rounds = slice(T_REAL, T_REAL + K_REAL)
    count = run.active[rounds].cumprod(axis=0).sum(axis=0).astype(np.uint8)       # frames in rounds 0 .. count-1
    step(K_REAL, run.frames[rounds], run.times[rounds], count, run.gyro[rounds], True)
    assert tally["sent"] >= S and tally["held"] >= S and tally["accepted"] > 50 and tally["offset_learned"] >= 2, tally
    eng.close()


def test_a_camera_push_then_the_imu_call(aof, gpu_device, real_run):
    """The sensor-frame push for records only, the IMU call behind it: the model on that push's records."""
    import torch
    run, S, cw, ch = real_run, S_REAL, 96, 80
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    cam = aof.bank_camera_params(cw, ch, 64, 64, 0, 200000)
    bank = eng.bank_create(aof.bank_params(S, FX, FY, 15, 0, 1, 100, 0), gpu_device, camera=cam)
    twin = eng.bank_create(aof.bank_params(S, FX, FY, 15, ob.OFFSET, 1, 100, 0), gpu_device, camera=cam)
    rng = np.random.default_rng(6)
    clock = np.full(S, 10 ** 9, np.int64)
    states = np.zeros(S, ref.STATE_DTYPE)
    states["offset_timestamp_usec"] = 99
    state = torch.from_numpy(states.view(np.uint8).reshape(S, 64).copy()).to(gpu_device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    x0, y0 = cw // 2 - 32, ch // 2 - 32
    sent = 0
    for k in range(6):
        sensor = rng.integers(0, 256, (S, ch, cw), dtype=np.uint8)
        sensor[:, y0:y0 + 64, x0:x0 + 64] = run.frames[k]
        samples, counts = real_samples(rng, 1, S, clock)
        out = eng.bank_push_camera(bank, up(sensor), up(run.times[k]), up(run.active[k]), None)
        out2 = eng.bank_push_camera(twin, up(sensor), up(run.times[k]), up(run.active[k]), up(run.gyro[k]), mavlink=True)
        records = out["records"]
        raw = records.clone()
        _, wire, lens = eng.bank_imu(up(samples.view(np.uint8).reshape(M_REAL, S, 24)), up(run.times[k]), records, state, up(counts[0]),
                                     records_out=records, first_seq=FIRST_SEQ)
        torch.cuda.synchronize()
        pushed = raw.cpu().numpy().view(aof.TICK_DTYPE).reshape(1, S)
        want = ref.run(samples, counts, run.times[k:k + 1].astype(np.uint64), pushed, states, first_seq=FIRST_SEQ)
        got = dict(records=aof.ticks_view(records).reshape(1, S), lengths=lens.cpu().numpy().reshape(1, S), states=aof.imu_states_view(state))
        same(got, want, ("camera tick", k))
        w = wire.cpu().numpy().reshape(1, S, 56)
        for s in range(S):
            n = int(want["lengths"][0, s])
            assert w[0, s, :n].tobytes() == want["frames"][0, s, :n].tobytes(), (k, s)
        check_flow_fields(got["records"], aof.ticks_view(out2["records"]).reshape(1, S), k)
        states = want["states"]
        sent += int((want["lengths"] > 0).sum())
    assert sent >= S
    eng.close()


# ---- the outbox behind the IMU call ----

def test_collect_behind_the_imu_call_lists_only_what_is_sent_and_is_polled_from_pinned_memory(aof, engine, gpu_device):
    import torch
    f = cached("family", ref.family)
    imu = Imu(aof, engine, gpu_device, f)
    K, S = imu.K, imu.S
    n = K * S
    out = torch.zeros((K, S, 48), dtype=torch.uint8, device=gpu_device)
    wire = torch.full((K, S, 56), ref.SENTINEL, dtype=torch.uint8, device=gpu_device)
    lens = torch.zeros((K, S), dtype=torch.uint8, device=gpu_device)
    box = aof.HostOutbox(n)
    box.array[:] = ob.FILL
    torch.cuda.synchronize()
    tag = 0x4242000001
    engine.bank_imu(imu.samples, imu.times, imu.records_in, imu.state, imu.counts, records_out=out, out_frames=wire, out_lengths=lens,
                    first_seq=f["first_seq"])
    engine.bank_collect(out, wire, lens, capacity_messages=n, outbox=box, tag=tag)
    assert box.wait(tag, timeout_s=5.0), ("the tag did not arrive", hex(box.tag))     # a deadline: fail, never hang
    got = box.array.copy()                                                              # (no synchronisation in front)
    want = f["want"]
    expect = ob.compact(want["records"], want["frames"], want["lengths"], None, None, n, 0, tag=tag)
    assert got.tobytes() == expect.tobytes(), "the outbox against compact() of the model's outputs"
    torch.cuda.synchronize()
    assert got.tobytes() == ob.compact(out, wire, lens, None, None, n, 0, tag=tag).tobytes(), "... and of the IMU call's outputs"
    header, messages, _ = aof.outbox_view(box)
    q = want["records"]["quality"]
    assert int(header["n_messages"]) == int((q >= 0).sum()) == want["tally"]["sent"] > 0
    assert (messages["record"]["quality"] >= 0).all() and (messages["mavlink_len"] > 0).all(), "no dropped record in the outbox"
    assert ((q == ref.STALE_GYRO) | (q == ref.NO_OFFSET)).sum() > 0
    box.close()


def test_a_captured_push_imu_collect_chain_replayed_twice_equals_eager_execution(aof, gpu_device, real_run):
    """One linear graph on one stream (no parallel branches): records-only push -> IMU call -> collect with d_tag; fresh
    frames and samples are copied into the same tensors between the replays."""
    import torch
    run, S = real_run, S_REAL
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    bp = aof.bank_params(S, FX, FY, 0, 0, 1, 100, 0)               # rate 0: every frame publishes
    rng = np.random.default_rng(9)
    clock = np.full(S, 10 ** 9, np.int64)
    ticks = [real_samples(rng, 1, S, clock) for _ in range(3)]
    total = aof.outbox_layout(S, 0).total_bytes

    class Chain:
        def __init__(self):
            self.bank = eng.bank_create(bp, gpu_device)
            self.frames = torch.zeros((S, 64, 64), dtype=torch.uint8, device=gpu_device)
            self.times = torch.zeros(S, dtype=torch.int64, device=gpu_device)
            self.samples = torch.zeros((M_REAL, S, 24), dtype=torch.uint8, device=gpu_device)
            self.counts = torch.zeros(S, dtype=torch.uint8, device=gpu_device)
            self.records = torch.zeros((S, 48), dtype=torch.uint8, device=gpu_device)
            self.wire = torch.zeros((S, 56), dtype=torch.uint8, device=gpu_device)
            self.lens = torch.zeros(S, dtype=torch.uint8, device=gpu_device)
            self.state = torch.zeros((S, 64), dtype=torch.uint8, device=gpu_device)
            self.box = torch.zeros(total, dtype=torch.uint8, device=gpu_device)
            self.tag = torch.zeros(1, dtype=torch.int64, device=gpu_device)
            self.start()

        def start(self):
            eng.bank_reset(self.bank)
            eng.bank_imu_reset(self.state, offset0=123456)

        def load(self, k):
            self.frames.copy_(torch.from_numpy(run.frames[k]))
            self.times.copy_(torch.from_numpy(run.times[k]))
            self.samples.copy_(torch.from_numpy(ticks[k][0].view(np.uint8).reshape(M_REAL, S, 24)))
            self.counts.copy_(torch.from_numpy(ticks[k][1][0]))
            self.tag.fill_(700 + k)
            self.box.fill_(ob.FILL)

        def enqueue(self):
            eng.bank_push(self.bank, self.frames, self.times, None, None, records=self.records)
            eng.bank_imu(self.samples, self.times, self.records, self.state, self.counts, records_out=self.records,
                         out_frames=self.wire, out_lengths=self.lens, first_seq=FIRST_SEQ)
            eng.bank_collect(self.records, self.wire, self.lens, capacity_messages=S, outbox=self.box, tag=0, tag_tensor=self.tag)

        def read(self):
            torch.cuda.synchronize()
            return self.box.cpu().numpy(), self.state.cpu().numpy()

    eager = Chain()
    outs = []
    for k in range(3):
        eager.load(k)
        eager.enqueue()
        outs.append(eager.read())
    assert sum(int(aof.outbox_view(o[0], S)[0]["n_messages"]) for o in outs) >= S
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
        box, state = c.read()
        assert box.tobytes() == outs[k][0].tobytes(), ("replayed outbox", k)
        assert state.tobytes() == outs[k][1].tobytes(), ("replayed states", k)
    eng.close()


# ---- the facade ----

def test_the_facade_with_imu_equals_one_opencv_object_per_stream_completed_by_the_model(aof, synth, gpu_device):
    """OpticalFlowBank with enableImu over 3 streams and 20 ticks, fed interleaved pushImu and push: per stream its entries
    are the non-negative calcFlow returns of one OpticalFlowOpenCV object, filtered and completed (gyro sums, frames) by
    the model."""
    S, T, M = 3, 20, 4
    OFFSET0 = 1_650_000_000_000_000
    run = make_run(synth, 128, 128, S, T, 14, density=0.85, black=False)
    bank = aof.OpticalFlowBank(FX, FY, 15, 128, 128, S)
    assert bank.engineOk()
    assert bank.pushImu(0, 1, 0.0, 0.0, 0.0) == EINVAL, "no enableImu yet"
    assert bank.enableImu(0) == EINVAL and bank.enableImu(17) == EINVAL and bank.engineOk()
    assert bank.enableImu(M, OFFSET0) == 0, bank.lastError()
    assert bank.enableImu(M, OFFSET0) == EINVAL and "already" in bank.lastError() and bank.engineOk()
    assert bank.pushImu(-1, 1, 0.0, 0.0, 0.0) == EINVAL and bank.pushImu(S, 1, 0.0, 0.0, 0.0) == EINVAL
    singles = [aof.OpticalFlowOpenCV(FX, FY, 15, 128, 128) for _ in range(S)]
    rng = np.random.default_rng(3)
    clock = np.full(S, 5 * 10 ** 8, np.int64)
    states = np.zeros(S, ref.STATE_DTYPE)
    states["offset_timestamp_usec"] = OFFSET0
    frames_given = np.zeros(S, np.int64)
    sent = dropped = 0
    for k in range(T):
        samples = np.zeros((1, M, S), ref.SAMPLE_DTYPE)
        counts = np.zeros((1, S), np.uint8)
        for s in range(S):
            # now and then a tick without a sample; stream 0's IMU falls silent behind tick 3: its second publication
            # from there on has no sample since the previous take and is dropped as stale
            n = 0 if (k + s) % 7 == 3 or (s == 0 and k > 3) else int(rng.integers(1, M + 1))
            for j in range(n):
                clock[s] += int(rng.integers(2000, 3000))
                m = (int(clock[s]), *rng.normal(0, 0.5, 3).astype(np.float32), 0)
                samples[0, j, s] = m
                assert bank.pushImu(s, m[0], m[1], m[2], m[3]) == 0
            counts[0, s] = n
            if n == M:
                assert bank.pushImu(s, 1, 0.0, 0.0, 0.0) == ENOBUFS and bank.engineOk(), "a full queue refuses and stays usable"
        records = np.zeros((1, S), ref.RECORD_DTYPE)
        for s in range(S):
            if not run.active[k, s]:
                records[0, s]["quality"] = ref.IDLE
                continue
            frames_given[s] += 1
            q, dt, fx, fy = singles[s].calcFlow(run.frames[k, s], int(run.times[k, s]) & 0xFFFFFFFF)
            r = records[0, s]
            r["quality"], r["frame"] = (q, frames_given[s]) if q >= 0 else (ref.HELD, frames_given[s])
            if q >= 0:
                r["dt_us"], r["flow_x"], r["flow_y"] = dt, np.float32(fx), np.float32(fy)
        want = ref.run(samples, counts, run.times[k:k + 1].astype(np.uint64), records, states, first_seq=0)
        states = want["states"]
        n, entries = bank.push(run.frames[k], run.times[k], run.active[k], run.gyro[k])      # (the gyro argument is ignored)
        assert n == len(entries) >= 0, (n, bank.lastError())
        q = want["records"]["quality"][0]
        assert list(entries["stream"]) == list(np.flatnonzero(q >= 0)), (k, q, entries["stream"])
        for e in entries:
            s, r, w = int(e["stream"]), e["record"], want["records"][0, int(e["stream"])]
            for name in ("quality", "dt_us", "flow_x", "flow_y", "gyro_x", "gyro_y", "gyro_z"):
                assert r[name].tobytes() == w[name].tobytes(), (k, s, name, r, w)
            ln = int(want["lengths"][0, s])
            assert int(e["mavlink_len"]) == ln > 0 and bytes(e["mavlink"][:ln]) == want["frames"][0, s, :ln].tobytes(), (k, s)
        sent += n
        dropped += int(((q == ref.STALE_GYRO) | (q == ref.NO_OFFSET)).sum())
    assert sent >= 2 * S and dropped >= 1, (sent, dropped)
    # a reset restarts the IMU state as well: the first frames come back, stale (no sample since), so nothing is listed
    assert bank.pushImu(1, int(clock[1]) + 1000, 0.1, 0.1, 0.1) == 0       # queued, then dropped with the stream's past
    assert bank.reset(None) == 0
    t0 = np.full(S, 1_000_000, np.int64)
    n, entries = bank.push(run.frames[0], t0, None, None)
    assert n == 0 and bank.engineOk()
    for s in range(S):
        assert bank.pushImu(s, int(clock[s]) + 2500, 0.1, 0.1, 0.1) == 0
    n, entries = bank.push(run.frames[1], t0 + 100000, None, None)       # (behind the limiter's interval: published)
    assert n == S and (entries["mavlink_len"] > 0).all(), "published again, with a fresh sample: sent"
    for f in singles:
        f.close()
    bank.close()
