"""The stream bank's auto-exposure control on the device (aof_bank_exposure_control_device / aof_bank_exposure_reset_device,
include/aof.h) and the facade's sensor-frame form (OpticalFlowBank::pushCamera): states and commands must equal, byte for
byte, the numpy float32 model of tests/exposure_control_ref.py and aof_exposure_control_host -- on synthetic [K][S]
records of the coverage family (no flow needed), and end to end behind camera pushes and camera bursts, where the model
is fed the oracle's mean sample values (tests/bank_camera_ref.py).  Every command buffer is pre-filled with 0xEE and has
guard bytes behind it."""
import ctypes as C

import numpy as np
import pytest

import bank_camera_ref as cref
import exposure_control_ref as xref
from bank_cases import make_burst_run
from bank_ref import FX, FY
from bank_rig import EINVAL, EIO, FILL, OFFSET, BankRig, Guarded, params_of, same, same_exposure
from bank_rig import engine, time_limit   # (this module's fixtures too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

UPDATES = 32          # updates per stream of the synthetic runs: two calls of K = 16


class Controller:
    """S controller states and a [K][S] command buffer on the device, both with guard bytes; skew: the tensors start that
    many bytes into their allocations (4: the pointers are only 4-byte aligned)."""

    def __init__(self, aof, eng, gpu_device, S, K, states, skew=0):
        import torch
        self.aof, self.eng, self.torch, self.S, self.K, self.dev = aof, eng, torch, S, K, gpu_device
        self.state_buf, self.cmd_buf = Guarded(gpu_device, (S, 16), skew=skew), Guarded(gpu_device, (K, S, 16), skew=skew)
        self.state, self.commands = self.state_buf.tensor, self.cmd_buf.tensor
        self.records = torch.zeros(48 * K * S + 64, dtype=torch.uint8, device=gpu_device)[skew:skew + 48 * K * S].view(K, S, 48)
        eng.bank_exposure_reset(self.state, exposures=torch.from_numpy(states["exposure"].astype(np.int16)).to(gpu_device),
                                gains=torch.from_numpy(np.ascontiguousarray(states["gain"])).to(gpu_device))

    def load(self, records):
        """records: RECORD_DTYPE [k, S], k <= K."""
        k = len(records)
        self.records[:k].copy_(self.torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(k, self.S, 48)))
        self.cmd_buf.refill()
        return k

    def run(self, records):
        k = self.load(records)
        self.eng.bank_exposure_control(self.records[:k], self.state, self.commands[:k])
        return self.read(k)

    def read(self, k):
        """(states, commands of the first k rounds); the bytes around both must be untouched."""
        self.torch.cuda.synchronize()
        return (self.state_buf.read().reshape(-1).view(self.aof.EXPOSURE_STATE_DTYPE),
                self.cmd_buf.read(16 * k * self.S).view(self.aof.EXPOSURE_COMMAND_DTYPE).reshape(k, self.S))


_synthetic = {}


def synthetic(S):
    """The coverage family for S streams over UPDATES updates as records with gaps (S = 48: every record due, the family
    itself), and the model's answer, computed once per S: (states0, records, model states after 16 and 32 updates,
    commands, tally)."""
    if S not in _synthetic:
        states0, msv = xref.family(S, UPDATES)
        if S == 48:
            due = np.ones(msv.shape, bool)
        else:
            rng = np.random.default_rng(S)
            due = rng.random(msv.shape) < 0.7
            due[3:9, 0] = False                         # a gap
            if S > 2:
                due[:, S // 2] = False                  # a stream that is never due
        records = xref.records_of(msv, due)
        half, first, _ = xref.control(records[:16], states0)
        full, second, _ = xref.control(records[16:], half)
        tally = xref.control(records[:24], states0)[2] if S == 48 else None
        _synthetic[S] = (states0, records, half, full, np.concatenate([first, second]), tally)
    return _synthetic[S]


@pytest.mark.parametrize("S", [1, 48, 63, 257, 300])
@pytest.mark.parametrize("K", [1, 2, 16])
def test_states_and_commands_equal_the_model_and_the_host_function(aof, engine, gpu_device, K, S):
    states0, records, half, full, commands, tally = synthetic(S)
    if S == 48:
        assert all(tally[name] > 0 for name in xref.OUTCOMES), tally      # 48 x 24: all 17 outcomes
    ctl = Controller(aof, engine, gpu_device, S, K, states0)
    host = states0.copy()
    same(ctl.read(0)[0], states0, "reset")
    for u in range(0, UPDATES, K):
        got_states, got_commands = ctl.run(records[u:u + K])
        host_commands = aof.exposure_control_host(records[u:u + K], host)
        same(got_commands, commands[u:u + K], ("commands against the model", u))
        same(got_commands, host_commands, ("commands against the host function", u))
        same(got_states, host, ("states against the host function", u))
        if u + K == 16:
            same(got_states, half, "states against the model after 16 updates")
    same(got_states, full, "states against the model")
    not_due = records["due"] == 0
    assert (S == 48) == (not not_due.any())


@pytest.mark.parametrize("S", [63, 300])
def test_pointers_that_are_only_four_byte_aligned(aof, engine, gpu_device, S):
    states0, records, half, full, commands, _ = synthetic(S)
    ctl = Controller(aof, engine, gpu_device, S, 16, states0, skew=4)
    assert ctl.state.data_ptr() % 16 == 4 and ctl.commands.data_ptr() % 16 == 4 and ctl.records.data_ptr() % 8 == 4
    for u in (0, 16):
        got_states, got_commands = ctl.run(records[u:u + 16])
        same(got_commands, commands[u:u + 16], u)
    same(got_states, full, "states")


def test_one_call_of_16_rounds_leaves_what_16_calls_of_one_round_leave(aof, engine, gpu_device):
    S = 300
    states0, records, half, full, commands, _ = synthetic(S)
    burst, twin = Controller(aof, engine, gpu_device, S, 16, states0), Controller(aof, engine, gpu_device, S, 1, states0)
    got_states, got_commands = burst.run(records[:16])
    for k in range(16):
        twin_states, twin_commands = twin.run(records[k:k + 1])
        same(twin_commands[0], got_commands[k], ("round", k))
    same(got_states, twin_states, "states")
    same(got_states, half, "model")


def test_a_masked_reset_restarts_only_the_masked_streams(aof, engine, gpu_device):
    import torch
    S = 257
    states0, records, half, full, commands, _ = synthetic(S)
    ctl = Controller(aof, engine, gpu_device, S, 16, states0)
    got_states, _ = ctl.run(records[:16])
    same(got_states, half, "before the reset")
    ctl.cmd_buf.refill()                                # (a reset writes no command either: read(0) looks)
    mask =(np.arange(S) % 3 == 1).astype(np.uint8)
    assert (half["updates"][mask == 1] > 0).any()
    # scalars for the masked streams ...
    engine.bank_exposure_reset(ctl.state, torch.from_numpy(mask).to(gpu_device), exposure0=1234, gain0=56)
    want = half.copy()
    want[mask == 1] = xref.new_states([1234], [56])[0]
    same(ctl.read(0)[0], want, "masked reset from the scalars")
    # ... and per-stream arrays where they are given (the gain alone: the exposure from the scalar)
    gains = (np.arange(S) % 100 + 1).astype(np.uint8)
    mask2 = (np.arange(S) % 5 == 0).astype(np.uint8)
    engine.bank_exposure_reset(ctl.state, torch.from_numpy(mask2).to(gpu_device), exposure0=77, gain0=9,
                               gains=torch.from_numpy(gains).to(gpu_device))
    fresh = xref.new_states(np.full(S, 77), gains)
    want[mask2 == 1] = fresh[mask2 == 1]
    same(ctl.read(0)[0], want, "masked reset from the gain array")
    # the controller goes on from there
    got_states, got_commands = ctl.run(records[16:])
    model_states, model_commands, _ = xref.control(records[16:], want)
    same(got_commands, model_commands, "commands behind the reset")
    same(got_states, model_states, "states behind the reset")


def test_commands_in_host_memory_are_read_behind_a_polled_collect_tag(aof, engine, gpu_device):
    """Commands kept in aof_outbox_alloc_host memory: control, then a collect on the same stream; once the host has seen
    the collect's tag it reads the commands without any synchronisation."""
    import torch
    S, K = 300, 16
    states0, records, half, full, commands, _ = synthetic(S)
    ctl = Controller(aof, engine, gpu_device, S, K, states0)
    mem = C.c_void_p()
    assert aof.lib.aof_outbox_alloc_host(16 * K * S, C.byref(mem)) == 0
    pinned = np.frombuffer((C.c_uint8 * (16 * K * S)).from_address(mem.value), dtype=np.uint8)
    box = aof.HostOutbox(S)
    ticks = np.zeros(S, aof.TICK_DTYPE)
    ticks["quality"] = aof.TICK_IDLE
    ticks = torch.from_numpy(ticks.view(np.uint8).reshape(S, 48)).to(gpu_device)
    for call, (u, tag) in enumerate(((0, 0x51), (16, 0x7700000052))):
        ctl.load(records[u:u + K])
        pinned[:] = FILL
        box.array[:] = FILL
        torch.cuda.synchronize()
        engine.bank_exposure_control(ctl.records, ctl.state, pinned)
        engine.bank_collect(ticks, capacity_messages=S, outbox=box, tag=tag)
        assert box.wait(tag, timeout_s=5.0), ("the tag did not arrive", hex(box.tag))     # a deadline: fail, never hang
        got = pinned.copy()                                                                 # (no synchronisation in front)
        same(got.view(aof.EXPOSURE_COMMAND_DTYPE).reshape(K, S), commands[u:u + K], ("host memory", call))
    torch.cuda.synchronize()
    same(ctl.read(0)[0], full, "states")
    pinned = None
    box.close()
    assert aof.lib.aof_outbox_free_host(mem) == 0


def test_a_captured_control_launch_replayed_twice_equals_the_eager_twin(aof, engine, gpu_device):
    """One linear graph (one stream, no parallel branches) of the control launch; new records are copied into the same
    input tensor between the replays."""
    import torch
    S, K = 257, 16
    states0, records, half, full, commands, _ = synthetic(S)
    eager = Controller(aof, engine, gpu_device, S, K, states0)
    outs = [eager.run(records[u:u + K]) for u in (0, 16)]
    ctl = Controller(aof, engine, gpu_device, S, K, states0)
    ctl.run(records[:K])                                  # (the kernel has run once before the capture)
    engine.bank_exposure_reset(ctl.state, exposures=torch.from_numpy(states0["exposure"].astype(np.int16)).to(gpu_device),
                               gains=torch.from_numpy(np.ascontiguousarray(states0["gain"])).to(gpu_device))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        engine.bank_exposure_control(ctl.records, ctl.state, ctl.commands)
    engine.bank_exposure_reset(ctl.state, exposures=torch.from_numpy(states0["exposure"].astype(np.int16)).to(gpu_device),
                               gains=torch.from_numpy(np.ascontiguousarray(states0["gain"])).to(gpu_device))
    for i, u in enumerate((0, 16)):
        ctl.load(records[u:u + K])
        g.replay()
        got_states, got_commands = ctl.read(K)
        same(got_commands, outs[i][1], ("replay", i))
        same(got_states, outs[i][0], ("replay states", i))
    same(got_states, full, "model")


def test_refused_calls_write_nothing(aof, engine, gpu_device):
    import torch
    S, K = 63, 2
    states0, records, half, full, commands, _ = synthetic(S)
    ctl = Controller(aof, engine, gpu_device, S, K, states0)
    ctl.load(records[:K])
    before = ctl.read(0)[0]
    stream = torch.cuda.current_stream().cuda_stream
    call, ec = aof.lib.aof_bank_exposure_control_device, aof.exposure_control_default()

    def control(**kw):
        c = aof.exposure_control_default()
        for name, value in kw.items():
            setattr(c, name, value)
        return c

    def args(**kw):
        e = kw.get("ec", ec)
        return [kw.get("ctx", engine._ctx), C.byref(e) if e is not None else None, kw.get("S", S), kw.get("K", K),
                kw.get("recs", ctl.records.data_ptr()), kw.get("state", ctl.state.data_ptr()),
                kw.get("cmds", ctl.commands.data_ptr()), stream]

    refused = [dict(ctx=None), dict(ec=None), dict(recs=None), dict(state=None), dict(cmds=None), dict(S=0), dict(S=-4),
               dict(K=0), dict(K=aof.BANK_BURST_MAX + 1), dict(recs=ctl.records.data_ptr() + 2),
               dict(state=ctl.state.data_ptr() + 2), dict(cmds=ctl.commands.data_ptr() + 1),
               dict(ec=control(exposure_p=float("nan"))), dict(ec=control(gain_change_threshold=float("inf"))),
               dict(ec=control(exposure_max=0.0)), dict(ec=control(exposure_max=65536.0)), dict(ec=control(gain_max=0.5)),
               dict(ec=control(gain_max=256.0))]
    for kw in refused:
        assert call(*args(**kw)) == EINVAL, kw
    reset = aof.lib.aof_bank_exposure_reset_device
    assert reset(None, S, None, 1, 1, None, None, ctl.state.data_ptr(), stream) == EINVAL
    assert reset(engine._ctx, 0, None, 1, 1, None, None, ctl.state.data_ptr(), stream) == EINVAL
    assert reset(engine._ctx, S, None, 1, 1, None, None, None, stream) == EINVAL
    assert reset(engine._ctx, S, None, 1, 1, None, None, ctl.state.data_ptr() + 2, stream) == EINVAL
    assert b"exposure" in aof.lib.aof_last_error(engine._ctx)
    got_states, got_commands = ctl.read(0)
    same(got_states, before, "a refused call must leave the states untouched")
    assert (ctl.cmd_buf.alloc.cpu().numpy() == FILL).all(), "a refused call must write no command"
    # the context is still usable, with the widest constants allowed
    assert call(*args(ec=control(exposure_max=65535.0, gain_max=255.0))) == 0
    wide = xref.control(records[:K], states0, xref.Constants(exposure_max=65535.0, gain_max=255.0))
    got_states, got_commands = ctl.read(K)
    same(got_commands, wide[1], "exposure_max 65535, gain_max 255")
    same(got_states, wide[0], "exposure_max 65535, gain_max 255: states")


def test_a_faulted_context_controls_nothing(aof, synth, gpu_device):
    """The context's sticky device-side condition (raised as tests/test_gpu_bank_outbox.py raises it): -EIO before the
    launch, states and commands keep their bytes."""
    import torch
    S, K = 63, 2
    states0, records, *_ = synthetic(S)
    p = aof.default_params(640, 480)
    hp, hc, _ = synth.make_batch(640, 480, 8, 4, 4300)
    idx = np.arange(256) % 8
    eng = aof.FlowEngine(p, 0)
    ctl = Controller(aof, eng, gpu_device, S, K, states0)
    ctl.load(records[:K])
    eng.set_search_mode(aof.SEARCH_EXHAUSTIVE)
    eng.set_reduce_fusion(True)
    eng.debug_vote_deadline_ticks(0)
    eng.flow_batch(torch.from_numpy(hp[idx]).to(gpu_device), torch.from_numpy(hc[idx]).to(gpu_device))
    torch.cuda.synchronize()
    with pytest.raises(aof.AofError) as e:
        eng.bank_exposure_control(ctl.records, ctl.state, ctl.commands)
    assert e.value.code == EIO
    with pytest.raises(aof.AofError) as e:
        eng.bank_exposure_reset(ctl.state)
    assert e.value.code == EIO
    same(ctl.read(0)[0], states0, "states")
    assert (ctl.cmd_buf.alloc.cpu().numpy() == FILL).all()
    eng.close()


# ---- end to end: camera push -> control, against the model fed the oracle's mean sample values ---------------------------

CONFIGS = {"px4-64-from-320x240": ("px4-64", (320, 240), 6, 41), "opencv-128-from-640x480": ("opencv-128", (640, 480), 4, 42)}
K_BURST, BURSTS = 4, 6                # 24 ticks, as 24 camera pushes or as 6 camera bursts of 4 rounds
INTERVAL = 12_000                     # us: an active frame every 9..18 ms, about half of the ticks active: about 8 updates
BRIGHTNESS = (0.12, 1.0, 0.12, 1.7, 0.5, 0.12)     # per stream: dark scenes saturate the exposure and reach for the gain
START = ((1700, 1), (400, 1), (1727, 1), (900, 1), (1727, 90), (20, 1))


class EndToEnd:
    """The inputs of one configuration and what the model expects, made once on the CPU: a burst-shaped run (stream s has
    frames in rounds 0..count-1 of each burst, so that the same run serves single ticks and bursts) with per-stream
    brightness, its sensor frames, the gate, the oracle's exposure records and the model's commands and states."""

    def __init__(self, aof, orc, synth, name):
        cfg, sensor, S, seed = CONFIGS[name]
        self.p, self.S, self.sensor, self.seed = params_of(aof, cfg), S, sensor, seed
        p = self.p
        self.run, self.counts, self.given = make_burst_run(synth, p.width, p.height, S, K_BURST, BURSTS, seed)
        for s in range(S):
            lit = self.run.active[:, s] == 1
            self.run.frames[lit, s] = np.clip(self.run.frames[lit, s].astype(np.float32) * BRIGHTNESS[s % 6], 0, 255).astype(np.uint8)
        cref.add_saturated_patches(self.run)
        self.T = self.run.T
        self.cam = aof.bank_camera_params(sensor[0], sensor[1], p.width, p.height, 0, INTERVAL, None, FX, FY)
        self.cam_run = cref.CameraRun(self.run, sensor[0], sensor[1], seed)
        self.due, _ = cref.gate(self.run.times, self.run.active, INTERVAL)
        self.sensors = [self.cam_run.sensor(k) for k in range(self.T)]
        self.records = np.stack([cref.expected_exposure(aof, orc, self.sensors[k], self.run, k, self.due[k]) for k in range(self.T)])
        self.states0 = xref.new_states([START[s % 6][0] for s in range(S)], [START[s % 6][1] for s in range(S)])
        self.states, self.commands, _ = self.model(self.states0)
        # conditions on the INPUT, asserted on the model: a controller that never commands, or always does, cannot pass
        flags, updates = self.commands["flags"], self.due.sum(0)
        assert (flags & xref.SET_EXPOSURE).any() and (flags & xref.SET_GAIN).any() and (flags == xref.UPDATED).any(), flags
        assert 2 <= updates.min() and 6 <= updates.mean() <= 10, updates       # about 8 per stream
        assert (self.states["updates"] == updates).all()

    def model(self, states0):
        states, out = states0, []
        for b in range(0, self.T, 8):
            states, commands, _ = xref.control(self.records[b:b + 8], states)
            out.append(commands)
        return states, np.concatenate(out), None

    def bp(self, aof):
        return aof.bank_params(self.S, FX, FY, 15, OFFSET, 1, 100, 0)

    def new_controller_state(self, aof, eng, gpu_device):
        import torch
        state = torch.zeros((self.S, 16), dtype=torch.uint8, device=gpu_device)
        eng.bank_exposure_reset(state, exposures=torch.from_numpy(self.states0["exposure"].astype(np.int16)).to(gpu_device),
                                gains=torch.from_numpy(np.ascontiguousarray(self.states0["gain"])).to(gpu_device))
        return state


_end_to_end = {}


@pytest.fixture
def e2e(aof, orc, synth, request):
    name = request.param
    if name not in _end_to_end:
        _end_to_end[name] = EndToEnd(aof, orc, synth, name)
    return _end_to_end[name]


@pytest.mark.parametrize("e2e", sorted(CONFIGS), indirect=True)
def test_camera_push_then_control_equals_the_model_fed_the_oracles_msv(aof, gpu_device, e2e):
    import torch
    eng = aof.FlowEngine(e2e.p, 0)
    dev = BankRig(aof, eng, e2e.run, e2e.bp(aof), gpu_device, camera=(e2e.cam, e2e.cam_run))
    state = e2e.new_controller_state(aof, eng, gpu_device)
    commands = torch.zeros((e2e.S, 16), dtype=torch.uint8, device=gpu_device)
    host = e2e.states0.copy()
    for k in range(e2e.T):
        dev.load(k, sensors=e2e.sensors[k])
        commands.fill_(FILL)
        dev.enqueue()
        eng.bank_exposure_control(dev.exposure, state, commands)
        torch.cuda.synchronize()
        got_records = aof.exposure_view(dev.exposure)
        same_exposure(got_records, e2e.records[k], k, "the push's exposure records against the oracle")
        got = aof.exposure_commands_view(commands)
        same(got, e2e.commands[k], ("commands against the model", k))
        same(got, aof.exposure_control_host(got_records, host), ("commands against the host function", k))
    same(aof.exposure_states_view(state), e2e.states, "states against the model")
    same(aof.exposure_states_view(state), host, "states against the host function")
    eng.close()


@pytest.mark.parametrize("e2e", sorted(CONFIGS), indirect=True)
def test_the_same_run_as_camera_bursts(aof, gpu_device, e2e):
    """6 camera bursts of 4 rounds, one control call of 4 rounds behind each: the commands and states of the 24 ticks."""
    import torch
    eng = aof.FlowEngine(e2e.p, 0)
    dev = BankRig(aof, eng, e2e.run, e2e.bp(aof), gpu_device, K=K_BURST, camera=(e2e.cam, e2e.cam_run))
    state = e2e.new_controller_state(aof, eng, gpu_device)
    commands = torch.zeros((K_BURST, e2e.S, 16), dtype=torch.uint8, device=gpu_device)
    for j in range(BURSTS):
        ticks = slice(j * K_BURST, (j + 1) * K_BURST)
        dev.load(j, e2e.given, e2e.sensors[ticks])
        commands.fill_(FILL)
        dev.enqueue()
        eng.bank_exposure_control(dev.exposure, state, commands)
        torch.cuda.synchronize()
        got_records = dev.exposure.cpu().numpy().view(aof.EXPOSURE_DTYPE).reshape(K_BURST, e2e.S)
        same(got_records, e2e.records[ticks], ("the burst's exposure records against the oracle", j))
        same(aof.exposure_commands_view(commands), e2e.commands[ticks], ("commands against the model", j))
    same(aof.exposure_states_view(state), e2e.states, "states against the model")
    eng.close()


@pytest.mark.parametrize("e2e", sorted(CONFIGS), indirect=True)
def test_the_facades_push_camera_equals_one_opencv_object_per_stream_and_the_model(aof, gpu_device, e2e):
    """OpticalFlowBank::pushCamera on sensor frames: per stream the messages of an OpticalFlowOpenCV object fed the crops
    and (uint32_t) times, bit for bit; the commands of every tick are the model's (every controller from one start)."""
    S, run, p = e2e.S, e2e.run, e2e.p
    bank = aof.OpticalFlowBank(FX, FY, 15, p.width, p.height, S)
    assert bank.engineOk() and bank.exposureCommands() is None
    assert bank.enableCamera(e2e.sensor[0], e2e.sensor[1], 1700, 1, INTERVAL) == 0, bank.lastError()
    assert not bank.exposureCommands().view(np.uint8).any()
    singles = [aof.OpticalFlowOpenCV(FX, FY, 15, p.width, p.height) for _ in range(S)]
    assert bank.getPyramidLevels() == singles[0].getPyramidLevels()
    states0 = xref.new_states(np.full(S, 1700), np.full(S, 1))
    states, commands, _ = e2e.model(states0)
    flags = commands["flags"]
    assert (flags & xref.SET_EXPOSURE).any() and (flags & xref.SET_GAIN).any() and (flags == xref.UPDATED).any(), flags
    got, want = [[] for _ in range(S)], [[] for _ in range(S)]
    published = 0
    for k in range(e2e.T):
        n, entries = bank.pushCamera(e2e.sensors[k], run.times[k], run.active[k], run.gyro[k])
        assert n == len(entries) >= 0, (n, bank.lastError())
        same(bank.exposureCommands(), commands[k], ("commands against the model", k))
        for e in entries:
            s, r = int(e["stream"]), e["record"]
            got[s].append((k, int(r["quality"]), int(r["dt_us"]), r["flow_x"].tobytes(), r["flow_y"].tobytes()))
        for s in range(S):
            if run.active[k, s]:
                q, dt, fx, fy = singles[s].calcFlow(run.frames[k, s], int(run.times[k, s]) & 0xFFFFFFFF)
                if q >= 0:
                    want[s].append((k, q, dt, np.float32(fx).tobytes(), np.float32(fy).tobytes()))
        published += n
    assert got == want and published >= S, published          # (at least every stream's first frame)
    # a second enableCamera() and a sensor smaller than the image are refused and leave the object usable
    assert bank.enableCamera(e2e.sensor[0], e2e.sensor[1], 1, 1) == EINVAL and "already" in bank.lastError()
    assert bank.engineOk()
    small = aof.OpticalFlowBank(FX, FY, 15, p.width, p.height, 1)
    assert small.enableCamera(p.width - 1, p.height, 1, 1) == EINVAL and small.engineOk() and small.exposureCommands() is None
    small.close()
    # the plain push still works on the grown bank
    assert bank.reset(None) == 0
    n, entries = bank.push(run.frames[0], run.times[0], None, None)
    assert n == S and (entries["record"]["frame"] == 1).all()
    for f in singles:
        f.close()
    bank.close()
