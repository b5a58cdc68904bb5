"""aof_sequence_field_device (include/aof_sequence_field.h) on the device: against aof_sequence_field_host byte for byte on
d_fields, d_out and the state over fabricated workspaces (no sequence call in front: designed block records at 25 blocks a
pair, flows, records and count words written at the layout's offsets of a sentinel-filled workspace) at every edge of the
window pass; end to end behind aof_sequence_device against a one-stream bank with aof_bank_field_device behind every push; in
front of and behind aof_sequence_imu_device; from one captured graph; the refusals; a corrupted count word and record frames
out of order, which must stay inside every array; and a NULL state.  The workspace is only read: every byte of it is
compared.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import bank_field_rig as bank_rig
import imu_ref as imu
import sequence_field_ref as ref
import sequence_field_rig as rig
import sequence_imu_rig as imu_rig
from bank_rig import FILL, GUARD, Guarded, time_limit   # noqa: F401  (time_limit: this module's autouse fixture too)
from sequence_ref import crop_of

pytestmark = pytest.mark.gpu

FX, FY = 216.6677, 216.2457
RECORD_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 513)


@pytest.fixture(scope="module")
def px4(aof, gpu_device):
    """PX4 64 x 64: 25 blocks a pair, sub-pixel (the sub-directions reach the fit)."""
    p = aof.px4flow_params(64, 64)
    eng = aof.FlowEngine(p, 0)
    assert eng.nblocks(0) == 25 and p.subpixel
    yield eng, p, aof.sequence_params(64, 64, 64, 64, FX, FY, 15)
    eng.close()


class Fabricated:
    """A sentinel-filled workspace for n frames with fabricated records, flows and block records, on the device between guard
    bytes, the three outputs each between guard bytes of their own (fields 8-byte aligned and no more, records 4-byte
    aligned and no more), and what the host function makes of the same arrays."""

    def __init__(self, aof, eng, p, sp, gpu_device, n):
        import torch
        self.aof, self.eng, self.p, self.sp, self.dev, self.torch, self.n = aof, eng, p, sp, gpu_device, torch, n
        self.L = L = aof.sequence_layout(p, sp, n)
        self.alloc = torch.empty(L.total_bytes + 2 * GUARD, dtype=torch.uint8, device=gpu_device)
        self.ws = self.alloc[GUARD:GUARD + L.total_bytes]
        assert self.ws.data_ptr() % 256 == 0
        self.at_blocks, self.at_subdirs = rig.block_offsets(aof, p, L, n)
        self.fields = Guarded(gpu_device, (max(n - 1, 1) * 64,), skew=264)
        self.out = Guarded(gpu_device, (n * 48,), skew=260)
        self.state = Guarded(gpu_device, (64,), skew=8)
        assert self.fields.tensor.data_ptr() % 16 == 8 and self.out.tensor.data_ptr() % 8 == 4

    def put(self, offset, a):
        t = rig.up(self.torch, a, self.dev)
        assert offset + t.numel() <= self.L.total_bytes
        self.ws[offset:offset + t.numel()].copy_(t)

    def load(self, records, blocks, subdirs, flows, count0=None):
        L = self.L
        self.alloc.fill_(FILL)
        for g in (self.fields, self.out, self.state):
            g.refill()
        self.put(L.count, np.array([len(records) if count0 is None else count0, 0, 0, 0], np.uint32))
        self.put(L.records, records)
        if self.n > 1:
            self.put(L.flows, flows)
            self.put(self.at_blocks, blocks)
            self.put(self.at_subdirs, subdirs)
        self.before = self.alloc.clone()

    def run(self, state=True, fp=None):
        rc = rig.device(self.aof, self.eng, self.sp, self.n, self.ws, self.fields.tensor, self.out.tensor,
                        self.state.tensor if state else None, fp=fp)
        assert rc == 0, self.aof.lib.aof_last_error(self.eng._ctx)

    def read(self, M):
        """(fields [n - 1], out [M], state [1]) as records; the workspace and every byte around an output must be untouched."""
        self.torch.cuda.synchronize()
        assert self.torch.equal(self.alloc, self.before), "the workspace is only read"
        fields = self.fields.read().view(self.aof.FIELD_DTYPE)[:self.n - 1] if self.n > 1 else np.zeros(0, self.aof.FIELD_DTYPE)
        if self.n == 1:
            assert (self.fields.read() == FILL).all()
        return fields, self.out.read(used=48 * M).view(rig.RECORD_DTYPE), self.state.read().view(rig.STATE_DTYPE)

    def same_as_host(self, records, blocks, subdirs, flows, what, fp=None):
        rc, w_fields, w_out, w_state = rig.host(self.aof, self.p, self.sp, self.n, blocks, subdirs, flows, records, fp=fp)
        assert rc == 0
        fields, out, state = self.read(len(records))
        assert fields.tobytes() == w_fields.tobytes(), (what, "fields", differing(fields, w_fields))
        assert out.tobytes() == w_out.tobytes(), (what, "records", differing(out, w_out))
        assert state.tobytes() == w_state.tobytes(), (what, "state", state, w_state)
        return w_fields, w_out, w_state


def differing(got, want):
    return [(i, got[i], want[i]) for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()][:2]


# ---- 1. fabricated workspaces --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", RECORD_COUNTS)
def test_the_kernels_equal_the_host_function_on_fabricated_workspaces(aof, px4, gpu_device, M):
    """Record counts on either side of a wave and of one and two workgroups; short windows, tails of 0, 1 and 2 pairs, two
    windows without a valid fit; both passes of the fit and one."""
    eng, p, sp = px4
    rng = np.random.default_rng(M)
    windows = ref.random_windows(rng, M - 1, longest=9 if M >= 255 else 6)
    records, n = ref.record_list(windows, M % 3, seed=M)
    F = records["frame"]
    empty = [(int(F[m - 1]), int(F[m])) for m in {1, M // 2} if 1 <= m < M]
    blocks, subdirs, flows = ref.designed_pairs(p, n - 1, seed=M, invalid_spans=empty) if n > 1 else (None, None, None)
    fab = Fabricated(aof, eng, p, sp, gpu_device, n)
    for fp in (None, aof.field_params(passes=1, exclude_reach=0)):
        fab.load(records, blocks, subdirs, flows)
        fab.run(fp=fp)
        fields, out, state = fab.same_as_host(records, blocks, subdirs, flows, M, fp=fp)
        assert int(state["published"][0]) == M and int(state["pairs"][0]) == M % 3
        for lo, hi in empty:
            m = int(np.searchsorted(F, hi))
            assert int(out[m]["status"]) == 0 and int(out[m]["pairs"]) == hi - lo and not out[m]["zoom"]
        if M >= 63:
            assert 2 * int((out["status"] >= 1).sum()) >= M and (out["zoom"] != 0).any()


def test_long_windows_and_a_long_tail(aof, px4, gpu_device):
    """Windows on either side of the wave, of 1 024 and of 4 096 pairs, two of them without a valid fit, and a tail of three
    thousand pairs: one lane each."""
    eng, p, sp = px4
    windows = [63, 64, 65, 1, 1023, 1024, 1025, 2, 4095, 4096, 4097, 1]
    records, n = ref.record_list(windows, 3000, seed=1)
    F = records["frame"]
    empty = [(int(F[2]), int(F[3])), (int(F[6]), int(F[7]))]
    blocks, subdirs, flows = ref.designed_pairs(p, n - 1, seed=2, invalid_spans=empty)
    fab = Fabricated(aof, eng, p, sp, gpu_device, n)
    fab.load(records, blocks, subdirs, flows)
    fab.run()
    _, out, state = fab.same_as_host(records, blocks, subdirs, flows, "long")
    assert out["pairs"][1:].tolist() == windows and int(out[3]["status"]) == 0 and int(out[7]["status"]) == 0
    assert int(state["pairs"][0]) == 3000 and int(state["fits"][0]) > 1500


def test_one_frame_and_a_recording_nobody_published(aof, px4, gpu_device):
    eng, p, sp = px4
    records, n = ref.record_list([], 0)
    fab = Fabricated(aof, eng, p, sp, gpu_device, 1)
    fab.load(records, None, None, None)
    fab.run()
    fields, out, state = fab.same_as_host(records, None, None, None, "one frame")
    assert int(out[0]["status"]) == 0 and int(state["published"][0]) == 1 and not int(state["pairs"][0])
    # count[0] == 0: the tail window is the whole recording
    records, n = ref.record_list([3, 4], 5)
    blocks, subdirs, flows = ref.designed_pairs(p, n - 1, seed=3)
    fab = Fabricated(aof, eng, p, sp, gpu_device, n)
    fab.load(records, blocks, subdirs, flows, count0=0)
    fab.run()
    _, _, state = fab.same_as_host(records[:0], blocks, subdirs, flows, "nothing published")
    assert int(state["pairs"][0]) == n - 1 and int(state["published"][0]) == 0


def test_without_a_state_only_fields_and_records_are_written(aof, px4, gpu_device):
    eng, p, sp = px4
    records, n = ref.record_list(ref.random_windows(np.random.default_rng(1), 299), 4, seed=9)
    blocks, subdirs, flows = ref.designed_pairs(p, n - 1, seed=9)
    fab = Fabricated(aof, eng, p, sp, gpu_device, n)
    fab.load(records, blocks, subdirs, flows)
    fab.run(state=False)
    rc, w_fields, w_out, _ = rig.host(aof, p, sp, n, blocks, subdirs, flows, records)
    fields, out, state = fab.read(len(records))
    assert rc == 0 and fields.tobytes() == w_fields.tobytes() and out.tobytes() == w_out.tobytes()
    assert (state.view(np.uint8) == FILL).all()


def test_a_corrupted_count_and_record_frames_out_of_order_stay_inside_every_array(aof, px4, gpu_device):
    """The device call cannot see count[0] or the records; its kernel clamps.  Only that it completes and that nothing around
    an output -- the guard bytes of Guarded, the workspace -- was written."""
    eng, p, sp = px4
    M, n = 600, 640
    rng = np.random.default_rng(6)
    blocks, subdirs, flows = ref.designed_pairs(p, n - 1, seed=6)
    for count0, what in ((0xFFFFFFFF, "count"), (M, "frames")):
        records, _ = ref.record_list([1] * (M - 1), n - M)
        if what == "frames":
            records["frame"] = rng.integers(0, 2 * n, M)                  # no order at all, values behind the recording among them
            records["frame"][::7] = 0xFFFFFFFF
            records["frame"][5] = 0xFFFFFFF0
        full = np.zeros(n, ref.SEQ_RECORD_DTYPE)
        full[:M] = records
        full["frame"][M:] = rng.integers(0, 1 << 32, n - M)               # what a count above M makes the kernel read
        fab = Fabricated(aof, eng, p, sp, gpu_device, n)
        fab.load(full, blocks, subdirs, flows, count0=count0)
        fab.run()
        fab.torch.cuda.synchronize()
        assert fab.torch.equal(fab.alloc, fab.before), "the workspace is only read"
        for g in (fab.fields, fab.out, fab.state):
            g.read()                                                          # (asserts its guard bytes)
        fields = fab.fields.read().view(aof.FIELD_DTYPE)
        assert fields.tobytes() == rig.host(aof, p, sp, n, blocks, subdirs, flows, full[:0])[1].tobytes(), "the fits do not depend on the records"


def test_refused_calls_write_nothing(aof, px4, gpu_device):
    import torch
    eng, p, sp = px4
    records, n = ref.record_list([3, 2, 4, 1], 2)
    blocks, subdirs, flows = ref.designed_pairs(p, n - 1, seed=4)
    fab = Fabricated(aof, eng, p, sp, gpu_device, n)
    fab.load(records, blocks, subdirs, flows)
    call = rig.bind(aof).aof_sequence_field_device
    stream = torch.cuda.current_stream().cuda_stream
    other_crop = aof.sequence_params(96, 96, 32, 32, FX, FY, 15)
    no_focal = aof.sequence_params(64, 64, 64, 64, 0.0, FY, 15)
    wide = aof.FlowEngine(aof.default_params(8192, 2048), 0)             # a grid beyond the fit's integer range
    wide_sp = aof.sequence_params(8192, 2048, 8192, 2048, FX, FY, 15)

    def args(**kw):
        fp = kw.get("fp", aof.field_params())
        s = kw.get("sp", sp)
        return [kw.get("ctx", eng._ctx), None if s is None else C.byref(s), None if fp is None else C.byref(fp), kw.get("n", n),
                kw.get("ws", fab.ws.data_ptr()), kw.get("bytes", fab.L.total_bytes), kw.get("fields", fab.fields.tensor.data_ptr()),
                kw.get("out", fab.out.tensor.data_ptr()), kw.get("state", fab.state.tensor.data_ptr()), stream]

    refused = [dict(ctx=None), dict(sp=None), dict(fp=None), dict(ws=None), dict(fields=None), dict(out=None), dict(n=-1),
               dict(n=0x7FFFFFF0), dict(sp=other_crop), dict(sp=no_focal), dict(ws=fab.ws.data_ptr() + 16),
               dict(fields=fab.fields.tensor.data_ptr() + 4), dict(state=fab.state.tensor.data_ptr() + 4),
               dict(out=fab.out.tensor.data_ptr() + 2), dict(ctx=wide._ctx, sp=wide_sp, n=2, bytes=1 << 40)]
    refused += [dict(fp=aof.field_params(**kw)) for kw in (dict(min_blocks=2), dict(passes=3), dict(exclude_reach=2), dict(gate_px=0.0),
                                                           dict(gate_px=float("nan")))]
    for kw in refused:
        assert call(*args(**kw)) == rig.EINVAL, kw
    assert call(*args(bytes=fab.L.total_bytes - 1)) == rig.ENOSPC
    assert b"sequence field" in aof.lib.aof_last_error(eng._ctx)
    assert call(*args(n=0)) == 0, "no frames: nothing to do"
    torch.cuda.synchronize()
    assert torch.equal(fab.alloc, fab.before), "a refused call must leave the workspace untouched"
    for g in (fab.fields, fab.out, fab.state):
        assert (g.read() == FILL).all()
    wide.close()
    # the context is still usable
    fab.run()
    fab.same_as_host(records, blocks, subdirs, flows, "after the refusals")


# ---- 2. end to end: aof_sequence_device + the field call against a one-stream bank pushed frame by frame ---------------------------
def bank_chain(aof, eng, gpu_device, cropped, d_times, rate, imu_feed=None):
    """A bank of one stream, a tick per frame, aof_bank_field_device behind every push (and behind the bank's IMU call, with
    imu_feed = (samples, sample_end)) -> (ticks TICK_DTYPE [n], fields [n], out [n], final state [1])."""
    import torch
    n = cropped.shape[0]
    bp = aof.bank_params(1, FX, FY, rate, 0, 1, 100, 0)
    bank = eng.bank_create(bp, gpu_device)
    state = torch.zeros((1, 64), dtype=torch.uint8, device=gpu_device)
    assert bank_rig.reset(aof, eng, state) == 0
    if imu_feed is not None:
        samples, sample_end = imu_feed
        istate = torch.zeros((1, 64), dtype=torch.uint8, device=gpu_device)
        eng.bank_imu_reset(istate, offset0=0)
        per_frame = np.diff(np.concatenate([[0], sample_end.astype(np.int64)]))
        slots = int(per_frame.max())
        assert 1 <= slots <= 16
    ticks, outs, fields = [], [], []
    for k in range(n):
        records = eng.bank_push(bank, cropped[k:k + 1], d_times[k:k + 1])
        if imu_feed is not None:
            chunk = np.zeros((slots, 1), imu.SAMPLE_DTYPE)
            lo = int(sample_end[k]) - int(per_frame[k])
            chunk[:per_frame[k], 0] = samples[lo:lo + per_frame[k]]
            eng.bank_imu(imu_rig.up(torch, chunk, gpu_device).view(slots, 1, 24), d_times[k:k + 1], records, istate,
                         torch.tensor([int(per_frame[k])], dtype=torch.uint8, device=gpu_device), records_out=records, mavlink=False)
        o, f = torch.zeros((1, 48), dtype=torch.uint8, device=gpu_device), torch.zeros((1, 64), dtype=torch.uint8, device=gpu_device)
        assert bank_rig.device(aof, eng, bp, bank.buffer, records, state, o, f) == 0, aof.lib.aof_last_error(eng._ctx)
        ticks.append(records.clone()), outs.append(o), fields.append(f)
    torch.cuda.synchronize()
    cut = lambda ts, dt: torch.cat(ts).cpu().numpy().reshape(-1).view(dt).copy()
    return (aof.ticks_view(torch.cat(ticks)).reshape(n), cut(fields, aof.FIELD_DTYPE), cut(outs, rig.RECORD_DTYPE),
            state.cpu().numpy().reshape(-1).view(rig.STATE_DTYPE).copy())


def same_as_the_bank(got, chain, n):
    """got = (records of the sequence call, fields, out, state) against a bank chain."""
    records, fields, out, state = got
    ticks, b_fields, b_out, b_state = chain
    published = np.flatnonzero(b_out["status"] >= 0)
    assert records["frame"].tolist() == published.tolist() and len(published) >= 3
    assert fields.tobytes() == b_fields[1:].tobytes(), ("fits", differing(fields, b_fields[1:]))
    want = b_out[published].copy()
    assert (want["frame"] == published + 1).all()
    want["frame"] = published                              # the sequence counts frames from 0, the bank from 1
    assert out.tobytes() == want.tobytes(), ("records", differing(out, want))
    assert state.tobytes() == b_state.tobytes(), ("final state", state, b_state)
    assert 2 * int((out["status"] >= 1).sum()) >= len(out) and ((out["zoom"] != 0) | (out["rotation"] != 0)).any()


class Outputs:
    """d_fields, d_out and the state of one recording, between guard bytes."""

    def __init__(self, gpu_device, n):
        self.n = n
        self.fields, self.out, self.state = Guarded(gpu_device, ((n - 1) * 64,), skew=8), Guarded(gpu_device, (n * 48,), skew=4), Guarded(gpu_device, (64,), skew=8)

    def read(self, aof, M):
        return (self.fields.read().view(aof.FIELD_DTYPE).copy(), self.out.read(used=48 * M).view(rig.RECORD_DTYPE).copy(),
                self.state.read().view(rig.STATE_DTYPE).copy())


@pytest.mark.parametrize("name", list(ref.E2E))
def test_sequence_and_field_call_equal_a_one_stream_bank_pushed_frame_by_frame(aof, synth, gpu_device, name):
    import torch
    case = ref.E2E[name]
    cw, ch = case["crop"]
    cam_w, cam_h = case["cam"]
    n, rate = case["n"], case["rate"]
    frames, times = ref.e2e_recording(synth, case)
    eng = aof.FlowEngine(ref.e2e_params(aof, case), 0)
    if case["generic"]:
        eng.force_generic(True)
    d_frames, d_times = torch.from_numpy(frames).to(gpu_device), torch.from_numpy(times).to(gpu_device)
    chain = bank_chain(aof, eng, gpu_device, torch.from_numpy(crop_of(frames, cw, ch)).to(gpu_device), d_times, rate)
    forms = [None] + ([(4.5, 0.01)] if name == "px4-64-rate15" else [])          # and once behind a de-rotating sequence call
    for derotate in forms:
        sp = aof.sequence_params(cam_w, cam_h, cw, ch, FX, FY, rate, 0, 1, 100, 0, derotate=derotate)
        gyro = None if derotate is None else torch.zeros((n, 4), dtype=torch.float32, device=gpu_device)
        o = Outputs(gpu_device, n)
        ws, L = eng.sequence(sp, d_frames, d_times, gyro=gyro)
        before = ws.clone()
        assert rig.device(aof, eng, sp, n, ws, o.fields.tensor, o.out.tensor, o.state.tensor) == 0, aof.lib.aof_last_error(eng._ctx)
        torch.cuda.synchronize()
        assert torch.equal(ws, before), "the workspace is only read"
        seq = eng.sequence_outputs(sp, ws, L, n)
        assert seq["status"] == 0
        same_as_the_bank((seq["records"],) + o.read(aof, len(seq["records"])), chain, n)
        if rate > 0:
            assert int(chain[2]["pairs"].max()) >= 3
    eng.close()


# ---- 3. in front of and behind the sequence IMU call ---------------------------------------------------------------------------------
def test_in_front_of_and_behind_the_sequence_imu_call(aof, synth, gpu_device):
    """Samples at 250 Hz with the autopilot silent for 0.3 s: the records of that stretch turn AOF_TICK_STALE_GYRO, and their
    windows close all the same -- whichever call runs first, and in the bank's chain."""
    import torch
    case = dict(ref.E2E["px4-64-rate15"], n=45, seed=6)
    n, rate = case["n"], case["rate"]
    frames, times = ref.e2e_recording(synth, case)
    arrival = np.arange(-20000, int(times[-1]) + 20000, 4000)
    arrival = arrival[(arrival <= times[12]) | (arrival > times[12] + 300000)]
    samples = np.zeros(len(arrival), imu.SAMPLE_DTYPE)
    samples["time_usec"] = 7_000_000 + arrival
    rng = np.random.default_rng(2)
    samples["xgyro"], samples["ygyro"], samples["zgyro"] = rng.normal(0, 0.8, (3, len(arrival))).astype(np.float32)
    sample_end = np.searchsorted(arrival, times, side="left").astype(np.uint32)
    eng = aof.FlowEngine(ref.e2e_params(aof, case), 0)
    sp = aof.sequence_params(160, 120, 64, 64, FX, FY, rate, 0, 1, 100, 0)
    d_frames, d_times = torch.from_numpy(frames).to(gpu_device), torch.from_numpy(times).to(gpu_device)
    d_samples = imu_rig.up(torch, samples, gpu_device).view(-1, 24)
    d_end = imu_rig.up(torch, sample_end, gpu_device).view(torch.int32)
    ip = imu_rig.params(len(samples), 0, 1, 100, 0)
    got = []
    for field_first in (True, False):
        o = Outputs(gpu_device, n)
        ws, L = eng.sequence(sp, d_frames, d_times)
        calls = [lambda: rig.device(aof, eng, sp, n, ws, o.fields.tensor, o.out.tensor, o.state.tensor),
                 lambda: imu_rig.device(aof, eng, sp, ip, n, d_times, d_samples, d_end, ws, None)]
        for call in (calls if field_first else calls[::-1]):
            assert call() == 0, aof.lib.aof_last_error(eng._ctx)
        torch.cuda.synchronize()
        seq = eng.sequence_outputs(sp, ws, L, n)
        got.append((seq["records"].copy(),) + o.read(aof, len(seq["records"])))
    for a, b in zip(got[0], got[1]):
        assert a.tobytes() == b.tobytes(), "in front of the IMU call and behind it"
    stale = got[0][0]["quality"] == imu.STALE_GYRO
    assert stale.sum() >= 2 and (got[0][0]["quality"] >= 0).sum() >= 3
    assert (got[0][2]["status"][stale] >= 0).all() and (got[0][2]["dt_us"][stale] == got[0][0]["dt_us"][stale]).all()
    chain = bank_chain(aof, eng, gpu_device, torch.from_numpy(crop_of(frames, 64, 64)).to(gpu_device), d_times, rate, imu_feed=(samples, sample_end))
    assert (chain[0]["quality"] == imu.STALE_GYRO).sum() == stale.sum()
    same_as_the_bank(got[1], chain, n)
    eng.close()


# ---- 4. one captured graph ---------------------------------------------------------------------------------------------------------------
def test_one_captured_graph_of_both_calls_replayed_on_changed_frames(aof, synth, gpu_device):
    """One linear graph on one stream: aof_sequence_device, then the field call.  Replayed on other frames it gives what eager
    execution gives for them."""
    import torch
    a, b = dict(ref.E2E["px4-64-rate15"], n=30), dict(ref.E2E["px4-64-rate15"], n=30, seed=11)
    n = 30
    (fa, times), (fb, _) = ref.e2e_recording(synth, a), ref.e2e_recording(synth, b)
    eng = aof.FlowEngine(ref.e2e_params(aof, a), 0)
    sp = aof.sequence_params(160, 120, 64, 64, FX, FY, 15, 0, 1, 100, 0)
    cam, tt = torch.from_numpy(fa).to(gpu_device), torch.from_numpy(times).to(gpu_device)
    o = Outputs(gpu_device, n)

    def both(ws=None):
        ws, L = eng.sequence(sp, cam, tt, workspace=ws)
        assert rig.device(aof, eng, sp, n, ws, o.fields.tensor, o.out.tensor, o.state.tensor) == 0
        return ws, L

    def result(ws, L):
        torch.cuda.synchronize()
        seq = eng.sequence_outputs(sp, ws, L, n)
        return (seq["records"].tobytes(),) + tuple(x.tobytes() for x in o.read(aof, len(seq["records"])))

    eager = []
    for f in (fa, fb):
        cam.copy_(torch.from_numpy(f).to(gpu_device))
        eager.append(result(*both()))
    assert eager[0][1:] != eager[1][1:]
    ws, L = both()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both(ws)
    for i, f in enumerate((fa, fb, fa)):
        cam.copy_(torch.from_numpy(f).to(gpu_device))
        ws.zero_()
        for x in (o.fields, o.out, o.state):
            x.refill()
        g.replay()
        assert result(ws, L) == eager[i % 2], ("replay", i)
    eng.close()
