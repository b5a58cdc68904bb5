"""aof_sequence_imu_device (include/aof_sequence_imu.h) on the device: against aof_sequence_imu_host byte for byte over the
whole workspace and the final state on fabricated records (no flow is run: records, count words and lengths are written at
the layout's offsets of a sentinel-filled workspace) at every edge of the record pass, of the scan over its workgroup counts
and of the sample pass; end to end behind aof_sequence_device against a one-stream bank pushed frame by frame with
aof_bank_imu_device behind every push; from a captured graph; the refusals; and a decreasing sample_end, which must stay
inside every array.  The four limiter buffers at the start of the scratch region are the call's own (the contract lends
them); every other byte of the workspace is compared.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import imu_ref as imu
import sequence_imu_ref as ref
import sequence_imu_rig as rig
from bank_rig import GUARD, Guarded, time_limit   # noqa: F401  (time_limit: this module's autouse fixture too)
from sequence_ref import crop_of

pytestmark = pytest.mark.gpu

FX, FY = 216.6677, 216.2457
FILL = 0xEE
RECORD_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 513, 65535, 65536, 65537)
SAMPLE_COUNTS = (0, 1, 63, 64, 65, 40003)


@pytest.fixture(scope="module")
def small(aof, gpu_device):
    """The smallest frame the engine takes: the workspace of 65 537 frames stays at 29 MB."""
    p = aof.default_params(16, 16)
    eng = aof.FlowEngine(p, 0)
    yield eng, p, aof.sequence_params(16, 16, 16, 16, FX, FY, 15, 0, ref.SYSTEM_ID, ref.COMPONENT_ID, 0)
    eng.close()


class Fabricated:
    """A sentinel-filled workspace for n frames with M fabricated records, on the device with guard bytes around it, and what
    the host function makes of the same bytes."""

    def __init__(self, aof, eng, p, sp, gpu_device, n):
        import torch
        self.aof, self.eng, self.sp, self.dev, self.torch, self.n = aof, eng, sp, gpu_device, torch, n
        self.L = L = aof.sequence_layout(p, sp, n)
        self.alloc = torch.empty(L.total_bytes + 2 * GUARD, dtype=torch.uint8, device=gpu_device)
        self.ws = self.alloc[GUARD:GUARD + L.total_bytes]
        assert self.ws.data_ptr() % 256 == 0
        self.state_buf = Guarded(gpu_device, (64,))
        self.own = (L.scratch, L.scratch + 4 * rig.limiter_slot_bytes(n))    # the limiter's buffers: the call's scratch

    def load(self, r):
        """The workspace as the sequence call would leave it for recording r (sentinel where it matters to nobody)."""
        torch, L, n = self.torch, self.L, self.n
        assert r["n"] == n
        self.alloc.fill_(FILL)
        self.state_buf.refill()
        self.count = np.array([r["M"], 0xEEEEEEEE, 0x77, 0x55], np.uint32)
        self.lengths = np.full(n, FILL, np.uint8)
        self.lengths[:r["M"]] = 0
        self.put(L.count, self.count)
        self.put(L.records, r["records"])
        self.put(L.frame_len, self.lengths)
        self.ws[L.frames:L.frames + 56 * n].fill_(ref.SENTINEL)
        self.before = self.alloc.clone()
        self.times = rig.up(torch, r["times"], self.dev).view(torch.int64)
        self.samples = rig.up(torch, r["samples"], self.dev).view(-1, 24) if len(r["samples"]) else None
        self.sample_end = rig.up(torch, r["sample_end"], self.dev).view(torch.int32)

    def put(self, offset, a, alloc=None):
        t = rig.up(self.torch, a, self.dev)
        (self.alloc if alloc is None else alloc)[GUARD + offset:GUARD + offset + t.numel()].copy_(t)

    def run(self, r, state=True):
        ip = rig.params(len(r["samples"]), r["offset0"], ref.SYSTEM_ID, ref.COMPONENT_ID, r["first_seq"])
        return rig.device(self.aof, self.eng, self.sp, ip, self.n, self.times, self.samples, self.sample_end, self.ws,
                          self.state_buf.tensor if state else None)

    def expected(self, r):
        """self.before with the host function's outputs in place -> (device tensor, state bytes)."""
        n, L = self.n, self.L
        records, count = r["records"].copy(), self.count.copy()
        frames, lengths = np.full((n, 56), ref.SENTINEL, np.uint8), self.lengths.copy()
        state = np.full(64, FILL, np.uint8).view(ref.STATE_DTYPE)
        ip = rig.params(len(r["samples"]), r["offset0"], ref.SYSTEM_ID, ref.COMPONENT_ID, r["first_seq"])
        assert rig.host(self.aof, ip, n, r["times"], r["samples"], r["sample_end"], records, count, frames, lengths, state) == 0
        want = self.before.clone()
        for offset, a in ((L.count, count), (L.records, records), (L.frames, frames), (L.frame_len, lengths)):
            self.put(offset, a, want)
        return want, state, int(count[1])

    def same_outside_the_scratch(self, want, what):
        torch = self.torch
        lo, hi = GUARD + self.own[0], GUARD + self.own[1]
        for a, b, part in ((self.alloc[:lo], want[:lo], "in front of the scratch"), (self.alloc[hi:], want[hi:], "behind the limiter's buffers")):
            if not torch.equal(a, b):
                at = int(torch.nonzero(a != b)[0])
                raise AssertionError((what, part, "first differing byte at", at - (GUARD if part[0] == "i" else -hi + GUARD),
                                      int(a[at]), int(b[at]), "layout", {f: getattr(self.L, f) for f, _ in self.L._fields_}))


@pytest.mark.parametrize("M", RECORD_COUNTS)
def test_the_kernels_equal_the_host_function_on_fabricated_records(aof, small, gpu_device, M):
    """Every record count with every sample count, every sample design and both offset forms; first_seq 250."""
    import torch
    eng, p, sp = small
    n = M if M >= 65535 else M + 2        # (65 535 / 65 536 frames: 256 / 257 workgroup counts, the edge of the scan's second level)
    fab = Fabricated(aof, eng, p, sp, gpu_device, n)
    sent = 0
    for T in SAMPLE_COUNTS:
        for design in ref.DESIGNS:
            for offset0 in (0, ref.PRESET):
                r = ref.designed(M, n, T, design, offset0, seed=M)
                assert r["first_seq"] == 250
                fab.load(r)
                assert fab.run(r) == 0
                want, state, frames_sent = fab.expected(r)
                torch.cuda.synchronize()
                fab.same_outside_the_scratch(want, r["name"])
                assert fab.state_buf.read().tobytes() == state.tobytes(), (r["name"], "final state")
                sent += frames_sent
    assert sent > 0 or M == 1


def test_without_a_state_nothing_but_the_workspace_is_written(aof, small, gpu_device):
    import torch
    eng, p, sp = small
    r = ref.designed(257, 300, 4000, "edges", 0, seed=5)
    fab = Fabricated(aof, eng, p, sp, gpu_device, 300)
    fab.load(r)
    assert fab.run(r, state=False) == 0
    want, _, sent = fab.expected(r)
    torch.cuda.synchronize()
    fab.same_outside_the_scratch(want, "no state")
    assert sent > 10 and (fab.state_buf.read() == FILL).all()


def test_a_decreasing_sample_end_stays_inside_every_array(aof, small, gpu_device):
    """The device call cannot see the array; its kernels clamp.  Only that it completes, that nothing around an output was
    written and that no more frames are counted than records."""
    import torch
    eng, p, sp = small
    M, n, T = 600, 640, 3000
    for seed, design in enumerate(("steady", "duplicates")):
        r = ref.designed(M, n, T, design, 0, seed=seed)
        rng = np.random.default_rng(seed)
        r["sample_end"] = rng.integers(0, 2 * T, n).astype(np.uint32)       # no order at all, values above T among them
        r["sample_end"][::7] = 0xFFFFFFFF
        r["records"]["frame"][5] = 0xFFFFFFF0                                # and a frame index far behind the recording
        fab = Fabricated(aof, eng, p, sp, gpu_device, n)
        fab.load(r)
        assert fab.run(r) == 0
        torch.cuda.synchronize()
        got = fab.alloc.cpu().numpy()
        before = fab.before.cpu().numpy()
        L = fab.L
        written = [(L.count + 4, 4), (L.records, 32 * M), (L.frames, 56 * M), (L.frame_len, M), (fab.own[0], fab.own[1] - fab.own[0])]
        keep = np.ones(got.size, bool)
        for offset, size in written:
            keep[GUARD + offset:GUARD + offset + size] = False
        assert (got[keep] == before[keep]).all(), "a byte outside the call's outputs was written"
        fab.state_buf.read()                                                 # (asserts its guard bytes)
        count = got[GUARD + L.count:GUARD + L.count + 16].view(np.uint32)
        assert count[0] == M and count[1] <= count[0]
        rec = got[GUARD + L.records:GUARD + L.records + 32 * n].view(ref.RECORD_DTYPE)
        for name in ("frame", "dt_us", "flow_x", "flow_y"):
            assert rec[name].tobytes() == r["records"][name].tobytes(), name


def test_refused_calls_write_nothing(aof, small, gpu_device):
    import torch
    eng, p, sp = small
    n = 40
    r = ref.designed(30, n, 500, "steady", 0, seed=3)
    fab = Fabricated(aof, eng, p, sp, gpu_device, n)
    fab.load(r)
    call = rig.bind(aof).aof_sequence_imu_device
    stream = torch.cuda.current_stream().cuda_stream
    with_offset = aof.sequence_params(16, 16, 16, 16, FX, FY, 15, 5_000_000, 1, 100, 0)
    derotate = aof.sequence_params(16, 16, 16, 16, FX, FY, 15, 0, 1, 100, 0, derotate=(4.5, 0.01))
    other_crop = aof.sequence_params(32, 32, 24, 24, FX, FY, 15, 0, 1, 100, 0)

    def args(**kw):
        ip = rig.params(kw.get("T", 500), 0, 1, 100, 250)
        return [kw.get("ctx", eng._ctx), None if kw.get("sp", sp) is None else C.byref(kw.get("sp", sp)),
                None if kw.get("ip", 1) is None else C.byref(ip), kw.get("n", n), kw.get("times", fab.times.data_ptr()),
                kw.get("samples", fab.samples.data_ptr()), kw.get("end", fab.sample_end.data_ptr()), kw.get("ws", fab.ws.data_ptr()),
                kw.get("bytes", fab.L.total_bytes), kw.get("state", fab.state_buf.tensor.data_ptr()), stream]

    refused = [dict(ctx=None), dict(sp=None), dict(ip=None), dict(times=None), dict(end=None), dict(ws=None), dict(samples=None),
               dict(T=-1), dict(T=1 << 32), dict(n=-1), dict(n=0x7FFFFFF0), dict(sp=other_crop), dict(ws=fab.ws.data_ptr() + 16),
               dict(sp=with_offset), dict(sp=derotate), dict(samples=fab.samples.data_ptr() + 4), dict(times=fab.times.data_ptr() + 4),
               dict(state=fab.state_buf.tensor.data_ptr() + 4), dict(end=fab.sample_end.data_ptr() + 2)]
    for kw in refused:
        assert call(*args(**kw)) == rig.EINVAL, kw
    assert b"sequence imu" in aof.lib.aof_last_error(eng._ctx)
    assert call(*args(bytes=fab.L.total_bytes - 1)) == rig.ENOSPC
    torch.cuda.synchronize()
    assert torch.equal(fab.alloc, fab.before), "a refused call must leave the workspace untouched"
    assert (fab.state_buf.read() == FILL).all()
    assert call(*args(n=0)) == 0, "no frames: nothing to do"
    torch.cuda.synchronize()
    assert torch.equal(fab.alloc, fab.before)
    # the context is still usable
    assert call(*args()) == 0
    want, state, _ = fab.expected(r)
    torch.cuda.synchronize()
    fab.same_outside_the_scratch(want, "after the refusals")
    assert fab.state_buf.read().tobytes() == state.tobytes()


# ---- end to end: aof_sequence_device + the IMU call against a one-stream bank pushed frame by frame ----

def flight_samples(rng, times, first_at=-30000, gap_frames=(), silent_frames=()):
    """HIGHRES_IMU at 250 Hz over the recording (times: the frames' own, microseconds from the first frame; the vehicle's
    clock runs 7 s ahead), with designed gaps: around gap_frames the autopilot is silent for 60 ms, between silent_frames
    (a, b) nothing arrives at all.  Returns (samples SAMPLE_DTYPE [T], sample_end [n])."""
    base = 7_000_000
    t, out = first_at, []
    end_time = int(times[-1]) + 20000
    gaps = {int(times[k]) for k in gap_frames}
    while t < end_time:
        step = int(rng.integers(3900, 4100))
        if any(t <= g < t + step for g in gaps):
            step += 60000
        t += step
        if any(int(times[a]) < t <= int(times[b]) for a, b in silent_frames):
            continue
        out.append((base + t,) + tuple(float(v) for v in rng.normal(0, 0.8, 3).astype(np.float32)))
    a = np.zeros(len(out), imu.SAMPLE_DTYPE)
    for i, s in enumerate(out):
        a[i] = s + (0,)
    arrival = a["time_usec"].astype(np.int64) - base
    return a, np.searchsorted(arrival, times, side="left").astype(np.uint32)


E2E = [dict(cls="px4", crop=(64, 64), cam=(160, 120), n=90, rate=15, seed=3),
       dict(cls="px4", crop=(64, 64), cam=(160, 120), n=40, rate=0, seed=5),
       dict(cls="opencv", crop=(128, 128), cam=(320, 240), n=75, rate=15, seed=4)]


@pytest.mark.parametrize("case", E2E, ids=lambda c: f"{c['cls']}-{c['crop'][0]}-rate{c['rate']}-n{c['n']}")
@pytest.mark.parametrize("offset0", [0, ref.PRESET], ids=["learnt", "preset"])
def test_sequence_and_imu_call_equal_a_one_stream_bank_pushed_frame_by_frame(aof, synth, gpu_device, case, offset0):
    import torch
    cw, ch = case["crop"]
    cam_w, cam_h = case["cam"]
    n, rate = case["n"], case["rate"]
    rng = np.random.default_rng(100 + case["seed"])
    times = np.cumsum(np.concatenate([[0], rng.integers(9000, 18000, n - 1)])).astype(np.int64)   # ~75 fps with jitter
    frames, _ = synth.make_sequence(cam_w, cam_h, n, 4, seed=case["seed"], max_step=3)
    # the first sample after frame 0 for the learnt form (frame 0 stale before any sample), before it for the preset one
    samples, sample_end = flight_samples(rng, times, first_at=2000 if offset0 == 0 else -30000, gap_frames=(n // 3,),
                                         silent_frames=((n // 2, n // 2 + (12 if rate else 2)),))
    p = aof.px4flow_params(cw, ch) if case["cls"] == "px4" else aof.px4flow_params(cw, ch, pyramid_levels=2, mean_subtract=1)
    eng = aof.FlowEngine(p, 0)
    first_seq = 250

    # ---- the sequence pipeline: two calls ----
    sp = aof.sequence_params(cam_w, cam_h, cw, ch, FX, FY, rate, 0, 1, 100, 0)
    d_times = torch.from_numpy(times).to(gpu_device)
    d_samples = rig.up(torch, samples, gpu_device).view(-1, 24)
    d_end = rig.up(torch, sample_end, gpu_device).view(torch.int32)
    state = Guarded(gpu_device, (64,))
    ws, L = eng.sequence(sp, torch.from_numpy(frames).to(gpu_device), d_times)
    ip = rig.params(len(samples), offset0, 1, 100, first_seq)
    assert rig.device(aof, eng, sp, ip, n, d_times, d_samples, d_end, ws, state.tensor) == 0
    torch.cuda.synchronize()
    out = eng.sequence_outputs(sp, ws, L, n)
    assert out["status"] == 0

    # ---- a bank of one stream, a tick per frame, the IMU call behind every push ----
    bank = eng.bank_create(aof.bank_params(1, FX, FY, rate, 0, 1, 100, 0), gpu_device)
    bstate = torch.zeros((1, 64), dtype=torch.uint8, device=gpu_device)
    eng.bank_imu_reset(bstate, offset0=offset0)
    cropped = torch.from_numpy(crop_of(frames, cw, ch)).to(gpu_device)
    per_frame = np.diff(np.concatenate([[0], sample_end.astype(np.int64)]))
    slots = int(per_frame.max())
    assert 1 <= slots <= 16
    ticks, wires, lens = [], [], []
    for k in range(n):
        chunk = np.zeros((slots, 1), imu.SAMPLE_DTYPE)
        lo = int(sample_end[k]) - int(per_frame[k])
        chunk[:per_frame[k], 0] = samples[lo:lo + per_frame[k]]
        records = eng.bank_push(bank, cropped[k:k + 1], d_times[k:k + 1])
        rec, wire, length = eng.bank_imu(rig.up(torch, chunk, gpu_device).view(slots, 1, 24), d_times[k:k + 1], records, bstate,
                                         torch.tensor([int(per_frame[k])], dtype=torch.uint8, device=gpu_device), records_out=records,
                                         first_seq=first_seq)
        ticks.append(rec), wires.append(wire), lens.append(length)
    torch.cuda.synchronize()
    ticks = aof.ticks_view(torch.cat(ticks)).reshape(n)
    wires, lens = torch.cat(wires).cpu().numpy().reshape(n, 56), torch.cat(lens).cpu().numpy().reshape(n)
    published = np.flatnonzero((ticks["quality"] >= 0) | (ticks["quality"] == imu.STALE_GYRO) | (ticks["quality"] == imu.NO_OFFSET))

    got = out["records"]
    assert got["frame"].tolist() == published.tolist() and len(got) >= 2
    for name in ("quality", "dt_us", "flow_x", "flow_y", "gyro_x", "gyro_y", "gyro_z"):
        assert got[name].tobytes() == ticks[name][published].tobytes(), name
    assert [len(f) for f in out["mavlink"]] == lens[published].tolist()
    for m, k in enumerate(published):
        assert out["mavlink"][m] == bytes(wires[k, :lens[k]]), (m, k)
    bank_state = aof.imu_states_view(bstate)
    assert out["frames_sent"] == int(bank_state["messages"][0]) == int((lens > 0).sum()) >= 2
    assert state.read().tobytes() == bank_state.tobytes(), "the final state"
    q = got["quality"]
    assert (q == imu.STALE_GYRO).sum() >= 1 and (q >= 0).sum() >= 2, "the designed gaps must drop a record and leave others"
    assert (q != imu.NO_OFFSET).all()
    eng.close()


def test_one_captured_graph_of_both_calls_replayed_twice_on_changed_samples(aof, synth, gpu_device):
    """One linear graph on one stream: aof_sequence_device, then the IMU call.  Replayed on other samples it gives what eager
    execution gives for them."""
    import torch
    n, cw, ch = 48, 64, 64
    times = (np.arange(n) * 13333).astype(np.int64)
    frames, _ = synth.make_sequence(160, 120, n, 4, seed=21, max_step=3)
    rng = np.random.default_rng(9)
    sa, ea = flight_samples(rng, times, first_at=-20000, silent_frames=((10, 16),))
    sb, eb = flight_samples(rng, times, first_at=3000, gap_frames=(20,))
    T = max(len(sa), len(sb))
    eng = aof.FlowEngine(aof.px4flow_params(cw, ch), 0)
    sp = aof.sequence_params(160, 120, cw, ch, FX, FY, 15, 0, 1, 100, 0)
    cam, tt = torch.from_numpy(frames).to(gpu_device), torch.from_numpy(times).to(gpu_device)
    d_samples = torch.zeros((T, 24), dtype=torch.uint8, device=gpu_device)
    d_end = torch.zeros(n, dtype=torch.int32, device=gpu_device)
    state = torch.zeros(64, dtype=torch.uint8, device=gpu_device)
    ip = rig.params(T, 0, 1, 100, 250)

    def load(samples, end):
        d_samples.zero_()
        d_samples[:len(samples)].copy_(rig.up(torch, samples, gpu_device).view(-1, 24))
        d_end.copy_(rig.up(torch, end, gpu_device).view(torch.int32))     # (sample_end <= len(samples): the zero tail is never taken)

    def both(ws=None):
        ws, L = eng.sequence(sp, cam, tt, workspace=ws)
        assert rig.device(aof, eng, sp, ip, n, tt, d_samples, d_end, ws, state) == 0
        return ws, L

    def result(ws, L):
        torch.cuda.synchronize()
        o = eng.sequence_outputs(sp, ws, L, n)
        return o["records"].tobytes(), o["mavlink"], o["frames_sent"], state.cpu().numpy().tobytes()

    eager = []
    for samples, end in ((sa, ea), (sb, eb)):
        load(samples, end)
        eager.append(result(*both()))
    assert eager[0] != eager[1] and eager[0][2] >= 2 and eager[1][2] >= 2
    ws, L = both()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both(ws)
    for i, (samples, end) in enumerate(((sb, eb), (sa, ea))):
        load(samples, end)
        ws.zero_()
        state.zero_()
        g.replay()
        assert result(ws, L) == eager[1 - i], ("replay", i)
    eng.close()
