"""aof_sequence_mavlink_rx_device (include/aof_sequence_mavlink_rx.h) on the device: against aof_sequence_mavlink_rx_host byte
for byte -- the samples up to the written count, all of sample_end, the 128 state bytes, the sentinels behind the written
samples and in the guards around every output and the scratch -- on the family of designed logs (tests/sequence_rx_ref.py:
every size, seam, chain, chunk count, capacity, byte_end and frame count edge); without a state; end to end in front of
aof_sequence_device and aof_sequence_imu_device against the same chain fed the host function's arrays; from a captured graph
replayed on other bytes; and the refusals.  A byte_end in no order, with values far above N, is one of the family's cases: the
kernels clamp it (k_seq_rx_sample_end: q = min(byte_end, N), the chunk index below the chunk count, the list length to 512),
and each k is compared with the host all the same.  The DEEP family (sequence_rx_ref.deep_cases) holds the same call where a chunk
fills its list of 512, a workgroup's lanes take a second trip, the scan has two levels and a graph nine entry rounds; three logs of
268 MB on one upload hold three scan levels and 17 rounds, against the host function and against the tile rule.  No tolerance
anywhere."""
import ctypes as C

import numpy as np
import pytest

import sequence_imu_rig as imu_rig
import sequence_rx_ref as ref
import sequence_rx_rig as rig
from bank_rig import FILL, GUARD, Guarded, time_limit   # noqa: F401  (time_limit: this module's autouse fixture too)

pytestmark = pytest.mark.gpu

CASES = ref.cases()
DEEP = ref.deep_names()
FX, FY = 216.6677, 216.2457


@pytest.fixture(scope="module")
def small(aof, gpu_device):
    """The smallest frame the engine takes."""
    p = aof.default_params(16, 16)
    eng = aof.FlowEngine(p, 0)
    yield eng, p
    eng.close()


class Rx:
    """The device buffers of one call shape (N bytes, n frames, max_samples slots): the log with decoy start bytes behind N up
    to the next multiple of 16, guarded outputs, and the scratch at its exact size between guard bytes.  log: the loaded log
    buffer of another Rx whose first N bytes this one reads (arm() in place of load())."""

    def __init__(self, aof, eng, gpu_device, N, n, max_samples, log=None):
        import torch
        self.aof, self.eng, self.dev, self.torch, self.N, self.n, self.M = aof, eng, gpu_device, torch, N, n, max_samples
        self.log = torch.full((max((N + 15) // 16 * 16, 16),), 0xFD, dtype=torch.uint8, device=gpu_device) if log is None else log
        assert self.log.numel() >= N
        self.byte_end = torch.zeros(max(n, 1), dtype=torch.int32, device=gpu_device)
        self.samples = Guarded(gpu_device, (max_samples, 24))
        self.sample_end = Guarded(gpu_device, (max(n, 1), 4))
        self.state = Guarded(gpu_device, (128,))
        self.scratch_bytes = rig.scratch_bytes(aof, N)
        assert self.scratch_bytes > 0 and self.scratch_bytes % 256 == 0
        self.scratch_alloc = torch.full((self.scratch_bytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=gpu_device)
        self.scratch = self.scratch_alloc[GUARD:GUARD + self.scratch_bytes]
        assert self.scratch.data_ptr() % 256 == 0 and self.log.data_ptr() % 16 == 0

    def load(self, log, byte_end):
        torch = self.torch
        assert len(log) == self.N
        self.log.fill_(0xFD)
        if self.N:
            self.log[:self.N].copy_(rig.up(torch, log, self.dev))
        self.arm(byte_end)

    def arm(self, byte_end):
        """byte_end up, every output refilled."""
        torch = self.torch
        assert len(byte_end) == self.n
        if self.n:
            self.byte_end.copy_(rig.up(torch, np.asarray(byte_end, np.uint32), self.dev).view(torch.int32))
        for g in (self.samples, self.sample_end, self.state):
            g.refill()

    def run(self, state=True):
        with_frames = self.n > 0
        return rig.device(self.aof, self.eng, rig.params(self.N, self.M), self.n, self.log if self.N else None,
                          self.byte_end if with_frames else None, self.samples.tensor, self.sample_end.tensor if with_frames else None,
                          self.state.tensor if state else None, self.scratch)

    def same_as_host(self, log, byte_end, what, state=True):
        """Every output against the host function's, sentinels included."""
        self.torch.cuda.synchronize()
        want_samples, want_end, want_state = rig.run_host(self.aof, log, byte_end, self.M, FILL)
        total = int(np.frombuffer(want_state.tobytes(), ref.STATE_DTYPE)["imu_samples"][0])
        written = min(total, self.M)
        got = self.samples.read(used=written * 24)            # (asserts the fill behind the written samples and in the guards)
        assert got.tobytes() == want_samples[:written].tobytes(), (what, "samples")
        got_end = self.sample_end.read(used=self.n * 4)
        assert got_end.tobytes() == want_end.tobytes(), (what, "sample_end", got_end.view(np.uint32)[:8], want_end[:8])
        if state:
            assert self.state.read().tobytes() == want_state.tobytes(), (what, "state", self.state.read()[:64], want_state[:64])
        else:
            assert (self.state.read() == FILL).all(), (what, "no state was asked for")
        guards = self.scratch_alloc.cpu().numpy()
        assert (guards[:GUARD] == FILL).all() and (guards[GUARD + self.scratch_bytes:] == FILL).all(), (what, "bytes around the scratch")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_device_call_equals_the_host_function(aof, small, gpu_device, case):
    eng, _ = small
    rx = Rx(aof, eng, gpu_device, len(case["log"]), len(case["byte_end"]), case["max_samples"])
    rx.load(case["log"], case["byte_end"])
    assert rx.run() == 0
    rx.same_as_host(case["log"], case["byte_end"], case["name"])


@pytest.mark.parametrize("name", DEEP)
def test_the_device_call_equals_the_host_function_on_the_deep_family(aof, small, gpu_device, name):
    eng, _ = small
    case = ref.deep_case(name)
    rx = Rx(aof, eng, gpu_device, len(case["log"]), len(case["byte_end"]), case["max_samples"])
    rx.load(case["log"], case["byte_end"])
    assert rx.run() == 0
    rx.same_as_host(case["log"], case["byte_end"], name)


def same_as_expected(rx, want, what):
    """The outputs of a call against an expectation of the reference module (the sentinels are same_as_host's business)."""
    written = len(want["samples"])
    assert written == min(want["total"], rx.M)
    assert rx.samples.read(used=written * 24).tobytes() == want["samples"].tobytes(), (what, "samples")
    assert rx.sample_end.read(used=rx.n * 4).tobytes() == want["sample_end"].tobytes(), (what, "sample_end")
    assert rx.state.read().tobytes() == want["state"], (what, "state")


def test_three_scan_levels_equal_the_host_function(aof, small, gpu_device):
    """One upload of 268 MB; N = 65 537 C - 1 234 (three levels, 17 rounds, the last chunk alone in the top level's second entry),
    N = 65 536 C (two levels, every group full, 16 rounds) and N = 65 538 C - 1 234 (the last pass reads the top level's second
    entry) on its first bytes, each with outputs and a scratch of its own that no call wrote before.  Wall time: LAB_LOG.md."""
    import torch
    eng, _ = small
    names = list(ref.BIG)
    cases = [ref.deep_case(name) for name in names]
    whole = max(cases, key=lambda c: len(c["log"]))
    first = Rx(aof, eng, gpu_device, len(whole["log"]), len(whole["byte_end"]), whole["max_samples"])
    first.load(whole["log"], whole["byte_end"])
    for name, case in zip(names, cases):
        rx = first if case is whole else Rx(aof, eng, gpu_device, len(case["log"]), len(case["byte_end"]), case["max_samples"], log=first.log)
        rx.arm(case["byte_end"])
        assert rx.run() == 0
        rx.same_as_host(case["log"], case["byte_end"], name)
        same_as_expected(rx, case["want"], name)
        if rx is not first:
            del rx
            torch.cuda.empty_cache()
    del first
    torch.cuda.empty_cache()


def test_without_a_state_only_samples_and_sample_end_are_written(aof, small, gpu_device):
    eng, _ = small
    case = next(c for c in CASES if c["name"] == "3 chunks")
    rx = Rx(aof, eng, gpu_device, len(case["log"]), len(case["byte_end"]), case["max_samples"])
    rx.load(case["log"], case["byte_end"])
    assert rx.run(state=False) == 0
    rx.same_as_host(case["log"], case["byte_end"], "no state", state=False)


def test_one_captured_graph_replayed_twice_on_other_bytes(aof, small, gpu_device):
    import torch
    eng, _ = small
    rng = np.random.default_rng(11)
    N = 3 * ref.C + 123
    logs = [ref.mixed(rng, N), ref.healthy(rng, N + 300)[:N]]
    ends = [np.sort(rng.integers(0, N + 50, 70)).astype(np.uint32), np.linspace(0, N, 70).astype(np.uint32)]
    rx = Rx(aof, eng, gpu_device, N, 70, 40)
    rx.load(logs[0], ends[0])
    assert rx.run() == 0                      # (eager once: everything the launches need exists before the capture)
    rx.same_as_host(logs[0], ends[0], "eager")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert rx.run() == 0
    for i in (1, 0):
        rx.load(logs[i], ends[i])
        rx.scratch.fill_(FILL)
        g.replay()
        rx.same_as_host(logs[i], ends[i], ("replay", i))


def test_one_captured_graph_of_nine_entry_rounds_and_two_scan_levels_replayed_on_other_bytes(aof, small, gpu_device):
    import torch
    eng, _ = small
    case = ref.deep_case("257 chunks")
    N, n, M = len(case["log"]), len(case["byte_end"]), case["max_samples"]
    assert ref.plan(N)["rounds"] == 9 and len(ref.plan(N)["scan_entries"]) == 2
    other = np.frombuffer(ref.healthy(np.random.default_rng(12), N + 300, start=3)[:N], np.uint8)
    logs, ends = [case["log"], other], [case["byte_end"], case["byte_end"][::-1].copy()]
    rx = Rx(aof, eng, gpu_device, N, n, M)
    rx.load(logs[0], ends[0])
    assert rx.run() == 0                      # (eager once: everything the launches need exists before the capture)
    rx.same_as_host(logs[0], ends[0], "eager")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert rx.run() == 0
    for i in (1, 0):
        rx.load(logs[i], ends[i])
        rx.scratch.fill_(FILL)
        g.replay()
        rx.same_as_host(logs[i], ends[i], ("replay", i))


def test_refused_calls_write_nothing(aof, small, gpu_device):
    import torch
    eng, _ = small
    case = next(c for c in CASES if c["name"] == "2 chunks")
    N, n, M = len(case["log"]), len(case["byte_end"]), case["max_samples"]
    rx = Rx(aof, eng, gpu_device, N, n, M)
    rx.load(case["log"], case["byte_end"])
    call = rig.bind(aof).aof_sequence_mavlink_rx_device
    stream = torch.cuda.current_stream().cuda_stream
    before = rx.scratch_alloc.clone()

    def args(**kw):
        rp = rig.params(kw.get("N", N), kw.get("M", M))
        return [kw.get("ctx", eng._ctx), None if kw.get("rp", 1) is None else C.byref(rp), kw.get("n", n), kw.get("log", rx.log.data_ptr()),
                kw.get("byte_end", rx.byte_end.data_ptr()), kw.get("samples", rx.samples.tensor.data_ptr()),
                kw.get("sample_end", rx.sample_end.tensor.data_ptr()), kw.get("state", rx.state.tensor.data_ptr()),
                kw.get("scratch", rx.scratch.data_ptr()), kw.get("bytes", rx.scratch_bytes), stream]

    refused = [dict(ctx=None), dict(rp=None), dict(samples=None), dict(scratch=None), dict(log=None), dict(byte_end=None),
               dict(sample_end=None), dict(N=-1), dict(N=1 << 31), dict(M=0), dict(M=1 << 31), dict(n=-1), dict(n=0x7FFFFFF0),
               dict(log=rx.log.data_ptr() + 8), dict(samples=rx.samples.tensor.data_ptr() + 4), dict(state=rx.state.tensor.data_ptr() + 4),
               dict(byte_end=rx.byte_end.data_ptr() + 2), dict(sample_end=rx.sample_end.tensor.data_ptr() + 2),
               dict(scratch=rx.scratch.data_ptr() + 128)]
    for kw in refused:
        assert call(*args(**kw)) == rig.EINVAL, kw
    assert b"sequence mavlink rx" in aof.lib.aof_last_error(eng._ctx)
    assert call(*args(bytes=rx.scratch_bytes - 1)) == rig.ENOSPC
    torch.cuda.synchronize()
    for g in (rx.samples, rx.sample_end, rx.state):
        assert (g.read() == FILL).all(), "a refused call must leave the outputs untouched"
    assert torch.equal(rx.scratch_alloc, before), "and the scratch"
    # the context is still usable
    assert call(*args()) == 0
    rx.same_as_host(case["log"], case["byte_end"], "after the refusals")


def test_the_call_feeds_the_sequence_imu_call_what_the_host_arrays_feed_it(aof, small, gpu_device):
    """rx -> aof_sequence_device (records only) -> aof_sequence_imu_device with n_samples = max_samples, no host round trip,
    against the same two calls fed the host function's samples and sample_end: the workspace outside the IMU call's own
    scratch and the final IMU state."""
    import torch
    eng, p = small
    rng = np.random.default_rng(5)
    n, M = 40, 200
    times = (np.arange(n) * 13333).astype(np.int64)
    frames = rng.integers(0, 256, (n, 16, 16), dtype=np.uint8)
    log = np.frombuffer(ref.healthy(rng, 2 * ref.C + 500), np.uint8)
    N = len(log)
    byte_end = np.linspace(300, N, n).astype(np.uint32)
    want_samples, want_end, _ = rig.run_host(aof, log, byte_end, M, 0)
    assert 20 < want_end[-1] < M and want_end[0] >= 1
    sp = aof.sequence_params(16, 16, 16, 16, FX, FY, 15, 0, 1, 100, 0)
    d_frames, d_times = torch.from_numpy(frames).to(gpu_device), torch.from_numpy(times).to(gpu_device)
    ip = imu_rig.params(M, 0, 1, 100, 250)

    rx = Rx(aof, eng, gpu_device, N, n, M)
    rx.load(log, byte_end)
    rx.samples.tensor.zero_()                 # (slots behind the written samples are never read: sample_end <= the written count)
    assert rx.run() == 0
    results = []
    ws, L = eng.sequence(sp, d_frames, d_times)     # (the workspace, once; zeroed for each chain: it is not written everywhere)
    for samples, sample_end in ((rx.samples.tensor, rx.sample_end.tensor.view(torch.int32)),
                                (rig.up(torch, want_samples, gpu_device).view(-1, 24), rig.up(torch, want_end, gpu_device).view(torch.int32))):
        ws.zero_()
        eng.sequence(sp, d_frames, d_times, workspace=ws)
        state = Guarded(gpu_device, (64,))
        assert imu_rig.device(aof, eng, sp, ip, n, d_times, samples, sample_end, ws, state.tensor) == 0
        torch.cuda.synchronize()
        own = (L.scratch, L.scratch + 4 * imu_rig.limiter_slot_bytes(n))
        w = ws.cpu().numpy()
        results.append((w[:own[0]].tobytes(), w[own[1]:].tobytes(), state.read().tobytes(), eng.sequence_outputs(sp, ws, L, n)))
    assert results[0][:3] == results[1][:3]
    assert len(results[0][3]["records"]) >= 2
