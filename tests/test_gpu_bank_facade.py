"""The compositions of OpticalFlowBank (facade/include/flow_bank.hpp) that no feature's own test drives: pushCamera() with
enableImu() and with enableMavlinkRx(), enableCamera() behind the other two enables, and reset() with a mask in the plain,
IMU and receive forms.  Every test holds one object to another object on a path that another file holds to an oracle
(push() with enableImu(): tests/test_gpu_bank_imu.py; the receive path: tests/test_gpu_bank_mavlink_rx.py; pushCamera():
tests/test_gpu_bank_exposure.py), entry by entry on raw bytes.  S = 3 streams of 128 x 128 cropped from 144 x 136 sensor
frames (crop origin 8, 4), 14 ticks at output rate 0: every frame behind a stream's first may publish."""
import numpy as np
import pytest

import mavlink_rx_ref as rx
from bank_ref import FX, FY, make_run
from bank_rig import OFFSET, same, time_limit   # (time_limit: this module's fixture too)
from sequence_ref import crop_of

pytestmark = pytest.mark.gpu

S, T, M, B = 3, 14, 4, 272
W = H = 128
CW, CH = 144, 136
OFFSET0 = 1_650_000_000_000_000
INTERVAL = 30_000          # the exposure gate opens every second or third frame of a stream
EXPOSURE0, GAIN0 = 1700, 1
HELD_BACK = 25             # bytes of a read's last frame that arrive with the next tick's read


class Feed:
    """One input for every object of this file: sensor frames, their crops, and per tick and stream the IMU samples and
    the bytes that carry the same samples (HIGHRES_IMU in both wire versions, other frames between them; every other
    read ends HELD_BACK bytes before its last frame does)."""

    def __init__(self, synth):
        self.run = run = make_run(synth, CW, CH, S, T, 31, black=False)
        self.crops = np.stack([crop_of(run.frames[k], W, H) for k in range(T)])
        assert self.crops.shape == (T, S, H, W) and (CW // 2 - W // 2, CH // 2 - H // 2) == (8, 4)
        rng = np.random.default_rng(5)
        clock = np.full(S, 5 * 10 ** 8, np.int64)
        pending, i = [b""] * S, 0
        self.samples = [[[] for _ in range(S)] for _ in range(T)]
        self.reads = [[b""] * S for _ in range(T)]
        self.cut = np.zeros((T, S), bool)              # the read of (k, s) ends inside a frame
        for k in range(T):
            for s in range(S):
                n = 0 if (k + 2 * s) % 6 == 5 else 1 + (k + s) % 2      # now and then a tick without a sample
                buf = pending[s]
                for _ in range(n):
                    i += 1
                    clock[s] += int(rng.integers(2000, 3000))
                    x, y, z = (float(v) for v in rng.normal(0, 0.5, 3).astype(np.float32))
                    self.samples[k][s].append((int(clock[s]), x, y, z))
                    if i % 3 == 0:
                        buf += rx.frame_v2(30, rng.integers(0, 256, 28, dtype=np.uint8).tobytes(), seq=i & 255)
                    p = rx.imu_payload(int(clock[s]), x, y, z, rest=9.81)
                    buf += rx.frame_v1(105, p, seq=i & 255) if i % 2 else rx.frame_v2(105, p, seq=i & 255)
                keep = HELD_BACK if n and (k + s) % 2 == 1 else 0
                self.reads[k][s], pending[s] = buf[:len(buf) - keep], buf[len(buf) - keep:]
                self.cut[k, s] = keep > 0
                assert len(self.reads[k][s]) <= B
        # what the bytes hold is what pushImu() is given: every sample, each frame completed by the next tick's read
        for s in range(S):
            sent = b"".join(self.reads[k][s] for k in range(T)) + pending[s]
            assert rx.decode(sent) == [m for k in range(T) for m in self.samples[k][s]], s
        assert self.cut.any(axis=0).all(), "every stream has a frame cut across a tick"

    def garbage_gyro(self, k):
        g = self.run.gyro[k] + np.float32(1.5)
        assert (g != 0).all()
        return g

    def tail(self, k, s):
        """The bytes that complete the frame the read of (k - 1, s) was cut in: they open the read of (k, s)."""
        return self.reads[k][s][:HELD_BACK] if self.cut[k - 1, s] else b""

    def mid_frame(self, k, s):
        """The stream's receive state is inside a frame behind the reads of ticks 0..k."""
        p = rx.Parser()
        p.feed(b"".join(self.reads[j][s] for j in range(k + 1)), M, [])
        return p.phase != "idle"


@pytest.fixture(scope="module")
def feed(synth):
    return Feed(synth)


def new_bank(aof, form, camera=None, rate=0):
    """An object in the plain, "imu" or "rx" form; camera: "first" / "last" = enableCamera() in front of / behind the
    other enables."""
    bank = aof.OpticalFlowBank(FX, FY, rate, W, H, S)
    assert bank.engineOk(), bank.lastError()
    steps = []
    if form in ("imu", "rx"):
        steps.append(lambda: bank.enableImu(M, OFFSET0))
    if form == "rx":
        steps.append(lambda: bank.enableMavlinkRx(B))
    if form == "plain":
        bank.setTimestampOffset(OFFSET)
    enable_camera = lambda: bank.enableCamera(CW, CH, EXPOSURE0, GAIN0, INTERVAL)
    if camera == "first":
        steps.insert(1 if steps else 0, enable_camera)      # (behind enableImu(): enableMavlinkRx() then comes last)
    elif camera == "last":
        steps.append(enable_camera)
    for step in steps:
        assert step() == 0, bank.lastError()
    return bank


def queue(bank, feed, k, form, streams=range(S)):
    """Tick k's samples or bytes into the object's queues."""
    for s in streams:
        if form == "imu":
            for m in feed.samples[k][s]:
                assert bank.pushImu(s, *m) == 0
        elif form == "rx":
            assert bank.pushMavlink(s, feed.reads[k][s]) == 0


def tick(bank, feed, k, camera, gyro=None, queued=None):
    """queued: the form whose tick-k input is queued first.  Returns the published entries."""
    if queued:
        queue(bank, feed, k, queued)
    run = feed.run
    if camera:
        n, entries = bank.pushCamera(run.frames[k], run.times[k], run.active[k], gyro)
    else:
        n, entries = bank.push(feed.crops[k], run.times[k], run.active[k], gyro)
    assert n == len(entries) >= 0, (k, n, bank.lastError())
    return entries


def listed(entries, streams=range(S)):
    """What is compared of an entry: stream, round, the frame up to its length, the record's 48 bytes."""
    return [(int(e["stream"]), int(e["round"]), int(e["mavlink_len"]), e["mavlink"][:int(e["mavlink_len"])].tobytes(),
             e["record"].tobytes()) for e in entries if int(e["stream"]) in streams]


def per_stream(ticks):
    """Published entries per stream over a list of ticks' entries."""
    return np.bincount(np.concatenate([e["stream"] for e in ticks] + [np.zeros(0, np.uint32)]).astype(np.int64), minlength=S)


@pytest.mark.parametrize("form", ["imu", "rx"])
def test_push_camera_in_the_imu_and_receive_forms_equals_push_on_the_crops(aof, gpu_device, feed, form):
    """A: the form and enableCamera(), pushCamera() on sensor frames with a gyro argument of garbage.  B: the form only,
    push() on the crops with gyro NULL.  C: enableCamera() only, for the commands.  A's entries are B's, A's commands C's."""
    a, b, c = new_bank(aof, form, "first"), new_bank(aof, form), new_bank(aof, "plain", "first")
    got, flags = [], []
    for k in range(T):
        ea = tick(a, feed, k, True, feed.garbage_gyro(k), queued=form)
        eb = tick(b, feed, k, False, None, queued=form)
        tick(c, feed, k, True, feed.garbage_gyro(k))
        assert listed(ea) == listed(eb), ("entries", k)
        same(a.exposureCommands(), c.exposureCommands(), ("commands", k))
        got.append(ea)
        flags.append(c.exposureCommands()["flags"].copy())
    flags = np.stack(flags)
    assert per_stream(got).min() >= 4, per_stream(got)
    assert all(e["mavlink_len"].all() for e in got), "every entry of the IMU form carries its frame"
    assert ((flags != 0).sum(0) >= 2).all() and ((flags == 0).sum(0) >= 2).all(), ("due and not-due ticks per stream", flags)
    if form == "rx":        # published behind a tick whose read ended inside a frame: the frame was completed
        assert all(any(feed.cut[k, s] and (got[k + 1]["stream"] == s).any() for k in range(T - 1)) for s in range(S))
    for o in (a, b, c):
        o.close()


def test_enable_camera_behind_imu_and_receive_starts_every_stream_over(aof, gpu_device, feed):
    """P: enableImu(), enableMavlinkRx(), K ticks of push(); then bytes queued for every stream (tick K's read) while its
    receive state is inside a frame; then enableCamera().  Q: a fresh object with all three enables.  Both get ticks
    K+1.. through pushCamera(), and in front of them the bytes that would complete P's half-received frames: to a stream
    that started over they are junk, a receive state that survived would make a sample of them.  P's entries and
    commands are Q's -- the queued bytes, the half-received frame, the IMU state and the bank's streams of P's past are
    gone.  (K = 5 and not 3: stream 2 joins at tick 3, and the census wants an entry of every stream in front of the
    event.)"""
    K = 5
    p, q = new_bank(aof, "rx"), new_bank(aof, "rx", "last")
    before = [tick(p, feed, k, False, queued="rx") for k in range(K)]
    assert per_stream(before).min() >= 1, per_stream(before)
    queue(p, feed, K, "rx")
    crossing = [s for s in range(S) if feed.mid_frame(K - 1, s) and len(rx.decode(feed.reads[K][s])) >= 1]
    assert crossing, "a half-received frame and queued bytes that hold a whole frame, in one stream"
    assert p.enableCamera(CW, CH, EXPOSURE0, GAIN0, INTERVAL) == 0, p.lastError()
    for s in crossing:
        assert len(rx.decode(feed.reads[K - 1][s] + feed.tail(K, s))) == len(rx.decode(feed.reads[K - 1][s])) + 1
        assert p.pushMavlink(s, feed.tail(K, s)) == 0 and q.pushMavlink(s, feed.tail(K, s)) == 0
    after = []
    for k in range(K + 1, T):
        ep = tick(p, feed, k, True, queued="rx")
        eq = tick(q, feed, k, True, queued="rx")
        assert listed(ep) == listed(eq), ("entries", k)
        same(p.exposureCommands(), q.exposureCommands(), ("commands", k))
        after.append(ep)
    assert per_stream(after).min() >= 2, per_stream(after)
    p.close()
    q.close()


@pytest.mark.parametrize("form", ["plain", "imu", "rx"])
def test_a_masked_reset_starts_the_masked_streams_over_and_leaves_the_others_alone(aof, gpu_device, feed, form):
    """Three objects on one input.  In front of tick K, with tick K's samples or bytes already queued for every stream: X
    calls reset([0, 1, 0]), Y reset(NULL), Z nothing.  Stream 1 of X is Y's from K on; streams 0 and 2 of X are Z's over
    the whole run (their queued samples survive X's reset).  The mask is overwritten as soon as reset() returns."""
    K = 8
    x, y, z = (new_bank(aof, form) for _ in range(3))
    gyro = (lambda k: feed.run.gyro[k]) if form == "plain" else (lambda k: None)
    ticks = {}
    for k in range(T):
        for o in (x, y, z):
            queue(o, feed, k, form)
        if k == K:
            mask = np.array([0, 1, 0], np.uint8)
            assert x.reset(mask) == 0 and y.reset(None) == 0
            mask[:] = (1, 0, 1)
        ticks[k] = [tick(o, feed, k, False, gyro(k)) for o in (x, y, z)]
        ex, ey, ez = ticks[k]
        assert listed(ex, (0, 2)) == listed(ez, (0, 2)), ("the streams outside the mask", k)
        if k >= K:
            assert listed(ex, (1,)) == listed(ey, (1,)), ("the masked stream", k)
    # census: every stream published on both sides of the reset; the reset showed (stream 1 of X differs from Z's behind
    # it, streams 0 and 2 of Y from Z's); input queued in front of the reset reached stream 0's tick behind it
    assert per_stream([ticks[k][0] for k in range(K)]).min() >= 1 and per_stream([ticks[k][0] for k in range(K, T)]).min() >= 2
    assert any(listed(ticks[k][0], (1,)) != listed(ticks[k][2], (1,)) for k in range(K, T)), "the reset of stream 1 shows"
    assert any(listed(ticks[k][1], (0, 2)) != listed(ticks[k][2], (0, 2)) for k in range(K, T)), "and Y's of streams 0 and 2"
    if form != "plain":
        assert all(len(feed.samples[K][s]) >= 1 for s in (0, 1)), "a sample queued for streams 0 and 1"
        assert feed.run.active[K, 0] and (ticks[K][0]["stream"] == 0).any(), "stream 0 publishes in tick K: not stale"
    if form == "rx":
        assert len(rx.decode(feed.reads[K][0])) >= 1 and len(rx.decode(feed.reads[K][1])) >= 1
    for o in (x, y, z):
        o.close()
