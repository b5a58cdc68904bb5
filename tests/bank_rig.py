"""What the stream bank's device tests (tests/test_gpu_bank*.py, tests/test_gpu_tail_matrix.py) share: the constants, the
byte comparer, guarded output buffers, the fixtures, the helpers for burstable runs and bound device arrays, and BankRig,
the one device rig behind the four push entry points (aof_bank_push_device, aof_bank_push_camera_device and their burst
forms, include/aof.h).  A test file that wants a fixture imports its name.  The cases built on the rig:
tests/bank_cases.py; the rig whose camera buffer holds per-stream sensor layouts: tests/bank_sensor_rig.py."""
import faulthandler
from collections import namedtuple

import numpy as np
import pytest

EINVAL, ENOSPC, EIO, ENOBUFS = -22, -28, -5, -105
OFFSET = 5_000_000
LIMITED = (3, 10, 5)   # bank_ref's census per stream over 48 ticks at a limited rate: >= 3 published, >= 10 held, >= 5 idle
GATED = (2, 10)        # per stream, 48 ticks at 200 000 us: >= 2 due and >= 10 not-due active frames
SENSOR = {"px4-64": (320, 240), "opencv-128": (640, 480), "dense-192x160": (256, 224), "tile16-160x128": (224, 192)}
FILL, GUARD = 0xEE, 256
LIMIT_S = 120


def params_of(aof, cfg):
    if cfg == "px4-64":          # OpticalFlowPX4 at its default size
        return aof.px4flow_params(64, 64)
    if cfg == "opencv-128":      # what OpticalFlowOpenCV's constructor selects: two levels + equalisation
        return aof.px4flow_params(128, 128, pyramid_levels=2, mean_subtract=1)
    if cfg == "px4-96x80":
        return aof.px4flow_params(96, 80)
    if cfg == "px4-96x80-2":
        return aof.px4flow_params(96, 80, pyramid_levels=2, mean_subtract=1)
    if cfg == "opencv-64":
        return aof.px4flow_params(64, 64, pyramid_levels=2, mean_subtract=1)
    if cfg == "px4-128":
        return aof.px4flow_params(128, 128)
    if cfg == "dense-192x160":   # 22 x 18 = 396 blocks: outside the one-workgroup class
        return aof.default_params(192, 160, subpixel=1)
    if cfg == "tile16-160x128":  # 16x16 tiles, +-8 (the thresholds smoke() uses)
        return aof.default_params(160, 128, tile=16, search=8, value_threshold=12000, min_valid=0)
    raise KeyError(cfg)


def params_for(aof, cfg, overrides=None):
    p = params_of(aof, cfg)
    for k, v in (overrides or {}).items():
        setattr(p, k, int(v))
    return p


# ---- comparers: every comparison is on raw bytes --------------------------------------------------------------------

def same(got, want, what):
    """Two arrays of one shape hold the same bytes; if not, the first differing element of both is reported."""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if g.tobytes() == w.tobytes():
        return
    bad = np.flatnonzero(g.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1))
    i = int(bad[0]) // g.dtype.itemsize
    raise AssertionError((what, "first of", len(bad), "differing bytes at", int(bad[0]), "element", i, g.reshape(-1)[i], w.reshape(-1)[i]))


def same_records(got, want, tick, what, pixel=True):
    """Tick records [S]; pixel=False: every field but the pair's pixel record (the facade does not give it)."""
    if pixel:
        return same(got, want, (what, "tick", tick))
    for n in got.dtype.names:
        if n != "pixel":
            same(got[n], want[n], (what, "tick", tick, n))


def same_exposure(got, want, tick, what):
    same(got, want, (what, "tick", tick))


def untouched(a):
    return (np.asarray(a).view(np.uint8) == FILL).all()


class Guarded:
    """A device buffer of `shape` bytes that kernels write, with GUARD sentinel bytes behind it (and `skew` in front:
    the buffer then starts that many bytes into its allocation).  refill() before a launch; read() copies it to the
    host (synchronising) and asserts that no byte around it was written."""

    def __init__(self, gpu_device, shape, fill=FILL, skew=0):
        import torch
        self.shape, self.size, self.fill, self.skew = tuple(shape), int(np.prod(shape)), fill, skew
        self.alloc = torch.empty(skew + self.size + GUARD, dtype=torch.uint8, device=gpu_device)
        self.tensor = self.alloc[skew:skew + self.size].view(self.shape)
        self.refill()

    def refill(self):
        self.alloc.fill_(FILL)
        if self.fill != FILL:
            self.tensor.fill_(self.fill)

    def read(self, used=None):
        """The buffer as uint8 in its shape, or its first `used` bytes: the rest must then still hold the fill."""
        a = self.alloc.cpu().numpy()
        lo, end = self.skew, self.skew + self.size
        hi = end if used is None else lo + used
        assert (a[:lo] == FILL).all() and (a[end:] == FILL).all(), "bytes in front of or behind the buffer were written"
        assert (a[hi:end] == self.fill).all(), "bytes behind the used part of the buffer were written"
        return a[lo:hi].reshape(self.shape) if used is None else a[lo:hi]


# ---- fixtures -------------------------------------------------------------------------------------------------------

@pytest.fixture(autouse=True)
def time_limit():
    """Every test's device work under a limit of its own.  The exit is deliberate: a step that hangs on the device ends
    the whole process at once (os._exit behind a traceback), so that nothing more is started on a card that hung -- the
    tests behind it go without a report, which is the lesser evil.  Each test runs a few seconds; the limit is far above
    that and only a hang reaches it."""
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def engine(aof, gpu_device):
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    yield eng
    eng.close()


# ---- runs and device arrays ------------------------------------------------------------------------------------------

def up(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def put(t, s, rec):
    """Record s of a bound array, rewritten on the current stream: in order with the ticks around it."""
    t[s].copy_(up(t.device, np.frombuffer(np.asarray(rec).tobytes(), np.uint8).copy()))


def burstable(run, K):
    """The run with every stream's frames of a burst of K rounds moved to nobody: inside rounds [jK, jK + K) a stream
    keeps its leading frames only (aof_bank_burst's count).  The dropped frames are never given to anyone."""
    for k0 in range(0, run.T - run.T % K, K):
        run.active[k0:k0 + K] = run.active[k0:k0 + K].cumprod(axis=0)
    return run


def counts_of(run, K, T=None):
    """count [T // K, S] of a burstable run's bursts of K rounds (T None: the run's ticks)."""
    T = run.T if T is None else T
    a = run.active[:T - T % K].reshape(-1, K, run.S)
    assert (a.cumprod(axis=1).sum(axis=1) == a.sum(axis=1)).all(), "a burst's frames are a stream's first rounds"
    return a.sum(axis=1).astype(np.uint8)


# ---- the rig --------------------------------------------------------------------------------------------------------

Tick = namedtuple("Tick", "recs wire exposure derotated")   # records [S], frames [S] of bytes, exposure records [S], float [S, 2]


class BankRig:
    """One bank and the persistent buffers of its pushes on the device.  K None: a tick through aof_bank_push_device;
    K >= 1: a burst of K rounds through aof_bank_push_burst_device.  camera: (aof_bank_camera, sensor frames) for the
    sensor-frame forms, where sensor frames is an object with cam_w, cam_h and sensor(tick) -> [S, cam_h, cam_w]
    (bank_camera_ref.CameraRun).  skew: the input frames start that many bytes into their allocation (sensor frames need
    no alignment); pad: bytes added to the dense round_stride (0: round_stride is passed as 0).  Every output is a
    Guarded buffer, pre-filled with 0xEE (the wire frames with 0) by load() and checked by read().  bank: the bank of
    another rig to push into (ticks and bursts on one bank) instead of a new one."""

    def __init__(self, aof, eng, run, bp, gpu_device, K=None, camera=None, use_gyro=True, exposure=True, skew=0, pad=0, bank=None):
        import torch
        self.aof, self.eng, self.run, self.K, self.torch = aof, eng, run, K, torch
        self.cam, self.cam_run = camera if camera else (None, None)
        self.bank = bank or eng.bank_create(bp, gpu_device, camera=self.cam)
        S, R = run.S, K or 1
        if self.cam is None:
            self.item = run.frames.shape[2] * run.frames.shape[3]
            self.stride = bp.frame_stride or self.item
        else:
            self.item = self.cam_run.cam_w * self.cam_run.cam_h
            self.stride = self.cam.camera_stride or self.item
        self.round = S * self.stride + pad
        self.round_stride = self.round if pad else 0
        self.alloc = torch.zeros(R * self.round + 64, dtype=torch.uint8, device=gpu_device)
        self.frames = self.alloc[skew:skew + R * self.round]     # stream s of round k at k * round + s * stride
        lead = (S,) if K is None else (K, S)
        self.times = torch.zeros(lead, dtype=torch.int64, device=gpu_device)
        self.select = torch.zeros(S, dtype=torch.uint8, device=gpu_device)     # `active` of a tick, `count` of a burst
        self.gyro = torch.zeros(lead + (4,), dtype=torch.float32, device=gpu_device) if use_gyro else None
        self.outputs = [Guarded(gpu_device, lead + (48,)), Guarded(gpu_device, lead + (56,), fill=0), Guarded(gpu_device, lead),
                        Guarded(gpu_device, lead + (48,)), Guarded(gpu_device, lead + (8,))]
        self.records, self.wire, self.lens, self.exposure, self.derotated = (g.tensor for g in self.outputs)
        self.want_exposure = exposure

    def load(self, k, given=None, sensors=None, **fill):
        """A tick: tick k of the run; sensors: its sensor frames [S, cam_h, cam_w], else the camera run's.  A burst:
        burst k, the run's ticks k * K .. k * K + K - 1; given [B, S]: the counts the device is told; sensors: a list
        of K.  Every output is refilled (every record of every round must be written).  fill: what a subclass's
        fill_frames takes."""
        t, run, R = self.torch, self.run, self.K or 1
        self.fill_frames(k, sensors, **fill)
        ticks = slice(k * R, (k + 1) * R)
        self.times.copy_(t.from_numpy(run.times[ticks]).view(self.times.shape))
        self.select.copy_(t.from_numpy(run.active[k] if self.K is None else given[k]))
        if self.gyro is not None:
            self.gyro.copy_(t.from_numpy(run.gyro[ticks]).view(self.gyro.shape))
        for g in self.outputs:
            g.refill()

    def fill_frames(self, k, sensors=None):
        """The frame buffer of tick or burst k: every round's S frames, dense at the rig's strides."""
        t, run, S, R = self.torch, self.run, self.run.S, self.K or 1
        if self.K is None and sensors is not None:
            sensors = [sensors]
        for r in range(R):
            tick = k * R + r
            if self.cam is None:
                data = run.frames[tick]
            else:
                data = sensors[r] if sensors is not None else self.cam_run.sensor(tick)
            dst = self.frames[r * self.round:r * self.round + S * self.stride].view(S, self.stride)
            dst[:, :self.item].copy_(t.from_numpy(np.ascontiguousarray(data.reshape(S, -1))))

    def enqueue(self, all_rounds=False):
        """The push of what load() left; all_rounds: d_active / d_count is NULL."""
        select = None if all_rounds else self.select
        kw = dict(mavlink=True, records=self.records, out_frames=self.wire, out_lengths=self.lens)
        if self.cam is not None:
            kw.update(exposure=self.exposure if self.want_exposure else None, derotated=self.derotated, want_exposure=self.want_exposure)
        if self.K is None:
            push = self.eng.bank_push if self.cam is None else self.eng.bank_push_camera
            push(self.bank, self.frames, self.times, select, self.gyro, **kw)
        else:
            push = self.eng.bank_push_burst if self.cam is None else self.eng.bank_push_camera_burst
            push(self.bank, self.K, self.frames, self.times, select, self.gyro, round_stride=self.round_stride, **kw)

    def read(self):
        """Host copies as a Tick; of a burst: one Tick per round."""
        self.torch.cuda.synchronize()
        S, R = self.run.S, self.K or 1
        r, w, n, e, d = (g.read().reshape(R, S, -1) for g in self.outputs)
        n = n.reshape(R, S)
        ticks = [Tick(r[k].view(self.aof.TICK_DTYPE).reshape(S), [bytes(w[k, s, :n[k, s]]) for s in range(S)],
                      e[k].view(self.aof.EXPOSURE_DTYPE).reshape(S), d[k].view(np.float32)) for k in range(R)]
        return ticks[0] if self.K is None else ticks

    def push(self, k, given=None, sensors=None):
        self.load(k, given, sensors)
        self.enqueue()
        return self.read()

    def raw(self):
        """Every output buffer as bytes (for comparisons between two rigs)."""
        self.torch.cuda.synchronize()
        return b"".join(g.read().tobytes() for g in self.outputs)

    def bank_bytes(self):
        return self.bank.frames_bytes().tobytes() + self.bank.state_bytes().tobytes()

    def gate_bytes(self):
        """next_exposure_us of every stream: the last 8 bytes of its state record."""
        return np.ascontiguousarray(self.bank.state_bytes()[:, 56:64]).view("<u8").reshape(-1)
