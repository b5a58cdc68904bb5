"""The rigs of the packed-pixel GPU tests (tests/test_gpu_bank_pixels.py): SensorRig, a BankRig whose camera buffer holds
the mixed grey layouts of bank_sensors_ref (the grey sensor path the packed path is compared with), PixelRig, the same with
the packed layouts of bank_pixels_ref and a bound format array, and the small helpers around them.  Test modules do not
import each other, so SensorRig and its helpers are restated here as tests/test_gpu_bank_sensors.py has them."""
import numpy as np

import bank_camera_ref as cref
import bank_pixels_ref as pref
import bank_sensors_ref as sref
from bank_ref import FX, FY
from bank_rig import BankRig

SLACK = 4096      # bytes allocated (with BankRig's 64) behind what the library is told: a kernel without the guard would still read memory of the test's
INTERVAL = sref.INTERVAL


def up(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def table_tensor(dev, recs):
    t = up(dev, np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), 32))
    assert t.data_ptr() % 16 == 0
    return t


def put(t, s, rec):
    """Record s of a bound array, rewritten on the current stream: in order with the ticks around it."""
    t[s].copy_(up(t.device, np.frombuffer(np.asarray(rec).tobytes(), np.uint8).copy()))


def counts_of(run, K, T):
    a = run.active[:T - T % K].reshape(-1, K, run.S)
    assert (a.cumprod(axis=1).sum(axis=1) == a.sum(axis=1)).all(), "a burst's frames are a stream's first rounds"
    return a.sum(axis=1).astype(np.uint8)


def cameras(aof, cfg, p):
    """(A's aof_bank_camera: scalars no stream has; B's: the uniform sensor) with the same interval and de-rotation."""
    mk = lambda size: aof.bank_camera_params(size[0], size[1], p.width, p.height, 0, INTERVAL, cref.DEROTATE, FX, FY)
    return mk(sref.SCALARS[cfg]), mk(sref.UNIFORM[cfg])


class SensorRig(BankRig):
    """BankRig whose camera buffer holds the mixed layouts of bank_sensors_ref.TABLES[cfg]: `copies` layouts one behind the
    other per round (the rotating-buffer test uses two), the buffer one byte into its allocation, SLACK bytes allocated
    behind what the library is told (camera_bytes).  round_stride is always passed: 0 would mean the scalars' size.
    bind() binds the records of layout 0 (self.table: rewrite it with put())."""

    def __init__(self, aof, eng, run, bp, dev, cam, cfg, K=None, pad=0, bank=None, copies=1, seed=5):
        import torch
        scalars = type("Scalars", (), dict(cam_w=cam.ingest.camera_width, cam_h=cam.ingest.camera_height))
        super().__init__(aof, eng, run, bp, dev, K=K, camera=(cam, scalars), bank=bank)
        table, order = sref.TABLES[cfg]
        self.layouts, end = [], 0
        for _ in range(copies):
            recs, end = sref.layout(table, order, cam.ingest.crop_width, cam.ingest.crop_height, start=end)
            self.layouts.append(recs)
        R = K or 1
        self.recs, self.layout_bytes, self.seed = self.layouts[0], end, seed
        self.round = end + pad
        self.round_stride = self.round
        self.camera_bytes = (R - 1) * self.round + end
        self.alloc = torch.zeros(1 + R * self.round + SLACK + 64, dtype=torch.uint8, device=dev)
        self.frames = self.alloc[1:1 + R * self.round]
        self.table = table_tensor(dev, self.recs)

    def bind(self, camera_bytes=None):
        self.eng.set_bank_sensors(self.table, self.run.S, self.camera_bytes if camera_bytes is None else camera_bytes)

    def load(self, k, given=None, sensors=None, which=0):
        """As BankRig.load; the frames of every round packed by layout `which` into a buffer of noise."""
        t, run, R = self.torch, self.run, self.K or 1
        for r in range(R):
            buf = sref.pack(self.layouts[which], run.frames[k * R + r], self.layout_bytes, [self.seed, k * R + r])
            self.frames[r * self.round:r * self.round + self.layout_bytes].copy_(t.from_numpy(buf))
        ticks = slice(k * R, (k + 1) * R)
        self.times.copy_(t.from_numpy(run.times[ticks]).view(self.times.shape))
        self.select.copy_(t.from_numpy(run.active[k] if self.K is None else given[k]))
        self.gyro.copy_(t.from_numpy(run.gyro[ticks]).view(self.gyro.shape))
        for g in self.outputs:
            g.refill()


def same_rigs(a, b, what):
    assert a.raw() == b.raw(), (what, "outputs")
    assert a.bank_bytes() == b.bank_bytes(), (what, "bank frames and state")
    assert a.gate_bytes().tolist() == b.gate_bytes().tolist(), (what, "gates")


class PixelRig(SensorRig):
    """SensorRig whose camera buffer holds packed layouts: `tables` is a list of (table, order) of bank_pixels_ref (one
    layout behind the other per round), default its TABLES[cfg].  The formats of layout 0 sit in self.formats, a device
    array one byte into its allocation (no alignment is promised); bind() binds records and formats."""

    def __init__(self, aof, eng, run, bp, dev, cam, cfg, K=None, pad=0, bank=None, tables=None, seed=5):
        import torch
        scalars = type("Scalars", (), dict(cam_w=cam.ingest.camera_width, cam_h=cam.ingest.camera_height))
        BankRig.__init__(self, aof, eng, run, bp, dev, K=K, camera=(cam, scalars), bank=bank)
        self.layouts, self.layout_formats, end = [], [], 0
        for table, order in tables or [pref.TABLES[cfg]]:
            recs, fmts, end = pref.layout(table, order, cam.ingest.crop_width, cam.ingest.crop_height, start=end)
            self.layouts.append(recs)
            self.layout_formats.append(fmts)
        R = K or 1
        self.recs, self.layout_bytes, self.seed = self.layouts[0], end, seed
        self.round = end + pad
        self.round_stride = self.round
        self.camera_bytes = (R - 1) * self.round + end
        self.alloc = torch.zeros(1 + R * self.round + SLACK + 64, dtype=torch.uint8, device=dev)
        self.frames = self.alloc[1:1 + R * self.round]
        self.table = table_tensor(dev, self.recs)
        self.formats_alloc = torch.full((1 + run.S + 64,), 0xEE, dtype=torch.uint8, device=dev)
        self.formats = self.formats_alloc[1:1 + run.S]
        self.formats.copy_(torch.from_numpy(self.layout_formats[0]))
        assert self.formats.data_ptr() % 2 == 1

    def bind(self, camera_bytes=None):
        super().bind(camera_bytes)
        self.eng.set_bank_pixel_formats(self.formats, self.run.S)

    def load(self, k, given=None, sensors=None, which=0):
        t, run, R = self.torch, self.run, self.K or 1
        for r in range(R):
            buf = pref.pack(self.layouts[which], self.layout_formats[which], run.frames[k * R + r], self.layout_bytes, [self.seed, k * R + r])
            self.frames[r * self.round:r * self.round + self.layout_bytes].copy_(t.from_numpy(buf))
        ticks = slice(k * R, (k + 1) * R)
        self.times.copy_(t.from_numpy(run.times[ticks]).view(self.times.shape))
        self.select.copy_(t.from_numpy(run.active[k] if self.K is None else given[k]))
        self.gyro.copy_(t.from_numpy(run.gyro[ticks]).view(self.gyro.shape))
        for g in self.outputs:
            g.refill()

    def put_format(self, s, fmt):
        self.formats[s:s + 1].fill_(int(fmt))
