"""The rig of the per-stream sensor and packed-pixel GPU tests (tests/test_gpu_bank_sensors.py, tests/test_gpu_bank_pixels.py):
SensorRig, a BankRig whose camera buffer holds the mixed layouts of bank_sensors_ref or, with a bound format array, the
packed ones of bank_pixels_ref, and the small helpers around it."""
import numpy as np

import bank_camera_ref as cref
import bank_pixels_ref as pref
import bank_sensors_ref as sref
from bank_ref import FX, FY
from bank_rig import BankRig, up

SLACK = 4096      # bytes allocated (with BankRig's 64) behind what the library is told: a kernel without the guard would still read memory of the test's
INTERVAL = sref.INTERVAL


def table_tensor(dev, recs):
    t = up(dev, np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), 32))
    assert t.data_ptr() % 16 == 0
    return t


def cameras(aof, cfg, p):
    """(A's aof_bank_camera: scalars no stream has; B's: the uniform sensor) with the same interval and de-rotation."""
    mk = lambda size: aof.bank_camera_params(size[0], size[1], p.width, p.height, 0, INTERVAL, cref.DEROTATE, FX, FY)
    return mk(sref.SCALARS[cfg]), mk(sref.UNIFORM[cfg])


def same_rigs(a, b, what):
    assert a.raw() == b.raw(), (what, "outputs")
    assert a.bank_bytes() == b.bank_bytes(), (what, "bank frames and state")
    assert a.gate_bytes().tolist() == b.gate_bytes().tolist(), (what, "gates")


class SensorRig(BankRig):
    """BankRig whose camera buffer holds mixed layouts, one behind the other per round (the rotating-buffer tests use two):
    `tables` is a list of (table, order), default `copies` times the grey bank_sensors_ref.TABLES[cfg] or, with `formats`,
    the packed bank_pixels_ref.TABLES[cfg].  The buffer starts one byte into its allocation, with SLACK bytes allocated
    behind what the library is told (camera_bytes).  round_stride is always passed: 0 would mean the scalars' size.
    bind() binds the records of layout 0 (self.table: rewrite it with put()) and, with `formats`, its formats:
    self.formats, a device array one byte into its allocation (no alignment is promised; rewrite it with put_format())."""

    def __init__(self, aof, eng, run, bp, dev, cam, cfg, K=None, pad=0, bank=None, tables=None, copies=1, formats=False, seed=5):
        import torch
        scalars = type("Scalars", (), dict(cam_w=cam.ingest.camera_width, cam_h=cam.ingest.camera_height))
        super().__init__(aof, eng, run, bp, dev, K=K, camera=(cam, scalars), bank=bank)
        self.layouts, self.layout_formats, end = [], [], 0
        for table, order in tables or [(pref if formats else sref).TABLES[cfg]] * copies:
            recs, *fmts, end = sref.layout(table, order, cam.ingest.crop_width, cam.ingest.crop_height, start=end)
            assert bool(fmts) == bool(formats), "a table with a format column wants formats=True, and the other way round"
            self.layouts.append(recs)
            self.layout_formats.append(fmts[0] if fmts else None)
        R = K or 1
        self.recs, self.layout_bytes, self.seed = self.layouts[0], end, seed
        self.round = end + pad
        self.round_stride = self.round
        self.camera_bytes = (R - 1) * self.round + end
        self.alloc = torch.zeros(1 + R * self.round + SLACK + 64, dtype=torch.uint8, device=dev)
        self.frames = self.alloc[1:1 + R * self.round]
        self.table = table_tensor(dev, self.recs)
        self.formats = None
        if formats:
            self.formats_alloc = torch.full((1 + run.S + 64,), 0xEE, dtype=torch.uint8, device=dev)
            self.formats = self.formats_alloc[1:1 + run.S]
            self.formats.copy_(torch.from_numpy(self.layout_formats[0]))
            assert self.formats.data_ptr() % 2 == 1

    def bind(self, camera_bytes=None):
        self.eng.set_bank_sensors(self.table, self.run.S, self.camera_bytes if camera_bytes is None else camera_bytes)
        if self.formats is not None:
            self.eng.set_bank_pixel_formats(self.formats, self.run.S)

    def fill_frames(self, k, sensors=None, which=0):
        """The frames of every round packed by layout `which` into a buffer of noise."""
        R = self.K or 1
        for r in range(R):
            buf = sref.pack(self.layouts[which], self.run.frames[k * R + r], self.layout_bytes, [self.seed, k * R + r], self.layout_formats[which])
            self.frames[r * self.round:r * self.round + self.layout_bytes].copy_(self.torch.from_numpy(buf))

    def put_format(self, s, fmt):
        self.formats[s:s + 1].fill_(int(fmt))
