"""The rig of the sensor-table GPU tests (tests/test_gpu_bank_sensors.py, _pixels.py, _binning.py, _raw.py): SensorRig, a
BankRig whose camera buffer holds the frames of a layout table -- grey sensors, packed pixels, binned footprints, raw mono
pixels: whatever crop_source_ref can lay out and pack --, the constructors that pick the binning and the raw tests'
tables, GreyTwin, which is fed the crops the numpy model reads out of another rig's buffer, and the small helpers around
them."""
import numpy as np

import bank_binning_ref as bref
import bank_camera_ref as cref
import bank_pixels_ref as pref
import bank_raw_ref as rref
import bank_sensors_ref as sref
import crop_source_ref as csr
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
    `tables` is a list of (rows, order) or (rows, bins, order) in crop_source_ref.layout's form, default `copies` times the
    grey bank_sensors_ref.TABLES[cfg] or, with `formats`, the packed bank_pixels_ref.TABLES[cfg].  The buffer starts one
    byte into its allocation, with SLACK bytes allocated behind what the library is told (camera_bytes).  round_stride is
    always passed: 0 would mean the scalars' size.
    bind() binds the records of layout 0 (self.table: rewrite it with put()); with `formats` its formats and, where layout 0
    came with bins (and bind_bins), its bins: self.formats, self.bins, device arrays one byte into their allocations (no
    alignment is promised; rewrite them with put_format() and put_bin()).  host_formats, host_bins: what the packer packs
    layout 0 by; a put follows there if asked (host; default `follow`), else only the kernels see it.
    self.crops[r]: what the numpy model makes of round r's buffer as it was last filled -- [S, h, w]."""

    def __init__(self, aof, eng, run, bp, dev, cam, cfg, K=None, pad=0, bank=None, tables=None, copies=1, formats=False, bind_bins=True,
                 follow=False, seed=5):
        import torch
        scalars = type("Scalars", (), dict(cam_w=cam.ingest.camera_width, cam_h=cam.ingest.camera_height))
        super().__init__(aof, eng, run, bp, dev, K=K, camera=(cam, scalars), bank=bank)
        self.w, self.h = cam.ingest.crop_width, cam.ingest.crop_height
        self.layouts, self.layout_formats, end = [], [], 0
        for rows, *bins, order in tables or [(pref if formats else sref).TABLES[cfg]] * copies:
            assert (len(rows[0]) > 5) == bool(formats), "a table with a format column wants formats=True, and the other way round"
            recs, fmts, end = csr.layout(rows, order, self.w, self.h, bins[0] if bins else None, start=end)
            self.layouts.append(recs)
            self.layout_formats.append(fmts)
            if len(self.layouts) == 1:
                self.host_bins = np.array(bins[0], np.uint8) if bins else None
        assert len(self.layouts[0]) == run.S
        R = K or 1
        self.recs, self.layout_bytes, self.seed = self.layouts[0], end, seed
        self.round = end + pad
        self.round_stride = self.round
        self.camera_bytes = (R - 1) * self.round + end
        self.alloc = torch.zeros(1 + R * self.round + SLACK + 64, dtype=torch.uint8, device=dev)
        self.frames = self.alloc[1:1 + R * self.round]
        self.table = table_tensor(dev, self.recs)
        self.host_formats, self.bind_bins, self.follow = self.layout_formats[0].copy(), bind_bins, follow
        self.formats = self._odd(self.host_formats) if formats else None
        self.bins = self._odd(self.host_bins) if self.host_bins is not None else None
        self.crops = [None] * R

    def _odd(self, values):
        """A device copy of [S] bytes one byte into its allocation, 0xEE around it."""
        alloc = self.torch.full((1 + len(values) + 64,), 0xEE, dtype=self.torch.uint8, device=self.alloc.device)
        alloc[1:1 + len(values)].copy_(self.torch.from_numpy(values))
        assert alloc[1:].data_ptr() % 2 == 1
        return alloc[1:1 + len(values)]

    def bind(self, camera_bytes=None):
        self.eng.set_bank_sensors(self.table, self.run.S, self.camera_bytes if camera_bytes is None else camera_bytes)
        if self.formats is not None:
            self.eng.set_bank_pixel_formats(self.formats, self.run.S)
        if self.bins is not None and self.bind_bins:
            self.eng.set_bank_binning(self.bins, self.run.S)

    def fill_frames(self, k, sensors=None, which=0):
        """The frames of every round packed by layout `which` into a buffer of noise."""
        R = self.K or 1
        recs, fmts = self.layouts[which], self.layout_formats[which] if which else self.host_formats
        bins = self.host_bins if self.host_bins is not None else np.ones(self.run.S, np.uint8)
        for r in range(R):
            buf = self.pack(recs, fmts, bins, k * R + r)
            self.crops[r] = np.stack([csr.crop(buf, recs[s], int(fmts[s]), int(bins[s]), self.w, self.h) for s in range(self.run.S)])
            self.frames[r * self.round:r * self.round + self.layout_bytes].copy_(self.torch.from_numpy(buf))

    def pack(self, recs, fmts, bins, n):
        return csr.pack(recs, self.run.frames[n], self.layout_bytes, [self.seed, n], fmts, bins)

    def put_format(self, s, fmt, host=None):
        """Stream s's format on the device, on the current stream; host: the packer follows (False: only the kernels see it)."""
        self.formats[s:s + 1].fill_(int(fmt))
        if self.follow if host is None else host:
            self.host_formats[s] = fmt

    def put_bin(self, s, b, host=None):
        self.bins[s:s + 1].fill_(int(b))
        if self.follow if host is None else host:
            self.host_bins[s] = b


def BinnedRig(aof, eng, run, bp, dev, cam, w, h, K=None, pad=0, bank=None, table=None, bins=None, bind_bins=True, seed=5):
    """The binning tests' rig: the footprints of bank_binning_ref's table (one stream per layout x bin; `table`: other rows),
    the streams' bins (default: the table's) bound beside records and formats; bind_bins False: the array exists but is
    not bound by bind()."""
    rows, table_bins = bref.table(w, h)
    return SensorRig(aof, eng, run, bp, dev, cam, None, K=K, pad=pad, bank=bank, formats=True, bind_bins=bind_bins, follow=True, seed=seed,
                     tables=[(table or rows, table_bins if bins is None else bins, bref.ORDER)])


def RawRig(aof, eng, run, bp, dev, cam, cfg, K=None, pad=0, bank=None, table=None, seed=5):
    """The raw-mono tests' rig: the frames of a table in bank_raw_ref.table's form (rows, bins, order; default: the
    configuration's), any format of include/aof.h and any bin, formats and bins bound beside the records."""
    return SensorRig(aof, eng, run, bp, dev, cam, cfg, K=K, pad=pad, bank=bank, formats=True, follow=True, seed=seed,
                     tables=[table or rref.table(cfg)])


class GreyTwin(SensorRig):
    """Grey sensors (bank_raw_ref.grey_table, no formats, no bins) holding the crops of `source`, a rig loaded with the same
    tick or burst before this one: what the numpy model read out of its buffer."""

    def __init__(self, aof, eng, run, bp, dev, cam, source, K=None, pad=0, bank=None):
        w, h = cam.ingest.crop_width, cam.ingest.crop_height
        super().__init__(aof, eng, run, bp, dev, cam, None, K=K, pad=pad, bank=bank, tables=[(rref.grey_table(w, h, run.S), list(range(run.S)))])
        self.source = source

    def pack(self, recs, fmts, bins, n):
        return csr.pack(recs, self.source.crops[n % (self.K or 1)], self.layout_bytes, [self.seed, 77, n])
