"""The rigs of the raw-mono-pixel GPU tests (tests/test_gpu_bank_raw.py): RawRig, a SensorRig whose camera buffer holds the
frames of a bank_raw_ref table (any format of include/aof.h, any bin) with formats and bins bound beside the records, and
GreyTwin, a SensorRig on grey sensors that is fed the crops the numpy model reads out of a RawRig's buffer."""
import numpy as np

import bank_raw_ref as rref
import bank_sensors_ref as sref
from bank_rig import BankRig
from bank_sensor_rig import SLACK, SensorRig, table_tensor


class RawRig(SensorRig):
    """rows, bins, order: a table in bank_raw_ref.table's form (default: the configuration's).  The buffer starts one byte
    into its allocation, with SLACK (+ 64) bytes allocated behind camera_bytes; formats and bins are device arrays one
    byte into theirs (rewrite them with put_format() and put_bin()).  self.crops[r]: what the numpy model makes of round
    r's buffer as it was last filled -- [S, h, w]."""

    def __init__(self, aof, eng, run, bp, dev, cam, cfg, K=None, pad=0, bank=None, table=None, seed=5):
        import torch
        scalars = type("Scalars", (), dict(cam_w=cam.ingest.camera_width, cam_h=cam.ingest.camera_height))
        BankRig.__init__(self, aof, eng, run, bp, dev, K=K, camera=(cam, scalars), bank=bank)
        rows, bins, order = table or rref.table(cfg)
        self.w, self.h = cam.ingest.crop_width, cam.ingest.crop_height
        recs, fmts, end = rref.layout(rows, order, bins, self.w, self.h)
        assert len(recs) == run.S
        R = K or 1
        self.layouts, self.layout_formats = [recs], [fmts]
        self.recs, self.layout_bytes, self.seed = recs, end, seed
        self.round = end + pad
        self.round_stride = self.round
        self.camera_bytes = (R - 1) * self.round + end
        self.alloc = torch.zeros(1 + R * self.round + SLACK + 64, dtype=torch.uint8, device=dev)
        self.frames = self.alloc[1:1 + R * self.round]
        self.table = table_tensor(dev, self.recs)
        lead = lambda a: torch.cat([torch.full((1,), 0xEE, dtype=torch.uint8), torch.from_numpy(np.asarray(a, np.uint8)),
                                    torch.full((64,), 0xEE, dtype=torch.uint8)]).to(dev)
        self.host_formats, self.host_bins = fmts.copy(), np.array(bins, np.uint8)
        self.formats_alloc, self.bins_alloc = lead(fmts), lead(bins)
        self.formats, self.bins = self.formats_alloc[1:1 + run.S], self.bins_alloc[1:1 + run.S]
        assert self.formats.data_ptr() % 2 == 1 and self.bins.data_ptr() % 2 == 1
        self.crops = [None] * R

    def bind(self, camera_bytes=None):
        super().bind(camera_bytes)
        self.eng.set_bank_binning(self.bins, self.run.S)

    def put_format(self, s, fmt, host=True):
        """Stream s's format on the device, on the current stream; host: the packer follows (False: only the kernels see it)."""
        super().put_format(s, fmt)
        if host:
            self.host_formats[s] = fmt

    def put_bin(self, s, b, host=True):
        self.bins[s:s + 1].fill_(int(b))
        if host:
            self.host_bins[s] = b

    def fill_frames(self, k, sensors=None):
        R = self.K or 1
        for r in range(R):
            buf = rref.pack_buffer(self.recs, self.host_formats, self.host_bins, self.run.frames[k * R + r], self.layout_bytes,
                                   [self.seed, k * R + r])
            self.crops[r] = np.stack([rref.crop(buf, self.recs[s], int(self.host_formats[s]), int(self.host_bins[s]), self.w, self.h)
                                      for s in range(self.run.S)])
            self.frames[r * self.round:r * self.round + self.layout_bytes].copy_(self.torch.from_numpy(buf))


class GreyTwin(SensorRig):
    """Grey sensors (bank_raw_ref.grey_table, no formats, no bins) holding the crops of `source`, a RawRig loaded with the
    same tick or burst before this one."""

    def __init__(self, aof, eng, run, bp, dev, cam, source, K=None, pad=0, bank=None):
        w, h = cam.ingest.crop_width, cam.ingest.crop_height
        super().__init__(aof, eng, run, bp, dev, cam, None, K=K, pad=pad, bank=bank,
                         tables=[(rref.grey_table(w, h, run.S), list(range(run.S)))])
        self.source = source

    def fill_frames(self, k, sensors=None):
        R = self.K or 1
        for r in range(R):
            buf = sref.pack(self.recs, self.source.crops[r], self.layout_bytes, [self.seed, 77, k * R + r])
            self.frames[r * self.round:r * self.round + self.layout_bytes].copy_(self.torch.from_numpy(buf))
