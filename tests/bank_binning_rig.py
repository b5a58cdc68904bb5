"""The rigs of the binning GPU tests (tests/test_gpu_bank_binning.py): BinnedRig, a SensorRig whose camera buffer holds the
footprints of bank_binning_ref's table (one stream per layout x bin) with the streams' bins bound beside records and
formats, and TwinRig, a SensorRig on grey sensors that is fed the crops the numpy model bins out of a BinnedRig's buffer."""
import numpy as np

import bank_binning_ref as bref
import bank_sensors_ref as sref
from bank_sensor_rig import SensorRig


class BinnedRig(SensorRig):
    """bins: the streams' bins [S] (default: the table's); bind_bins False: the array exists but is not bound by bind().
    self.bins: a device array one byte into its allocation (no alignment is promised; rewrite it with put_bin()).
    self.crops[r]: what the numpy model makes of round r's buffer as it was last filled -- [S, h, w]."""

    def __init__(self, aof, eng, run, bp, dev, cam, w, h, K=None, pad=0, bank=None, table=None, bins=None, bind_bins=True, seed=5):
        import torch
        rows, table_bins = bref.table(w, h)
        super().__init__(aof, eng, run, bp, dev, cam, None, K=K, pad=pad, bank=bank, tables=[(table or rows, bref.ORDER)], formats=True,
                         seed=seed)
        self.w, self.h, self.bind_bins = w, h, bind_bins
        self.host_bins = np.array(table_bins if bins is None else bins, np.uint8)
        self.bins_alloc = torch.full((1 + run.S + 64,), 0xEE, dtype=torch.uint8, device=dev)
        self.bins = self.bins_alloc[1:1 + run.S]
        self.bins.copy_(torch.from_numpy(self.host_bins))
        assert self.bins.data_ptr() % 2 == 1
        self.crops = [None] * (K or 1)

    def bind(self, camera_bytes=None):
        super().bind(camera_bytes)
        if self.bind_bins:
            self.eng.set_bank_binning(self.bins, self.run.S)

    def put_bin(self, s, b, host=True):
        """Stream s's bin on the device, on the current stream; host: the packer follows (False: only the kernels see it)."""
        self.bins[s:s + 1].fill_(int(b))
        if host:
            self.host_bins[s] = b

    def fill_frames(self, k, sensors=None):
        R = self.K or 1
        fmts = self.layout_formats[0]
        for r in range(R):
            buf = bref.pack(self.recs, fmts, self.host_bins, self.run.frames[k * R + r], self.layout_bytes, [self.seed, k * R + r])
            self.crops[r] = np.stack([bref.crop(buf, self.recs[s], int(fmts[s]), int(self.host_bins[s]), self.w, self.h)
                                      for s in range(self.run.S)])
            self.frames[r * self.round:r * self.round + self.layout_bytes].copy_(self.torch.from_numpy(buf))


class TwinRig(SensorRig):
    """Grey sensors (bank_binning_ref.grey_table, bin 1, no formats) holding the crops `source` (a BinnedRig loaded with the
    same tick or burst before this one) binned on the host."""

    def __init__(self, aof, eng, run, bp, dev, cam, w, h, source, K=None, pad=0, bank=None):
        super().__init__(aof, eng, run, bp, dev, cam, None, K=K, pad=pad, bank=bank,
                         tables=[([t[:5] for t in bref.grey_table(w, h)], list(range(run.S)))])
        self.source = source

    def fill_frames(self, k, sensors=None):
        R = self.K or 1
        for r in range(R):
            buf = sref.pack(self.recs, self.source.crops[r], self.layout_bytes, [self.seed, 77, k * R + r])
            self.frames[r * self.round:r * self.round + self.layout_bytes].copy_(self.torch.from_numpy(buf))
