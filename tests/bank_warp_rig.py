"""The rig of the one-launch warped tick's GPU tests (tests/test_gpu_bank_warp_tick.py): the shapes, the run of whole
sensor planes and the rig with a mesh per stream that tests/test_gpu_bank_warp.py builds for the warp launch -- restated
here, because a test module is nobody's library (tests/test_layout.py) --, and the mesh sets of those tests.  S = 5, 64 x 64
crops out of 96 x 80 grey planes behind sensor records at every alignment, T = 6."""
import numpy as np

import bank_ref as ref
import bank_warp_ref as wref
import crop_source_ref as csr
from bank_rig import put, up
from bank_sensor_rig import SensorRig

S, W, H, PW, PH = 5, 64, 64, 96, 80
RATE, INTERVAL, T = 15, 50_000, 6
# sensor width, height, pitch, offset mod 16, crop origin: padded rows, every alignment, the plain crop at and off the centre
ROWS = [(PW, PH, PW, 0, None), (PW, PH, PW + 8, 8, (3, 5)), (PW, PH, PW + 1, 1, (31, 15)), (PW, PH, PW + 35, 7, (0, 0)), (PW, PH, PW, 15, None)]
ORDER = [0, 1, 4, 3, 2]


def planes_run(synth, seed, every_other=None):
    """bank_ref.Run whose `frames` are whole sensor planes [T, S, PH, PW] of moving texture (the warp reads anywhere in
    them); every stream has a frame in every tick but `every_other`, which has one in the even ticks."""
    rng = np.random.default_rng(seed)
    frames = np.zeros((T, S, PH, PW), np.uint8)
    times, active = np.zeros((T, S), np.int64), np.ones((T, S), np.uint8)
    gyro = rng.normal(0, 0.004, (T, S, 4)).astype(np.float32)
    gyro[..., 3] = 0.013
    for s in range(S):
        seq, _ = synth.make_sequence(PW, PH, T, 4, seed=1000 * seed + s, max_step=2)
        if s == every_other:
            active[1::2, s] = 0
        frames[np.flatnonzero(active[:, s]), s] = seq[:int(active[:, s].sum())]
        times[:, s] = np.cumsum(rng.integers(20000, 30000, T))
    return ref.Run(frames, times, gyro, active)


class WarpRig(SensorRig):
    """SensorRig on `rows` (default ROWS: grey planes) whose buffer holds the run's whole planes in the pixel format `fmt`;
    meshes: [S, ny, nx] (POINT_DTYPE) or None: no array.  self.warped[r]: the model's crops of round r's buffer by the
    records and meshes the HOST knows (self.recs, self.meshes; zeros for a record that is not valid)."""

    def __init__(self, aof, eng, run, bp, dev, cam, meshes=None, K=None, pad=0, bank=None, fmt=csr.GREY8, rows=None):
        super().__init__(aof, eng, run, bp, dev, cam, None, K=K, pad=pad, bank=bank, tables=[(rows or ROWS, ORDER)], formats=rows is not None)
        self.fmt = fmt
        self.meshes = None if meshes is None else np.ascontiguousarray(meshes, wref.POINT_DTYPE).copy()
        self.points = None if meshes is None else up(dev, self.meshes.view(np.uint8).reshape(S, -1))
        self.warped = [None] * (K or 1)

    def bind(self):
        super().bind()
        if self.points is not None:
            assert self.points.data_ptr() % 16 == 0
            self.eng.set_bank_warps(self.points, S)

    def give_meshes(self, meshes):
        self.meshes = np.ascontiguousarray(meshes, wref.POINT_DTYPE).copy()
        self.points = up(self.alloc.device, self.meshes.view(np.uint8).reshape(S, -1))

    def put_mesh(self, s, mesh):
        self.meshes[s] = mesh
        put(self.points, s, self.meshes[s])

    def fill_frames(self, k, sensors=None):
        R = self.K or 1
        for r in range(R):
            n = k * R + r
            buf = np.random.default_rng([self.seed, n]).integers(0, 256, self.layout_bytes, dtype=np.uint8)
            for s, rec in enumerate(self.layouts[0]):
                csr.put_grey(buf, int(rec["offset"]) + np.arange(PH)[:, None] * int(rec["pitch"]), self.fmt, np.arange(PW)[None, :], self.run.frames[n, s])
            self.warped[r] = np.stack([self.model(buf, s, r) for s in range(S)])
            self.frames[r * self.round:r * self.round + self.layout_bytes].copy_(self.torch.from_numpy(buf))

    def model(self, buf, s, r=0):
        if not csr.valid(self.recs[s], self.fmt, 1, W, H, self.camera_bytes - r * self.round):
            return np.zeros((H, W), np.uint8)
        mesh = self.meshes[s] if self.meshes is not None else wref.identity(W, H, int(self.recs[s]["x0"]), int(self.recs[s]["y0"]))
        return wref.warp(buf, self.recs[s], self.fmt, mesh, W, H)


def format_rows(fmt):
    """ROWS for planes of one pixel format: the same alignments, pitches in the format's row bytes, crop origins on a pixel
    group of every format (multiples of four)."""
    rb = csr.row_bytes(fmt, PW)
    return [(PW, PH, rb, 0, None, fmt), (PW, PH, rb + 8, 8, (4, 5), fmt), (PW, PH, rb + 1, 1, (28, 15), fmt), (PW, PH, rb + 35, 7, (0, 0), fmt),
            (PW, PH, rb, 15, None, fmt)]


def mixed_meshes(rig):
    """Stream 0 not warped, 1 the helper's barrel lens, 2 a quarter turn, 3 (whose record the tests break) a half-pixel
    shift, 4 a smooth random mesh."""
    d = [wref.designs(W, H, PW, PH, int(r["x0"]), int(r["y0"]), seed=s) for s, r in enumerate(rig.layouts[0])]
    none = d[0]["half-both"].copy()
    none[0, 0]["x"] = wref.NONE
    return np.stack([none, d[1]["barrel"], d[2]["quarter-turn"], d[3]["half-both"], d[4]["smooth-random"]])


def clamp_meshes(rig):
    """The designs that live off the clamp: stream 0 mirrored, 1 minified by two (runs off the plane), 2 with nodes far
    outside every border, 3 (whose record the tests break) a half-pixel shift, 4 not warped."""
    d = [wref.designs(W, H, PW, PH, int(r["x0"]), int(r["y0"]), seed=s) for s, r in enumerate(rig.layouts[0])]
    none = d[4]["barrel"].copy()
    none[0, 0]["x"] = wref.NONE
    return np.stack([d[0]["mirror"], d[1]["minify-2x"], d[2]["far-outside"], d[3]["half-both"], none])
