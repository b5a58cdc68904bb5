"""The rig of the one-launch warped tick's GPU tests (tests/test_gpu_bank_warp_tick.py, tests/test_gpu_bank_warp_tick_plan.py):
the shapes, the run of whole sensor planes and the rig with a mesh per stream that tests/test_gpu_bank_warp.py builds for
the warp launch -- restated here, because a test module is nobody's library (tests/test_layout.py) --, and the mesh sets of
those tests.  Every piece takes its shape (S streams, W x H crops out of PW x PH planes, T ticks) as an argument; the default
is S = 5, 64 x 64 crops out of 96 x 80 grey planes behind sensor records at every alignment, T = 6.  A shape's planes are at
least 32 columns and 16 rows larger than its crops (the crop origins of its rows)."""
from collections import namedtuple

import numpy as np

import bank_ref as ref
import bank_warp_ref as wref
import crop_source_ref as csr
from bank_rig import put, up
from bank_sensor_rig import SensorRig

Shape = namedtuple("Shape", "S W H PW PH T")
DEFAULT = Shape(5, 64, 64, 96, 80, 6)
S, W, H, PW, PH = DEFAULT[:5]
RATE, INTERVAL, T = 15, 50_000, DEFAULT.T


def shape_rows(shape=DEFAULT):
    """Sensor width, height, pitch, offset mod 16, crop origin of the shape's first S (up to five) streams: padded rows, every
    alignment, the plain crop at and off the centre."""
    pw, ph = shape.PW, shape.PH
    assert 1 <= shape.S <= 5 and pw - shape.W >= 32 and ph - shape.H >= 16
    return [(pw, ph, pw, 0, None), (pw, ph, pw + 8, 8, (3, 5)), (pw, ph, pw + 1, 1, (31, 15)), (pw, ph, pw + 35, 7, (0, 0)), (pw, ph, pw, 15, None)][:shape.S]


def shape_order(shape=DEFAULT):
    """The streams' order in the buffer."""
    return [s for s in (0, 1, 4, 3, 2) if s < shape.S]


ROWS, ORDER = shape_rows(), shape_order()


def planes_run(synth, seed, every_other=None, shape=DEFAULT, ticks=None):
    """bank_ref.Run whose `frames` are whole sensor planes [T, S, PH, PW] of moving texture (the warp reads anywhere in
    them); every stream has a frame in every tick but `every_other`, which has one in the even ticks.  ticks: more ticks than
    the shape's T (a burst behind the ticks)."""
    n, pw, ph = shape.S, shape.PW, shape.PH
    ticks = shape.T if ticks is None else ticks
    rng = np.random.default_rng(seed)
    frames = np.zeros((ticks, n, ph, pw), np.uint8)
    times, active = np.zeros((ticks, n), np.int64), np.ones((ticks, n), np.uint8)
    gyro = rng.normal(0, 0.004, (ticks, n, 4)).astype(np.float32)
    gyro[..., 3] = 0.013
    for s in range(n):
        seq, _ = synth.make_sequence(pw, ph, ticks, 4, seed=1000 * seed + s, max_step=2)
        if s == every_other:
            active[1::2, s] = 0
        frames[np.flatnonzero(active[:, s]), s] = seq[:int(active[:, s].sum())]
        times[:, s] = np.cumsum(rng.integers(20000, 30000, ticks))
    return ref.Run(frames, times, gyro, active)


def host_buffer(recs, nbytes, run, n, fmt=csr.GREY8, seed=5):
    """The camera buffer of tick n on the host: noise, and the run's planes of tick n written in format fmt where the
    records say."""
    ph, pw = run.frames.shape[2:]
    buf = np.random.default_rng([seed, n]).integers(0, 256, nbytes, dtype=np.uint8)
    for s, rec in enumerate(recs):
        csr.put_grey(buf, int(rec["offset"]) + np.arange(ph)[:, None] * int(rec["pitch"]), fmt, np.arange(pw)[None, :], run.frames[n, s])
    return buf


def host_model(buf, rec, fmt, mesh, w, h, camera_bytes):
    """The model's crop of one stream out of a host buffer: zeros for a record that is not valid; mesh None: the identity."""
    if not csr.valid(rec, fmt, 1, w, h, camera_bytes):
        return np.zeros((h, w), np.uint8)
    mesh = mesh if mesh is not None else wref.identity(w, h, int(rec["x0"]), int(rec["y0"]))
    return wref.warp(buf, rec, fmt, mesh, w, h)


class WarpRig(SensorRig):
    """SensorRig on `rows` (default: the shape's grey planes) whose buffer holds the run's whole planes in the pixel format
    `fmt`; meshes: [S, ny, nx] (POINT_DTYPE) or None: no array.  self.warped[r]: the model's crops of round r's buffer by the
    records and meshes the HOST knows (self.recs, self.meshes; zeros for a record that is not valid)."""

    def __init__(self, aof, eng, run, bp, dev, cam, meshes=None, K=None, pad=0, bank=None, fmt=csr.GREY8, rows=None, shape=DEFAULT):
        super().__init__(aof, eng, run, bp, dev, cam, None, K=K, pad=pad, bank=bank, tables=[(rows or shape_rows(shape), shape_order(shape))],
                         formats=rows is not None)
        assert (self.w, self.h) == (shape.W, shape.H) and run.S == shape.S
        self.fmt, self.shape = fmt, shape
        self.meshes = None if meshes is None else np.ascontiguousarray(meshes, wref.POINT_DTYPE).copy()
        self.points = None if meshes is None else up(dev, self.meshes.view(np.uint8).reshape(shape.S, -1))
        self.warped = [None] * (K or 1)

    def bind(self):
        super().bind()
        if self.points is not None:
            assert self.points.data_ptr() % 16 == 0
            self.eng.set_bank_warps(self.points, self.shape.S)

    def give_meshes(self, meshes):
        self.meshes = np.ascontiguousarray(meshes, wref.POINT_DTYPE).copy()
        self.points = up(self.alloc.device, self.meshes.view(np.uint8).reshape(self.shape.S, -1))

    def put_mesh(self, s, mesh):
        self.meshes[s] = mesh
        put(self.points, s, self.meshes[s])

    def fill_frames(self, k, sensors=None):
        R = self.K or 1
        for r in range(R):
            n = k * R + r
            buf = host_buffer(self.layouts[0], self.layout_bytes, self.run, n, self.fmt, self.seed)
            self.warped[r] = np.stack([self.model(buf, s, r) for s in range(self.shape.S)])
            self.frames[r * self.round:r * self.round + self.layout_bytes].copy_(self.torch.from_numpy(buf))

    def model(self, buf, s, r=0):
        return host_model(buf, self.recs[s], self.fmt, None if self.meshes is None else self.meshes[s], self.shape.W, self.shape.H,
                          self.camera_bytes - r * self.round)


def format_rows(fmt, shape=DEFAULT):
    """The shape's rows for planes of one pixel format: the same alignments, pitches in the format's row bytes, crop origins
    on a pixel group of every format (multiples of four)."""
    pw, ph = shape.PW, shape.PH
    rb = csr.row_bytes(fmt, pw)
    return [(pw, ph, rb, 0, None, fmt), (pw, ph, rb + 8, 8, (4, 5), fmt), (pw, ph, rb + 1, 1, (28, 15), fmt), (pw, ph, rb + 35, 7, (0, 0), fmt),
            (pw, ph, rb, 15, None, fmt)][:shape.S]


def stream_designs(recs, shape=DEFAULT):
    return [wref.designs(shape.W, shape.H, shape.PW, shape.PH, int(r["x0"]), int(r["y0"]), seed=s) for s, r in enumerate(recs)]


def mixed_meshes_of(recs, shape=DEFAULT):
    """Stream 0 not warped, 1 the helper's barrel lens, 2 a quarter turn, 3 (whose record the tests break) a half-pixel
    shift, 4 a smooth random mesh.  Four streams: not warped, barrel, smooth random, the refused one."""
    d = stream_designs(recs, shape)
    none = d[0]["half-both"].copy()
    none[0, 0]["x"] = wref.NONE
    if shape.S == 4:
        return np.stack([none, d[1]["barrel"], d[2]["smooth-random"], d[3]["half-both"]])
    return np.stack([none, d[1]["barrel"], d[2]["quarter-turn"], d[3]["half-both"], d[4]["smooth-random"]])


def mixed_meshes(rig, shape=None):
    return mixed_meshes_of(rig.layouts[0], shape or rig.shape)


def clamp_meshes(rig, shape=None):
    """The designs that live off the clamp: stream 0 mirrored, 1 minified by two (runs off the plane), 2 with nodes far
    outside every border, 3 (whose record the tests break) a half-pixel shift, 4 not warped."""
    d = stream_designs(rig.layouts[0], shape or rig.shape)
    none = d[4]["barrel"].copy()
    none[0, 0]["x"] = wref.NONE
    return np.stack([d[0]["mirror"], d[1]["minify-2x"], d[2]["far-outside"], d[3]["half-both"], none])
