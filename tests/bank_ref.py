"""Inputs and the expected outputs of the stream bank tests (tests/test_gpu_bank.py): S independent live streams over T
ticks, and for each stream what the reference's per-frame loop (mainloop.cpp:322-373) around a calcFlow implementation
leaves for every frame it is given -- the CPU oracle's calcFlow chain with the independent serializer of
tests/mavlink_model.py, or the C++ facade with its own packer.  Nothing here touches the GPU."""
import numpy as np

from mavlink_model import py_frame

FX, FY = 216.6677, 216.2457
TICK_HELD, TICK_IDLE = -1, -2


class Run:
    """frames [T, S, h, w] u8, times [T, S] i64, gyro [T, S, 4] f32, active [T, S] u8.  Entries of idle streams hold
    noise: nothing may read them."""

    def __init__(self, frames, times, gyro, active):
        self.frames, self.times, self.gyro, self.active = frames, times, gyro, active
        self.T, self.S = active.shape


def make_run(synth, w, h, S, T, case_seed, wrap=False, black=True, density=None, source=None):
    """The recipe of the issue: stream s uses make_sequence(w, h, T, 4, seed=1000*case_seed + s, max_step=3) -- or, with
    `source`, the T frames [T, h, w] that source(s, T) returns --; it joins at
    tick s % 4; it is idle in tick k when (7k + 3s) % 5 == 0 (or, with `density`, with that probability); every active
    tick advances its clock by 9 000..18 000 us; streams with s % 5 == 3 see three black frames (their frames 7..9);
    with `wrap`, the 32-bit time stamp of every third stream wraps in the middle of the run."""
    rng = np.random.default_rng(case_seed)
    frames = rng.integers(0, 256, (T, S, h, w), dtype=np.uint8)
    times = rng.integers(0, 1 << 40, (T, S)).astype(np.int64)
    gyro = rng.normal(0, 1.0, (T, S, 4)).astype(np.float32)
    active = np.zeros((T, S), np.uint8)
    for s in range(S):
        if source is None:
            seq, _ = synth.make_sequence(w, h, T, 4, seed=1000 * case_seed + s, max_step=3)
        else:
            seq = np.array(source(s, T), dtype=np.uint8)
            assert seq.shape == (T, h, w)
        if black and s % 5 == 3:
            seq[7:10] = 0
        n, clock = 0, 0
        for k in range(T):
            if k < s % 4:
                continue
            idle = (7 * k + 3 * s) % 5 == 0 if density is None else rng.random() >= density
            if idle:
                continue
            clock += int(rng.integers(9000, 18000))
            if wrap and s % 3 == 0 and k == T // 2:
                clock += (1 << 32) - clock - 20000       # the 32-bit time stamp wraps shortly behind this frame
            active[k, s] = 1
            frames[k, s] = seq[n]
            times[k, s] = clock
            gyro[k, s, :3] = rng.normal(0, 0.004, 3).astype(np.float32)
            gyro[k, s, 3] = 0.013
            n += 1
    return Run(frames, times, gyro, active)


class Chain:
    """One stream: mainloop.cpp:322-373 around `calc_flow(img, t32) -> (q, dt, ax, ay)`: the negative-return gate, the
    gyro taken and zeroed with every published flow, the frame.  `pixel(prev, cur)` gives the pair's aof_flow record
    (None: the record's pixel field is left zero and the caller does not compare it)."""

    def __init__(self, tick_dtype, calc_flow, pack, offset, first_seq, pixel=None, use_gyro=True):
        self.dtype, self.calc_flow, self.pack, self.pixel = tick_dtype, calc_flow, pack, pixel
        self.offset, self.seq, self.use_gyro = offset, first_seq, use_gyro
        self.g = np.zeros(3, np.float64)
        self.n = 0
        self.prev = None

    def push(self, img, t, gyro):
        rec = np.zeros((), self.dtype)
        self.n += 1
        if self.use_gyro:
            self.g += gyro[:3].astype(np.float64)                   # integrated since the last message (:383-405)
        q, dt, ax, ay = self.calc_flow(img, int(t) & 0xFFFFFFFF)
        rec["frame"] = self.n
        if self.pixel is not None and self.prev is not None:
            rec["pixel"] = self.pixel(self.prev, img)
        self.prev = img
        if q < 0:                                                   # :327-331
            rec["quality"] = TICK_HELD
            return rec, b""
        taken, self.g = self.g.copy(), np.zeros(3, np.float64)      # :333-334
        rec["quality"], rec["dt_us"] = q, dt
        rec["flow_x"], rec["flow_y"] = np.float32(ax), np.float32(ay)
        rec["gyro_x"], rec["gyro_y"], rec["gyro_z"] = (np.float32(v) for v in taken)
        wire = b""
        if self.offset:                                             # :353-357
            wire = self.pack(self.offset, int(t), dt, float(np.float32(ax)), float(np.float32(ay)),
                             tuple(float(v) for v in taken), q, self.seq & 0xFF)
            self.seq += 1
        return rec, wire


def oracle_chain(aof, orc, p, rate, offset, first_seq, use_gyro=True, fx=FX, fy=FY):
    po = orc.params_from(p)
    o = orc.Px4(po, fx, fy, rate)
    return Chain(aof.TICK_DTYPE, o.calc_flow, py_frame, offset, first_seq,
                 pixel=lambda a, b: orc.flow_pair(po, a, b)["flow"], use_gyro=use_gyro)


def expected(run, chains, resets=None, new_chain=None):
    """records [T, S] (TICK_DTYPE) and wire [T][S] (bytes) of feeding every stream's chain its active frames.
    resets: {tick: mask [S]}: before that tick the masked streams start over with new_chain(s)."""
    T, S = run.T, run.S
    recs = np.zeros((T, S), chains[0].dtype)
    wire = [[b""] * S for _ in range(T)]
    for k in range(T):
        if resets and k in resets:
            for s in np.flatnonzero(resets[k]):
                chains[s] = new_chain(int(s))
        for s in range(S):
            if not run.active[k, s]:
                recs[k, s]["quality"] = TICK_IDLE
                continue
            recs[k, s], wire[k][s] = chains[s].push(run.frames[k, s], run.times[k, s], run.gyro[k, s])
    return recs, wire


def census(recs):
    """Per stream: (published, held, idle) over the run."""
    q = recs["quality"]
    return (q >= 0).sum(0), (q == TICK_HELD).sum(0), (q == TICK_IDLE).sum(0)
