"""The stream bank in bursts (aof_bank_push_burst_device / aof_bank_push_camera_burst_device, include/aof.h): K frame
rounds per stream in one call must leave, byte for byte, what K calls of the single-tick entry point leave on a twin
bank -- call k with round k's buffers and d_active[s] = (k < count[s]) -- and what the CPU oracle's chain per stream
leaves (tests/bank_ref.py, tests/bank_camera_ref.py driven round by round with the same activity rule), so that the
feature is not held to the library's own tick alone.  Every case first asserts, on the oracle chain and before the
device is compared, that its input meets the situations it is there for (census()).  Every comparison is on raw
bytes; every output buffer is pre-filled with 0xEE (wire frames with 0)."""
import ctypes as C

import numpy as np
import pytest

import bank_camera_ref as cref
import bank_ref as ref
from bank_ref import FX, FY
from test_gpu_bank import OFFSET, Device, params_of, same_records
from test_gpu_bank_camera import SENSOR, CamDevice, same_exposure, untouched

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC, EIO = -22, -28, -5


def params_for(aof, cfg, overrides=None):
    p = params_of(aof, cfg)
    for k, v in (overrides or {}).items():
        setattr(p, k, int(v))
    return p


def make_burst_run(synth, w, h, S, K, B, seed, wrap=False):
    """B bursts of K rounds as a bank_ref.Run of T = B*K ticks (tick j*K + k is round k of burst j), with bank_ref's
    recipe for the streams (make_sequence per stream, 9 000..18 000 us per active frame, three black frames for streams
    with s % 5 == 3, the u32 time wrap of every third stream behind its fourth frame) and the activity of a burst:
    counts [B, S] drawn from 0..K, stream s active in rounds 0..counts[j, s]-1 of burst j.  Stream 0 has all K frames
    in burst 0 (a first frame with frames behind it), stream 1 % S none in burst 1 % B.  `given` is what the device is
    told: counts with one value above K (which counts as K).  Entries of idle rounds hold noise."""
    rng = np.random.default_rng(seed)
    T = B * K
    frames = rng.integers(0, 256, (T, S, h, w), dtype=np.uint8)
    times = rng.integers(0, 1 << 40, (T, S)).astype(np.int64)
    gyro = rng.normal(0, 1.0, (T, S, 4)).astype(np.float32)
    active = np.zeros((T, S), np.uint8)
    counts = rng.integers(0, K + 1, (B, S)).astype(np.uint8)
    counts[0, 0] = K
    counts[1 % B, 1 % S] = 0
    if S == 1:
        counts[0, 0] = K
    counts[B - 1, S - 1] = K
    given = counts.copy()
    given[B - 1, S - 1] = 200                          # clamped by the kernel: the host cannot see it
    for s in range(S):
        seq, _ = synth.make_sequence(w, h, T, 4, seed=1000 * seed + s, max_step=3)
        if s % 5 == 3:
            seq[7:10] = 0
        n, clock = 0, 0
        for t in range(T):
            j, k = divmod(t, K)
            if k >= counts[j, s]:
                continue
            clock += int(rng.integers(9000, 18000))
            if wrap and s % 3 == 0 and n == 3:
                clock += (1 << 32) - clock - 20000       # the 32-bit time stamp wraps shortly behind this frame
            active[t, s] = 1
            frames[t, s] = seq[n]
            times[t, s] = clock
            gyro[t, s, :3] = rng.normal(0, 0.004, 3).astype(np.float32)
            gyro[t, s, 3] = 0.013
            n += 1
    return ref.Run(frames, times, gyro, active), counts, given


def census(run, counts, K, want, wire, due, rate, first_seq):
    """Which of the situations a burst has to get right this input shows, on the oracle chain alone."""
    T, S = run.T, run.S
    q, frame = want["quality"], want["frame"]
    out = set()
    for t in range(T):
        j, k = divmod(t, K)
        for s in range(S):
            c = int(counts[j, s])
            if k == 0 and c == 0:
                out.add("count0")
            if not run.active[t, s]:
                continue
            if k == 0 and frame[t, s] == 1 and c >= 2:
                out.add("first-frame-then-more")
            if q[t, s] >= 0 and frame[t, s] > 1 and k < c - 1:
                out.add("publication-before-the-last-round")
            if q[t, s] == ref.TICK_HELD:
                out.add("held")
            if rate > 0 and frame[t, s] > 1 and want[t, s]["pixel"]["quality"] == 0:
                out.add("zero-quality-frame-skipped")
            if k >= 1 and (int(run.times[t, s]) >> 32) != (int(run.times[t - 1, s]) >> 32):
                out.add("u32-wrap-inside-a-burst")
            if due is not None and k >= 1 and due[t, s] and k < c - 1 and not due[t + 1:j * K + c, s].any():
                out.add("gate-opens-in-a-later-round-and-stays-shut")
    for s in range(S):
        seqs = [w[s][4] for w in wire if w[s]]           # MAVLink 2: the sequence number is byte 4
        if any(a == 255 and b == 0 for a, b in zip(seqs, seqs[1:])):
            out.add("sequence-255-to-0")
    if rate <= 0:
        out.add("rate0")
    return out


class BurstDevice:
    """One bank and the buffers of a burst of K rounds on the device.  camera: (aof_bank_camera, CameraRun) for the
    sensor-frame form.  pad: bytes added to the dense round_stride (0: round_stride is passed as 0)."""

    def __init__(self, aof, eng, run, K, bp, gpu_device, camera=None, use_gyro=True, exposure=True, skew=0, pad=0):
        import torch
        self.aof, self.eng, self.run, self.K, self.torch = aof, eng, run, K, torch
        self.cam, self.cam_run = camera if camera else (None, None)
        self.bank = eng.bank_create(bp, gpu_device, camera=self.cam)
        S = run.S
        self.pixels = run.frames.shape[2] * run.frames.shape[3]
        if self.cam is None:
            self.item, self.stride = self.pixels, bp.frame_stride or self.pixels
        else:
            self.item = self.cam_run.cam_w * self.cam_run.cam_h
            self.stride = self.cam.camera_stride or self.item
        self.round = S * self.stride + pad
        self.round_stride = self.round if pad else 0
        self.alloc = torch.zeros(K * self.round + 64, dtype=torch.uint8, device=gpu_device)
        self.frames = self.alloc[skew:skew + K * self.round]
        z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device=gpu_device)
        self.times, self.count = z(K, S, dtype=torch.int64), z(S)
        self.gyro = z(K, S, 4, dtype=torch.float32) if use_gyro else None
        self.records, self.wire, self.lens = z(K, S, 48), z(K, S, 56), z(K, S)
        self.exposure, self.derotated, self.want_exposure = z(K, S, 48), z(K, S, 8), exposure

    def load(self, j, given, sensors=None):
        t, run, K, S = self.torch, self.run, self.K, self.run.S
        for k in range(K):
            tick = j * K + k
            if self.cam is None:
                data = run.frames[tick].reshape(S, -1)
            else:
                data = (sensors[k] if sensors is not None else self.cam_run.sensor(tick)).reshape(S, -1)
            dst = self.frames[k * self.round:k * self.round + S * self.stride].view(S, self.stride)
            dst[:, :self.item].copy_(t.from_numpy(np.ascontiguousarray(data)))
        self.times.copy_(t.from_numpy(run.times[j * K:(j + 1) * K]))
        self.count.copy_(t.from_numpy(given[j]))
        if self.gyro is not None:
            self.gyro.copy_(t.from_numpy(run.gyro[j * K:(j + 1) * K]))
        for buf in (self.records, self.lens, self.exposure, self.derotated):   # (every output of every round must be written)
            buf.fill_(0xEE)
        self.wire.zero_()

    def enqueue(self, all_rounds=False):
        count = None if all_rounds else self.count
        if self.cam is None:
            self.eng.bank_push_burst(self.bank, self.K, self.frames, self.times, count, self.gyro, mavlink=True,
                                     records=self.records, out_frames=self.wire, out_lengths=self.lens,
                                     round_stride=self.round_stride)
        else:
            self.eng.bank_push_camera_burst(self.bank, self.K, self.frames, self.times, count, self.gyro, mavlink=True,
                                            records=self.records, exposure=self.exposure if self.want_exposure else None,
                                            derotated=self.derotated, out_frames=self.wire, out_lengths=self.lens,
                                            want_exposure=self.want_exposure, round_stride=self.round_stride)

    def read(self):
        """Per round: (records, wire frames, exposure records, de-rotated floats)."""
        self.torch.cuda.synchronize()
        w, n = self.wire.cpu().numpy(), self.lens.cpu().numpy()
        e, d = self.exposure.cpu().numpy(), self.derotated.cpu().numpy()
        S = self.run.S
        return [(self.aof.ticks_view(self.records[k]), [bytes(w[k, s, :n[k, s]]) for s in range(S)],
                 e[k].view(self.aof.EXPOSURE_DTYPE).reshape(S), d[k].view(np.float32)) for k in range(self.K)]

    def push(self, j, given, sensors=None):
        self.load(j, given, sensors)
        self.enqueue()
        return self.read()

    def raw(self):
        """Every output buffer as bytes (for comparisons between two devices)."""
        self.torch.cuda.synchronize()
        return b"".join(b.cpu().numpy().tobytes() for b in (self.records, self.wire, self.lens, self.exposure, self.derotated))

    def bank_bytes(self):
        return self.bank.frames_bytes().tobytes() + self.bank.state_bytes().tobytes()

    def gate_bytes(self):
        return np.ascontiguousarray(self.bank.state_bytes()[:, 56:64]).view("<u8").reshape(-1)


class Case:
    """The inputs of one case and everything the oracle chain expects of it, made on the CPU."""

    def __init__(self, aof, orc, synth, cfg, K, S=24, B=6, seed=1, camera=False, overrides=None, rate=15, first_seq=0,
                 wrap=False, use_gyro=True, exposure=True, derotate=True, sensor=None, skew=0, pad=0, frame_stride=0,
                 camera_stride=0, interval=cref.EXPOSURE_INTERVAL_US, path=0, needs=(), resets=None, fx=FX, fy=FY, burst_run=None):
        """fx, fy: the focal lengths of the bank, the camera's de-rotation and the oracle chains.  burst_run: (Run, counts,
        given) in make_burst_run's form to use in its place, as they are (no saturated patches)."""
        self.aof, self.K, self.S, self.B, self.camera, self.path = aof, K, S, B, camera, path
        self.use_gyro, self.exposure, self.derotate, self.skew, self.pad = use_gyro, exposure, derotate, skew, pad
        self.p = p = params_for(aof, cfg, overrides)
        if burst_run is not None:
            self.run, self.counts, self.given = burst_run
            assert (self.run.T, self.run.S) == (B * K, S)
        else:
            self.run, self.counts, self.given = make_burst_run(synth, p.width, p.height, S, K, B, seed, wrap=wrap)
            if camera:
                cref.add_saturated_patches(self.run)
        new = lambda s=0: ref.oracle_chain(aof, orc, p, rate, OFFSET, first_seq, use_gyro, fx=fx, fy=fy)
        tick_resets = {j * K: m for j, m in (resets or {}).items()}
        self.want, self.wire = ref.expected(self.run, [new() for _ in range(S)], resets=tick_resets, new_chain=new)
        self.bp = aof.bank_params(S, fx, fy, rate, OFFSET, 1, 100, first_seq, frame_stride)
        self.due = self.after = self.derot = self.cam = self.cam_run = None
        if camera:
            sensor = sensor or SENSOR[cfg]
            self.cam = aof.bank_camera_params(sensor[0], sensor[1], p.width, p.height, camera_stride, interval,
                                              cref.DEROTATE if derotate else None, fx, fy)
            self.cam_run = cref.CameraRun(self.run, sensor[0], sensor[1], seed)
            self.due, self.after = cref.gate(self.run.times, self.run.active, interval, resets=tick_resets)
            if not exposure:                # no statistics: the gate does not move
                self.due[:], self.after[:] = 0, 0
            self.derot = np.stack([cref.expected_derotated(orc, self.want[t], self.run.gyro[t], fx, fy, use_gyro=use_gyro)
                                   for t in range(self.run.T)])
        # conditions on the INPUT, checked on the CPU chain before the device is compared
        self.seen = census(self.run, self.counts, K, self.want, self.wire, self.due if exposure else None, rate, first_seq)
        if camera and not exposure:
            self.seen.add("no-exposure-records")
        if camera and (self.cam_run.y0 * self.cam_run.cam_w + self.cam_run.x0 + skew) % 2 == 1:
            self.seen.add("crop-origin-on-an-odd-byte")
        assert (self.given > K).any(), "one count above K"
        missing = set(needs) - self.seen
        assert not missing, ("the oracle chain of this input does not show", missing, "only", self.seen)

    def engine(self, path=None):
        eng = self.aof.FlowEngine(self.p, 0)
        eng.set_bank_path(self.path if path is None else path)
        return eng

    def burst_device(self, eng, gpu_device):
        return BurstDevice(self.aof, eng, self.run, self.K, self.bp, gpu_device, camera=(self.cam, self.cam_run) if self.camera else None,
                           use_gyro=self.use_gyro, exposure=self.exposure, skew=self.skew, pad=self.pad)

    def tick_device(self, eng, gpu_device):
        if self.camera:
            return CamDevice(self.aof, eng, self.run, self.cam_run, self.bp, self.cam, gpu_device, use_gyro=self.use_gyro,
                             exposure=self.exposure, skew=self.skew)
        return Device(self.aof, eng, self.run, self.bp, gpu_device, use_gyro=self.use_gyro)

    def sensors(self, j):
        return [self.cam_run.sensor(j * self.K + k) for k in range(self.K)] if self.camera else None

    def check_against_oracle(self, j, got, orc):
        """Burst j's outputs against the oracle chain, round by round."""
        for k, (recs, sent, expo, derot) in enumerate(got):
            t = j * self.K + k
            same_records(recs, self.want[t], t, "oracle")
            assert sent == self.wire[t], ("oracle wire", j, k, [s for s in range(self.S) if sent[s] != self.wire[t][s]][:4])
            if not self.camera:
                continue
            if self.exposure:
                want_e = cref.expected_exposure(self.aof, orc, self.cam_run.sensor(t), self.run, t, self.due[t])
                same_exposure(expo, want_e, t, "oracle exposure")
            else:
                assert untouched(expo), (j, k)
            if self.derotate:
                assert derot.tobytes() == self.derot[t].tobytes(), ("de-rotated", j, k)
            else:
                assert untouched(derot), (j, k)

    def check_against_ticks(self, j, got, twin):
        """Burst j's outputs against K single ticks on the twin bank (call k: round k's buffers, active = k < count)."""
        sensors = self.sensors(j)
        for k, (recs, sent, expo, derot) in enumerate(got):
            t = j * self.K + k
            assert (self.run.active[t] == (k < np.minimum(self.counts[j], self.K))).all()
            if self.camera:
                tick = twin.push(t, sensors[k])
                assert recs.tobytes() == tick.recs.tobytes() and sent == tick.wire, ("records of K ticks", j, k)
                assert expo.tobytes() == tick.exposure.tobytes(), ("exposure of K ticks", j, k)
                assert derot.tobytes() == tick.derotated.tobytes(), ("de-rotated of K ticks", j, k)
            else:
                trecs, twire = twin.push(t)
                assert recs.tobytes() == trecs.tobytes() and sent == twire, ("records of K ticks", j, k)


BASIC = ("first-frame-then-more", "count0", "publication-before-the-last-round", "held")
GATE = ("gate-opens-in-a-later-round-and-stays-shut",)

CASES = [
    dict(id="px4-64-K5", cfg="px4-64", K=5, seed=1, needs=BASIC + ("zero-quality-frame-skipped",)),
    dict(id="px4-64-K1", cfg="px4-64", K=1, B=24, seed=2, needs=("count0", "held")),
    dict(id="px4-64-K16-wrap", cfg="px4-64", K=16, B=3, seed=3, wrap=True, needs=BASIC + ("u32-wrap-inside-a-burst",)),
    dict(id="px4-64-K7-seq253", cfg="px4-64", K=7, B=8, seed=4, first_seq=253, needs=BASIC + ("sequence-255-to-0",)),
    dict(id="px4-64-K5-rate0", cfg="px4-64", K=5, seed=5, rate=0, needs=("rate0", "first-frame-then-more", "count0")),
    dict(id="px4-64-K3-no-subpixel-stride", cfg="px4-64", K=3, B=10, seed=6, overrides=dict(subpixel=0), frame_stride=64 * 64 + 48,
         pad=96, needs=BASIC),
    dict(id="px4-64-K5-mean-subtract", cfg="px4-64", K=5, seed=7, overrides=dict(mean_subtract=1), needs=BASIC),
    dict(id="opencv-128-K5", cfg="opencv-128", K=5, seed=8, needs=BASIC),
    dict(id="opencv-128-K16-no-gyro", cfg="opencv-128", K=16, B=3, S=12, seed=9, use_gyro=False, needs=BASIC),
    dict(id="opencv-128-K3-plain-levels", cfg="opencv-128", K=3, B=10, S=12, seed=10, overrides=dict(subpixel=0, mean_subtract=0),
         needs=BASIC),
    dict(id="px4-64-K5-composed", cfg="px4-64", K=5, seed=11, path=2, needs=BASIC),
    dict(id="dense-192x160-K4", cfg="dense-192x160", K=4, S=12, seed=12, needs=BASIC),
    dict(id="camera-px4-64-K5", cfg="px4-64", camera=True, K=5, seed=21, needs=BASIC + GATE + ("zero-quality-frame-skipped",)),
    dict(id="camera-px4-64-K1", cfg="px4-64", camera=True, K=1, B=24, seed=22, needs=("count0", "held")),
    dict(id="camera-px4-64-K16-wrap", cfg="px4-64", camera=True, K=16, B=3, seed=23, wrap=True,
         needs=BASIC + GATE + ("u32-wrap-inside-a-burst",)),
    dict(id="camera-odd-origin-K7", cfg="px4-64", camera=True, sensor=(322, 242), skew=2, K=7, B=6, seed=24, pad=37,
         camera_stride=322 * 242 + 5, needs=BASIC + GATE + ("crop-origin-on-an-odd-byte",)),
    dict(id="camera-no-exposure-K5", cfg="px4-64", camera=True, K=5, seed=25, exposure=False, needs=BASIC + ("no-exposure-records",)),
    dict(id="camera-no-subpixel-no-derotate-K3", cfg="px4-64", camera=True, K=3, B=10, seed=26, overrides=dict(subpixel=0),
         derotate=False, interval=50_000, needs=BASIC + GATE),
    dict(id="camera-opencv-128-K5", cfg="opencv-128", camera=True, K=5, S=12, seed=27, needs=BASIC + GATE),
    dict(id="camera-opencv-128-K16-rate0", cfg="opencv-128", camera=True, K=16, B=2, S=8, seed=28, rate=0, interval=50_000,
         needs=("rate0", "first-frame-then-more") + GATE),
    dict(id="camera-opencv-128-K3-plain-levels", cfg="opencv-128", camera=True, K=3, B=8, S=8, seed=29,
         overrides=dict(subpixel=0, mean_subtract=0), needs=BASIC),
    dict(id="camera-px4-64-K5-composed", cfg="px4-64", camera=True, K=5, seed=30, path=2, needs=BASIC + GATE),
    dict(id="camera-tile16-K4", cfg="tile16-160x128", camera=True, K=4, S=12, seed=31, interval=50_000, needs=BASIC + GATE),
]

EVERY_SITUATION = set(BASIC + GATE + ("zero-quality-frame-skipped", "u32-wrap-inside-a-burst", "sequence-255-to-0", "rate0",
                                      "no-exposure-records", "crop-origin-on-an-odd-byte"))


def test_the_cases_ask_for_every_situation_the_issue_lists():
    assert set().union(*(c["needs"] for c in CASES)) == EVERY_SITUATION
    ks = {c["K"] for c in CASES}
    assert 1 in ks and 16 in ks and any(k % 2 == 1 and k > 1 for k in ks)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_a_burst_equals_k_single_ticks_on_a_twin_bank_and_the_oracle_chain(aof, orc, synth, gpu_device, case):
    """After every burst of a run of several: every output against K single ticks on a twin bank and against the oracle
    chain per stream, and the bank's frames and state regions against the twin's."""
    c = Case(aof, orc, synth, **{k: v for k, v in case.items() if k != "id"})      # (asserts the census)
    eng, eng_t = c.engine(), c.engine()
    dev, twin = c.burst_device(eng, gpu_device), c.tick_device(eng_t, gpu_device)
    for j in range(c.B):
        got = dev.push(j, c.given, c.sensors(j))
        c.check_against_oracle(j, got, orc)
        c.check_against_ticks(j, got, twin)
        assert dev.bank.frames_bytes().tobytes() == twin.bank.frames_bytes().tobytes(), ("frames region", j)
        assert dev.bank.state_bytes().tobytes() == twin.bank.state_bytes().tobytes(), ("state region", j)
        if c.camera:
            assert dev.gate_bytes().tolist() == c.after[(j + 1) * c.K - 1].tolist(), ("gate", j)
    eng.close(), eng_t.close()


def test_a_null_count_means_every_round(aof, orc, synth, gpu_device):
    """d_count == NULL: all K rounds of every stream, against K ticks with d_active == NULL on a twin bank."""
    p = params_of(aof, "px4-64")
    S, K, B = 16, 5, 3
    run = ref.make_run(synth, 64, 64, S, K * B, 41, black=False)
    run.active[:] = 1
    for s in range(S):                                   # (make_run's idle entries hold noise: give every tick a frame)
        run.frames[:, s] = synth.make_sequence(64, 64, K * B, 4, seed=4100 + s, max_step=3)[0]
        run.times[:, s] = 11000 * (np.arange(K * B) + 1) + 7 * s
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    eng, eng_t = aof.FlowEngine(p, 0), aof.FlowEngine(p, 0)
    dev, twin = BurstDevice(aof, eng, run, K, bp, gpu_device), Device(aof, eng_t, run, bp, gpu_device)
    full = np.full((B, S), K, np.uint8)
    for j in range(B):
        dev.load(j, full)
        dev.enqueue(all_rounds=True)
        for k, (recs, sent, _, _) in enumerate(dev.read()):
            twin.load(j * K + k)
            eng_t.bank_push(twin.bank, twin.frames, twin.times, None, twin.gyro, mavlink=True, records=twin.records,
                            out_frames=twin.wire, out_lengths=twin.lens)
            trecs, twire = twin.read()
            assert recs.tobytes() == trecs.tobytes() and sent == twire, (j, k)
        assert dev.bank_bytes() == twin.bank.frames_bytes().tobytes() + twin.bank.state_bytes().tobytes(), j
    eng.close(), eng_t.close()


@pytest.mark.parametrize("camera,cfg,K,seed", [(False, "px4-64", 5, 51), (False, "opencv-128", 16, 52), (True, "px4-64", 7, 53),
                                               (True, "opencv-128", 5, 54)])
def test_both_paths_leave_identical_bytes_after_every_burst(aof, orc, synth, gpu_device, camera, cfg, K, seed):
    """aof_set_bank_path 1 and 2 over the same run: every output and the bank's frames and state regions identical
    after every burst; path 0 equals them."""
    c = Case(aof, orc, synth, cfg, K, S=16, B=4, seed=seed, camera=camera, needs=BASIC)
    engs = [c.engine(path) for path in (1, 2, 0)]
    devs = [c.burst_device(e, gpu_device) for e in engs]
    for j in range(c.B):
        sensors = c.sensors(j)
        outs = []
        for d in devs:
            d.load(j, c.given, sensors)
            d.enqueue()
            outs.append((d.raw(), d.bank_bytes()))
        assert outs[0][0] == outs[1][0], ("outputs, path 1 against path 2", j)
        assert outs[0][1] == outs[1][1], ("bank bytes, path 1 against path 2", j)
        assert outs[2] == outs[0], ("path 0", j)
    for e in engs:
        e.close()


@pytest.mark.parametrize("camera", [False, True])
def test_a_masked_reset_between_bursts(aof, orc, synth, gpu_device, camera):
    """A masked reset between two bursts: the reset streams are new to the next burst -- a first frame, sequence number
    first_seq, the gate open --, the others go on as if nothing had happened.  Against the oracle chain with fresh
    objects for the reset streams, on both paths."""
    import torch
    S, K, B, at = 24, 5, 6, 3
    mask = (np.arange(S) % 3 == 1).astype(np.uint8)
    c = Case(aof, orc, synth, "px4-64", K, S=S, B=B, seed=61, camera=camera, first_seq=9, resets={at: mask}, needs=BASIC)
    plain = Case(aof, orc, synth, "px4-64", K, S=S, B=B, seed=61, camera=camera, first_seq=9)
    assert c.want.tobytes() != plain.want.tobytes(), "the reset changes what the chain expects"
    for path in (1, 2):
        eng = c.engine(path)
        dev = c.burst_device(eng, gpu_device)
        for j in range(B):
            if j == at:
                before = dev.bank.state_bytes()
                eng.bank_reset(dev.bank, torch.from_numpy(mask).to(gpu_device))
                after = dev.bank.state_bytes()
                assert not after[mask == 1].any() and after[mask == 0].tobytes() == before[mask == 0].tobytes()
            got = dev.push(j, c.given, c.sensors(j))
            c.check_against_oracle(j, got, orc)
            if camera:
                assert dev.gate_bytes().tolist() == c.after[(j + 1) * K - 1].tolist(), (path, j)
        first_after = [(int(np.flatnonzero(c.run.active[at * K:, s])[0]) + at * K, s) for s in np.flatnonzero(mask)]
        assert all(c.want[t, s]["frame"] == 1 for t, s in first_after)
        eng.close()


@pytest.mark.parametrize("camera,path", [(False, 1), (False, 2), (True, 1), (True, 2)])
def test_a_captured_burst_replays_on_new_inputs(aof, orc, synth, gpu_device, camera, path):
    """One burst captured with torch.cuda.graph (a linear graph: one stream) and replayed for every burst of a run with
    new frames, times and counts copied into the same input tensors equals the eager run."""
    import torch
    c = Case(aof, orc, synth, "opencv-128", 5, S=12, B=5, seed=71, camera=camera, needs=BASIC)
    eng = c.engine(path)
    eager = c.burst_device(eng, gpu_device)
    outs = []
    for j in range(c.B):
        eager.load(j, c.given, c.sensors(j))
        eager.enqueue()
        outs.append(eager.raw())
    dev = c.burst_device(eng, gpu_device)
    dev.push(0, c.given, c.sensors(0))           # (every kernel of the burst has run once before the capture)
    eng.bank_reset(dev.bank)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dev.enqueue()
    for j in range(c.B):
        dev.load(j, c.given, c.sensors(j))
        g.replay()
        assert dev.raw() == outs[j], j
    assert dev.bank_bytes() == eager.bank_bytes()
    eng.close()


def test_burst_entry_points_argument_handling(aof, synth, gpu_device):
    """What the burst entry points refuse on top of the single-tick ones, with which code, and that a refused call
    leaves the bank and the outputs untouched."""
    import torch
    p = params_of(aof, "px4-64")
    S, K, cw, ch = 8, 4, 320, 240
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    cam = aof.bank_camera_params(cw, ch, 64, 64, 0, 200_000, cref.DEROTATE, FX, FY)
    L, staging = aof.bank_camera_layout(p, bp, cam)
    assert staging == aof.bank_layout(p, bp).total_bytes
    buf = torch.zeros(L.total_bytes + 256, dtype=torch.uint8, device=gpu_device)
    sensor = torch.randint(0, 256, (K, S, ch, cw), dtype=torch.uint8, device=gpu_device)
    frames = sensor[:, :, 88:152, 128:192].contiguous()
    times = (torch.arange(K * S, dtype=torch.int64, device=gpu_device).view(K, S) // S) * 12000 + 70000
    outs = dict(recs=torch.zeros((K, S, 48), dtype=torch.uint8, device=gpu_device),
                expo=torch.zeros(K * S * 48 + 4, dtype=torch.uint8, device=gpu_device),
                derot=torch.zeros(K * S * 8 + 4, dtype=torch.uint8, device=gpu_device),
                wire=torch.zeros((K, S, 56), dtype=torch.uint8, device=gpu_device),
                lens=torch.zeros((K, S), dtype=torch.uint8, device=gpu_device))
    stream = torch.cuda.current_stream().cuda_stream
    plain, camera, reset = aof.lib.aof_bank_push_burst_device, aof.lib.aof_bank_push_camera_burst_device, aof.lib.aof_bank_reset_device
    burst = aof.bank_burst_params(K)

    def pargs(**kw):
        b, u = kw.get("bp", bp), kw.get("burst", burst)
        return [kw.get("ctx", eng._ctx), C.byref(b) if b is not None else None, C.byref(u) if u is not None else None,
                kw.get("frames", frames.data_ptr()), kw.get("times", times.data_ptr()), None, None, kw.get("bank", buf.data_ptr()),
                kw.get("bytes", L.total_bytes), kw.get("recs", outs["recs"].data_ptr()), kw.get("wire", outs["wire"].data_ptr()),
                kw.get("lens", outs["lens"].data_ptr()), stream]

    def cargs(**kw):
        b, u, c = kw.get("bp", bp), kw.get("burst", burst), kw.get("cam", cam)
        return [kw.get("ctx", eng._ctx), C.byref(b) if b is not None else None, C.byref(c) if c is not None else None,
                C.byref(u) if u is not None else None, kw.get("sensor", sensor.data_ptr()), kw.get("times", times.data_ptr()), None, None,
                kw.get("bank", buf.data_ptr()), kw.get("bytes", L.total_bytes), kw.get("recs", outs["recs"].data_ptr()),
                kw.get("expo", outs["expo"].data_ptr()), kw.get("derot", outs["derot"].data_ptr()),
                kw.get("wire", outs["wire"].data_ptr()), kw.get("lens", outs["lens"].data_ptr()), stream]

    assert reset(eng._ctx, C.byref(bp), None, buf.data_ptr(), L.total_bytes, stream) == 0
    assert camera(*cargs()) == 0
    torch.cuda.synchronize()
    r = aof.ticks_view(outs["recs"][K - 1])
    assert (r["frame"] == K).all()
    for t in outs.values():
        t.fill_(0xEE)
    snapshot = buf.clone()
    bad = lambda **kw: aof.bank_params(**{**dict(n_streams=S, focal_x=FX, focal_y=FY, output_rate=15, offset_timestamp_usec=OFFSET), **kw})
    bcam = lambda *a, **kw: aof.bank_camera_params(*a, **{**dict(derotate=cref.DEROTATE, focal_x=FX, focal_y=FY), **kw})
    B = aof.bank_burst_params
    common = [
        (dict(ctx=None), EINVAL), (dict(bp=None), EINVAL), (dict(burst=None), EINVAL), (dict(bank=None), EINVAL),
        (dict(times=None), EINVAL), (dict(recs=None), EINVAL), (dict(lens=None), EINVAL),
        (dict(burst=B(0)), EINVAL), (dict(burst=B(17)), EINVAL), (dict(burst=B(-1)), EINVAL),
        (dict(bp=bad(n_streams=0)), EINVAL), (dict(bp=bad(frame_stride=4096 + 8)), EINVAL), (dict(bp=bad(focal_x=0.0)), EINVAL),
        (dict(bank=buf.data_ptr() + 16), EINVAL),
    ]
    plain_only = [
        (dict(frames=None), EINVAL),
        (dict(burst=B(K, S * 4096 - 16)), EINVAL),        # below one round
        (dict(burst=B(K, S * 4096 + 8)), EINVAL),         # not a multiple of 16
        (dict(burst=B(K, -S * 4096)), EINVAL),
        (dict(bytes=staging - 1), ENOSPC),                # (staging == aof_bank_layout().total_bytes)
        (dict(bp=bad(n_streams=S + 1), bytes=staging), ENOSPC),
    ]
    camera_only = [
        (dict(sensor=None), EINVAL), (dict(cam=None), EINVAL), (dict(derot=None), EINVAL),
        (dict(expo=outs["expo"].data_ptr() + 2), EINVAL), (dict(derot=outs["derot"].data_ptr() + 2), EINVAL),
        (dict(cam=bcam(cw, ch, 64, 48)), EINVAL), (dict(cam=bcam(64, 48, 64, 64)), EINVAL),
        (dict(cam=bcam(cw, ch, 64, 64, camera_stride=cw * ch - 1)), EINVAL),
        (dict(burst=B(K, S * cw * ch - 1)), EINVAL),      # below one round of sensor frames
        (dict(bytes=L.total_bytes - 1), ENOSPC), (dict(bp=bad(n_streams=S + 1)), ENOSPC),
        (dict(bytes=staging), ENOSPC),                    # a bank sized by aof_bank_layout
    ]
    for kw, code in common + plain_only:
        assert plain(*pargs(**kw)) == code, ("plain", kw)
    for kw, code in common + camera_only:
        assert camera(*cargs(**kw)) == code, ("camera", kw)
    torch.cuda.synchronize()
    assert torch.equal(buf, snapshot), "a refused call must leave the bank untouched"
    assert all(untouched(t.cpu().numpy()) for t in outs.values()), "a refused call must leave the outputs untouched"
    assert b"bank" in aof.lib.aof_last_error(eng._ctx)
    # the context is still usable: a padded round_stride for the camera form needs no alignment, and a bank sized by the
    # camera layout serves the plain burst; NULL d_count / d_gyro / d_mavlink / d_exposure are fine
    times += 80000
    assert plain(*pargs(wire=None, lens=None)) == 0
    torch.cuda.synchronize()
    assert (aof.ticks_view(outs["recs"][K - 1])["frame"] == 2 * K).all()
    off = aof.bank_camera_params(cw, ch, 64, 64, 0, 200_000, None, FX, FY)
    times += 80000
    assert camera(*cargs(cam=off, expo=None, derot=None, wire=None, lens=None)) == 0
    torch.cuda.synchronize()
    assert (aof.ticks_view(outs["recs"][0])["frame"] == 2 * K + 1).all()
    assert untouched(outs["expo"].cpu().numpy()) and untouched(outs["derot"].cpu().numpy())
    eng.close()


def test_a_faulted_context_launches_no_burst(aof, synth, gpu_device):
    """The context's sticky device-side condition (a finaliser deadline, as tests/test_gpu_parity.py raises it): the
    burst entry points return -EIO like the single-tick ones, before their first launch -- the bank keeps its bytes."""
    import torch
    p = aof.default_params(640, 480)
    hp, hc, _ = synth.make_batch(640, 480, 8, 4, 4300)
    idx = np.arange(256) % 8
    eng = aof.FlowEngine(p, 0)
    S, K = 2, 3
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    cam = aof.bank_camera_params(640, 480, 640, 480, 0, 200_000, None, FX, FY)
    bank = eng.bank_create(bp, gpu_device, camera=cam)
    eng.set_search_mode(aof.SEARCH_EXHAUSTIVE)
    eng.set_reduce_fusion(True)
    eng.debug_vote_deadline_ticks(0)
    eng.flow_batch(torch.from_numpy(hp[idx]).to(gpu_device), torch.from_numpy(hc[idx]).to(gpu_device))
    torch.cuda.synchronize()
    bank.buffer.fill_(0xC3)
    frames = torch.full((K, S, 480, 640), 0x5A, dtype=torch.uint8, device=gpu_device)
    times = torch.arange(K * S, dtype=torch.int64, device=gpu_device).view(K, S) * 40000
    codes = []
    for call in (lambda: eng.bank_push(bank, frames[0], times[0]), lambda: eng.bank_push_camera(bank, frames[0], times[0]),
                 lambda: eng.bank_push_burst(bank, K, frames, times), lambda: eng.bank_push_camera_burst(bank, K, frames, times)):
        with pytest.raises(aof.AofError) as e:
            call()
        codes.append(e.value.code)
        assert "deadline" in str(e.value)
    assert codes == [EIO] * 4
    torch.cuda.synchronize()
    assert bool((bank.buffer == 0xC3).all()), "the faulted context must not have launched anything into the bank"
    eng.close()
