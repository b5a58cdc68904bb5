"""The cases of the stream bank's device tests that more than one file runs (tests/test_gpu_bank*.py,
tests/test_gpu_tail_matrix.py): one bank over one run against the oracle chain tick by tick, in its frame form (run_case)
and its sensor-frame form (run_camera_case), and the burst cases (make_burst_run, census, Case).  Every case asserts on
the oracle chain, before the device is compared, that its input meets the situations it is there for.  Every comparison
is on raw bytes.  The device rig: tests/bank_rig.py; inputs and expected values: tests/bank_ref.py,
tests/bank_camera_ref.py."""
import numpy as np

import bank_camera_ref as cref
import bank_ref as ref
from bank_ref import FX, FY
from bank_rig import OFFSET, SENSOR, BankRig, params_for, params_of, same_exposure, same_records, untouched


def run_case(aof, orc, synth, gpu_device, cfg, S, T, seed, rate=15, offset=OFFSET, first_seq=0, wrap=False, use_gyro=True,
             path=0, facade=0, density=None, census=None, frame_stride=0, fx=FX, fy=FY, source=None):
    """One bank over one Run against the oracle chain (all streams) and the facade (streams < facade); returns the
    oracle's records.  fx, fy: the focal lengths of the bank, the chains and the facade objects; source: bank_ref.make_run's
    per-stream sequence source."""
    p = params_of(aof, cfg)
    run = ref.make_run(synth, p.width, p.height, S, T, seed, wrap=wrap, density=density, source=source)
    want, wire = ref.expected(run, [ref.oracle_chain(aof, orc, p, rate, offset, first_seq, use_gyro, fx=fx, fy=fy) for _ in range(S)])
    pub, held, idle = ref.census(want)
    if census is not None:          # a condition on the INPUT: a bank that never holds or never publishes cannot pass
        assert pub.min() >= census[0] and held.min() >= census[1] and idle.min() >= census[2], (pub, held, idle)
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    bp = aof.bank_params(S, fx, fy, rate, offset, 1, 100, first_seq, frame_stride)
    dev = BankRig(aof, eng, run, bp, gpu_device, use_gyro=use_gyro)
    stride = frame_stride or p.width * p.height
    facs = []
    for s in range(min(facade, S)):
        f = aof.OpticalFlowPX4(fx, fy, rate, p.width, p.height) if p.pyramid_levels == 1 else aof.OpticalFlowOpenCV(fx, fy, rate, p.width, p.height)
        assert f.getPyramidLevels() == p.pyramid_levels
        facs.append(f)
    chains_f = [ref.Chain(aof.TICK_DTYPE, f.calcFlow, aof.pack_optical_flow_rad, offset, first_seq, use_gyro=use_gyro) for f in facs]
    for k in range(T):
        before_frames, before_state = dev.bank.frames_bytes(), dev.bank.state_bytes()
        got, sent, _, _ = dev.push(k)
        same_records(got, want[k], k, "oracle")
        assert sent == wire[k], ("oracle wire", k, [s for s in range(S) if sent[s] != wire[k][s]][:4])
        if offset == 0:
            assert all(len(f) == 0 for f in sent)
        for s, ch in enumerate(chains_f):
            if run.active[k, s]:
                r, w = ch.push(run.frames[k, s], run.times[k, s], run.gyro[k, s])
                same_records(got[s:s + 1], np.array([r]), k, f"facade stream {s}", pixel=False)
                assert sent[s] == w, ("facade wire", k, s)
        # idle streams: nothing about them changed; active streams: the bank holds their new frame
        after_frames, after_state = dev.bank.frames_bytes(), dev.bank.state_bytes()
        for s in range(S):
            slot = slice(s * stride, s * stride + p.width * p.height)
            if run.active[k, s]:
                assert after_frames[slot].tobytes() == run.frames[k, s].tobytes(), ("stored frame", k, s)
            else:
                assert after_frames[slot].tobytes() == before_frames[slot].tobytes(), ("idle frame", k, s)
                assert after_state[s].tobytes() == before_state[s].tobytes(), ("idle state", k, s)
    for f in facs:
        f.close()
    eng.close()
    return want


def prepare(aof, orc, synth, p, S, T, seed, interval, rate, wrap, use_gyro, census, gated, exposure, derotate, fx=FX, fy=FY,
            source=None, patches=True):
    """The inputs and everything expected of a case, with the conditions on the INPUT asserted (no device needed)."""
    run = ref.make_run(synth, p.width, p.height, S, T, seed, wrap=wrap, source=source)
    if patches:
        cref.add_saturated_patches(run)
    want, wire = ref.expected(run, [ref.oracle_chain(aof, orc, p, rate, OFFSET, 0, use_gyro, fx=fx, fy=fy) for _ in range(S)])
    due, after = cref.gate(run.times, run.active, interval)
    if not exposure:                # no statistics: the gate does not move
        due[:], after[:] = 0, 0
    derot = np.stack([cref.expected_derotated(orc, want[k], run.gyro[k], fx, fy, use_gyro=use_gyro) for k in range(T)])
    # conditions on the INPUT, before the device runs: a bank that never gates, holds or de-rotates cannot pass
    if census is not None:
        pub, held, idle = ref.census(want)
        assert pub.min() >= census[0] and held.min() >= census[1] and idle.min() >= census[2], (pub, held, idle)
    if gated is not None:
        n_due, n_not = due.sum(0), ((run.active == 1) & (due == 0)).sum(0)
        assert n_due.min() >= gated[0] and n_not.min() >= gated[1], (n_due, n_not)
    if derotate and use_gyro:
        pairs = (want["quality"] != ref.TICK_IDLE) & (want["frame"] > 1)
        raw = np.stack([want["pixel"]["flow_x"], want["pixel"]["flow_y"]], -1)
        moved = (derot != raw).any(-1)
        assert (pairs & moved).any() and (pairs & ~moved & (raw != 0).any(-1)).any(), "some pair is compensated, some is left alone"
    return run, want, wire, due, after, derot


def run_camera_case(aof, orc, synth, gpu_device, cfg, S, T, seed, sensor=None, interval=cref.EXPOSURE_INTERVAL_US, rate=15,
             wrap=False, use_gyro=True, path=0, census=None, gated=None, frame_stride=0, camera_stride=0, exposure=True,
             derotate=True, skew=0, fx=FX, fy=FY, source=None, patches=True):
    """One camera bank over one Run against the oracle chain, tick by tick; returns (records, due).  fx, fy: the focal
    lengths of the bank, the de-rotation and the chains; source: bank_ref.make_run's per-stream sequence source; patches:
    the saturated patches of bank_camera_ref on the frames."""
    p = params_of(aof, cfg)
    sensor = sensor or SENSOR[cfg]
    run, want, wire, due, after, derot = prepare(aof, orc, synth, p, S, T, seed, interval, rate, wrap, use_gyro, census, gated,
                                                 exposure, derotate, fx=fx, fy=fy, source=source, patches=patches)
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    bp = aof.bank_params(S, fx, fy, rate, OFFSET, 1, 100, 0, frame_stride)
    cam = aof.bank_camera_params(sensor[0], sensor[1], p.width, p.height, camera_stride, interval,
                                 cref.DEROTATE if derotate else None, fx, fy)
    cam_run = cref.CameraRun(run, sensor[0], sensor[1], seed)
    dev = BankRig(aof, eng, run, bp, gpu_device, camera=(cam, cam_run), use_gyro=use_gyro, exposure=exposure, skew=skew)
    stride = frame_stride or p.width * p.height
    for k in range(T):
        frames_img = cam_run.sensor(k)
        want_e = cref.expected_exposure(aof, orc, frames_img, run, k, due[k])   # (asserts: the oracle's crop is the run's frame)
        before_frames, before_state = dev.bank.frames_bytes(), dev.bank.state_bytes()
        got = dev.push(k, sensors=frames_img)
        same_records(got.recs, want[k], k, "oracle")
        assert got.wire == wire[k], ("oracle wire", k, [s for s in range(S) if got.wire[s] != wire[k][s]][:4])
        if exposure:
            same_exposure(got.exposure, want_e, k, "oracle exposure")
        else:
            assert untouched(got.exposure), k
        if derotate:
            assert got.derotated.tobytes() == derot[k].tobytes(), ("de-rotated", k, got.derotated, derot[k])
        else:
            assert untouched(got.derotated), k
        after_frames, after_state = dev.bank.frames_bytes(), dev.bank.state_bytes()
        for s in range(S):
            slot = slice(s * stride, s * stride + p.width * p.height)
            if run.active[k, s]:
                assert after_frames[slot].tobytes() == run.frames[k, s].tobytes(), ("stored frame = the oracle's crop", k, s)
            else:
                assert after_frames[slot].tobytes() == before_frames[slot].tobytes(), ("idle frame", k, s)
                assert after_state[s].tobytes() == before_state[s].tobytes(), ("idle state and gate", k, s)
        assert dev.gate_bytes().tolist() == after[k].tolist(), ("gate", k)
    eng.close()
    return want, due


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

    def rig(self, eng, gpu_device, burst):
        return BankRig(self.aof, eng, self.run, self.bp, gpu_device, K=self.K if burst else None,
                       camera=(self.cam, self.cam_run) if self.camera else None, use_gyro=self.use_gyro, exposure=self.exposure,
                       skew=self.skew, pad=self.pad if burst else 0)

    def burst_device(self, eng, gpu_device):
        return self.rig(eng, gpu_device, True)

    def tick_device(self, eng, gpu_device):
        return self.rig(eng, gpu_device, False)

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
            tick = twin.push(t, sensors=sensors[k] if self.camera else None)      # (the frame forms leave both fills untouched)
            assert recs.tobytes() == tick.recs.tobytes() and sent == tick.wire, ("records of K ticks", j, k)
            assert expo.tobytes() == tick.exposure.tobytes(), ("exposure of K ticks", j, k)
            assert derot.tobytes() == tick.derotated.tobytes(), ("de-rotated of K ticks", j, k)
