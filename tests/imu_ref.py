"""The stream bank's IMU of include/aof.h ("the stream bank's IMU"; the reference's highres_imu_msg_callback,
mainloop.cpp:383-405, and its send gates, mainloop.cpp:333-357) restated in plain Python floats (IEEE doubles, every
operation rounded on its own) and ``struct``, from DESIGN.md section 2 "Stream bank IMU" and not from the C++.  run()
takes [K][M][S] samples and [K][S] records over S states and returns what the library's calls must write, byte for
byte, with a tally of which outcomes occurred; family() makes the inputs that reach all of them.  Nothing here touches
the GPU or the library (the dtypes and the OPTICAL_FLOW_RAD serializer are restated, so that the library's are checked
against them)."""
import collections
import math
import struct

import numpy as np

from mavlink_model import x25

SLOTS_MAX, BURST_MAX, FRAME_BYTES = 16, 16, 56
HELD, IDLE, STALE_GYRO, NO_OFFSET = -1, -2, -3, -4
SENTINEL = 0xA5                      # fill of frame bytes nobody may write
M64 = (1 << 64) - 1

SAMPLE_DTYPE = np.dtype([("time_usec", "<u8"), ("xgyro", "<f4"), ("ygyro", "<f4"), ("zgyro", "<f4"), ("reserved", "<u4")])
STATE_DTYPE = np.dtype([("gyro_x", "<f8"), ("gyro_y", "<f8"), ("gyro_z", "<f8"), ("prev_time_usec", "<u8"),
                        ("last_taken_time_usec", "<u8"), ("offset_timestamp_usec", "<u8"), ("messages", "<u4"),
                        ("samples_integrated", "<u4"), ("samples_rejected", "<u4"), ("dropped", "<u4")])
FLOW_DTYPE = np.dtype([("flow_x", "<f4"), ("flow_y", "<f4"), ("count", "<u4"), ("quality", "u1"), ("flags", "u1"),
                       ("pred_x", "i1"), ("pred_y", "i1")])
RECORD_DTYPE = np.dtype([("quality", "<i4"), ("dt_us", "<i4"), ("flow_x", "<f4"), ("flow_y", "<f4"), ("gyro_x", "<f4"),
                         ("gyro_y", "<f4"), ("gyro_z", "<f4"), ("frame", "<u4"), ("pixel", FLOW_DTYPE)])
assert SAMPLE_DTYPE.itemsize == 24 and STATE_DTYPE.itemsize == 64 and RECORD_DTYPE.itemsize == 48

# Everything the coverage family must reach at least once (test_bank_imu_ref.py asserts it on the model alone).
OUTCOMES = ("accepted", "rejected_prev_zero", "rejected_dt", "rejected_rate", "dt_exactly_50000", "dt_exactly_49999",
            "time_backwards", "rate_exactly_20", "rate_just_below_20", "negative_rate_accepted", "negative_rate_rejected",
            "nan", "plus_inf", "minus_inf", "time_zero", "offset_learned", "offset_preset_sent", "stale_before_any_sample",
            "stale_no_sample_between_takes", "sent_after_stale", "no_offset", "sent", "sent_first_frame", "held", "idle",
            "seq_wrapped", "count_zero", "count_full", "count_above_max", "idle_round_with_samples")
BELOW_20 = float(np.nextafter(np.float32(20), np.float32(0)))


def frame(time_usec, dt_us, flow_x, flow_y, g, quality, seq, system_id, component_id):
    """One MAVLink 2 OPTICAL_FLOW_RAD frame (message 106, CRC_EXTRA 138): wire order by field size, the gyro axes switched
    as mainloop.cpp:364-365 does, trailing zero bytes of the payload cut."""
    payload = struct.pack("<QI", time_usec & M64, dt_us & 0xFFFFFFFF)
    payload += np.array([flow_x, flow_y], "<f4").tobytes()                 # (the record's own bits, NaN payloads included)
    payload += np.array([-g[1], g[0], g[2]], "<f8").astype("<f4").tobytes()
    payload += struct.pack("<IfhBB", 0, -1.0, 0, 0, quality & 0xFF)
    assert len(payload) == 44
    while len(payload) > 1 and payload[-1] == 0:
        payload = payload[:-1]
    head = bytes([len(payload), 0, 0, seq & 0xFF, system_id, component_id, 106, 0, 0])
    return b"\xfd" + head + payload + struct.pack("<H", x25(bytes([138]), x25(head + payload)))


class Stream:
    """One stream's aof_imu_state, in Python numbers; `alt` are the sums of the order the design rejects (acc + the
    round's own sum), kept beside the real ones to show that the two orders differ."""

    def __init__(self, record):
        self.g = [float(record["gyro_x"]), float(record["gyro_y"]), float(record["gyro_z"])]
        self.prev, self.last, self.offset = (int(record[n]) for n in ("prev_time_usec", "last_taken_time_usec", "offset_timestamp_usec"))
        self.messages, self.integrated, self.rejected, self.dropped = (
            int(record[n]) for n in ("messages", "samples_integrated", "samples_rejected", "dropped"))
        self.alt, self.round_sum = list(self.g), [0.0, 0.0, 0.0]
        self.was_stale = False

    def store(self, record):
        record["gyro_x"], record["gyro_y"], record["gyro_z"] = self.g
        record["prev_time_usec"], record["last_taken_time_usec"], record["offset_timestamp_usec"] = self.prev, self.last, self.offset
        record["messages"], record["samples_integrated"] = self.messages & 0xFFFFFFFF, self.integrated & 0xFFFFFFFF
        record["samples_rejected"], record["dropped"] = self.rejected & 0xFFFFFFFF, self.dropped & 0xFFFFFFFF


def sample(st, t, x, y, z, tally):
    """One HIGHRES_IMU sample; x, y, z are float32 values held in Python floats."""
    step = (t - st.prev) & M64
    dt = float(step) / 1e6                         # (int -> float is correctly rounded, like the C conversion)
    rates_ok = abs(x) < 20.0 and abs(y) < 20.0 and abs(z) < 20.0     # (False for a NaN)
    if st.prev != 0:                               # the edges, counted where only they decide
        if t < st.prev:
            tally["time_backwards"] += 1
        if rates_ok:
            tally["dt_exactly_50000"] += step == 50000
            tally["dt_exactly_49999"] += step == 49999
        if dt < 0.05:
            for v in (x, y, z):
                tally["nan"] += math.isnan(v)
                tally["plus_inf"] += v == math.inf
                tally["minus_inf"] += v == -math.inf
                tally["rate_exactly_20"] += v == 20.0
                tally["negative_rate_rejected"] += v == -20.0
            if rates_ok:
                tally["rate_just_below_20"] += BELOW_20 in (abs(x), abs(y), abs(z))
                tally["negative_rate_accepted"] += min(x, y, z) < 0
    if st.prev != 0 and dt < 0.05 and rates_ok:
        for i, v in enumerate((x, y, z)):
            inc = v * dt
            st.g[i] = st.g[i] + inc
            st.round_sum[i] = st.round_sum[i] + inc
        st.integrated += 1
        tally["accepted"] += 1
    else:
        st.rejected += 1
        tally["rejected_prev_zero" if st.prev == 0 else "rejected_dt" if not dt < 0.05 else "rejected_rate"] += 1
    tally["time_zero"] += t == 0
    st.prev = t
    if st.offset == 0:
        st.offset = t                              # (t == 0 changes nothing)
        tally["offset_learned"] += t != 0


def end_of_round_samples(st):
    for i in range(3):
        st.alt[i] = st.alt[i] + st.round_sum[i]
        st.round_sum[i] = 0.0


def take(st, rec, t, first_seq, system_id, component_id, tally, preset):
    """The round's record (a numpy void of RECORD_DTYPE, changed in place).  Returns the frame's bytes, b"" if none."""
    q = int(rec["quality"])
    if q < 0:
        tally["held" if q == HELD else "idle"] += 1
        return b""
    g = tuple(st.g)
    st.g, st.alt = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    rec["gyro_x"], rec["gyro_y"], rec["gyro_z"] = np.array(g, "<f8").astype("<f4")
    if st.last == st.prev:
        rec["quality"] = STALE_GYRO
        st.dropped += 1
        tally["stale_before_any_sample" if st.prev == 0 and st.integrated + st.rejected == 0 else "stale_no_sample_between_takes"] += 1
        st.was_stale = True
        return b""
    st.last = st.prev
    if st.offset == 0:
        rec["quality"] = NO_OFFSET
        st.dropped += 1
        tally["no_offset"] += 1
        return b""
    seq = (first_seq + st.messages) & 0xFF
    tally["sent"] += 1
    tally["sent_first_frame"] += int(rec["frame"]) == 1
    tally["sent_after_stale"] += st.was_stale
    tally["offset_preset_sent"] += preset
    tally["seq_wrapped"] += first_seq + st.messages == 256
    st.was_stale = False
    st.messages += 1
    return frame(st.offset + int(t), int(rec["dt_us"]), rec["flow_x"], rec["flow_y"], g, q, seq, system_id, component_id)


def run(samples, counts, times, records, states, first_seq=0, system_id=1, component_id=100, pack=True):
    """samples SAMPLE_DTYPE [K, M, S]; counts u8 [K, S] or None; times u64 [K, S]; records RECORD_DTYPE [K, S]; states
    STATE_DTYPE [S] (not changed).  Returns dict(records [K, S], frames u8 [K, S, 56] filled with SENTINEL behind every
    length, lengths u8 [K, S], states [S], tally, alt: the [S, 3] sums of the per-round-increment order)."""
    K, M, S = samples.shape
    assert 1 <= K <= BURST_MAX and 1 <= M <= SLOTS_MAX and records.shape == (K, S) and times.shape == (K, S)
    out = records.copy()
    frames = np.full((K, S, FRAME_BYTES), SENTINEL, np.uint8)
    lengths = np.zeros((K, S), np.uint8)
    states_out = states.copy()
    tally = collections.Counter()
    alt = np.zeros((S, 3))
    for s in range(S):
        st = Stream(states[s])
        preset = int(states[s]["offset_timestamp_usec"]) != 0
        for k in range(K):
            n = M if counts is None else int(counts[k, s])
            tally["count_zero"] += n == 0
            tally["count_full"] += n == M
            tally["count_above_max"] += n > M
            n = min(n, M)
            tally["idle_round_with_samples"] += n > 0 and int(records[k, s]["quality"]) == IDLE
            for j in range(n):
                m = samples[k, j, s]
                sample(st, int(m["time_usec"]), float(m["xgyro"]), float(m["ygyro"]), float(m["zgyro"]), tally)
            end_of_round_samples(st)
            f = take(st, out[k, s], int(times[k, s]), first_seq, system_id, component_id, tally, preset)
            if pack and f:
                frames[k, s, :len(f)] = np.frombuffer(f, np.uint8)
                lengths[k, s] = len(f)
        st.store(states_out[s])
        alt[s] = st.alt
    return dict(records=out, frames=frames, lengths=lengths, states=states_out, tally=tally, alt=alt)


# ---- inputs ----

def synthetic_records(rng, kinds, frames_before=None):
    """RECORD_DTYPE [K, S] as a push with d_gyro = NULL leaves them, from kinds [K, S] of 'p' (published), 'f' (a first
    frame), 'h' (held), 'i' (idle).  The flow fields are arbitrary bits: the IMU call only carries them."""
    kinds = np.asarray(kinds)
    K, S = kinds.shape
    rec = np.zeros((K, S), RECORD_DTYPE)
    count = np.zeros(S, np.int64) if frames_before is None else np.array(frames_before, np.int64)
    for k in range(K):
        for s in range(S):
            kind = kinds[k, s]
            if kind == "i":
                rec[k, s]["quality"] = IDLE
                continue
            count[s] += 1
            r = rec[k, s]
            r["frame"] = count[s]
            if kind == "h":
                r["quality"] = HELD
            elif kind == "f":
                r["frame"] = 1
            else:
                r["quality"] = int(rng.integers(0, 256))
                r["dt_us"] = int(rng.integers(1, 200000))
                r["flow_x"], r["flow_y"] = rng.normal(0, 0.02, 2).astype(np.float32)
            if kind in "ph":
                r["pixel"] = np.frombuffer(rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), FLOW_DTYPE)[0]
    return rec


GARBAGE = (0xDEADBEEFDEADBEEF, 1e9, -1e9, float("nan"))   # a slot behind a round's count: never read as a sample


def pack_samples(per_round, M, S):
    """per_round[k][s]: a list of (t, x, y, z), at most M.  -> SAMPLE_DTYPE [K, M, S], unused slots holding GARBAGE."""
    K = len(per_round)
    a = np.zeros((K, M, S), SAMPLE_DTYPE)
    a["time_usec"], a["xgyro"], a["ygyro"], a["zgyro"] = GARBAGE
    a["reserved"] = 0x5A5A5A5A
    for k in range(K):
        for s in range(S):
            assert len(per_round[k][s]) <= M
            for j, (t, x, y, z) in enumerate(per_round[k][s]):
                a[k, j, s] = (t, x, y, z, 0)
    return a


FAMILY_S, FAMILY_K, FAMILY_M, FAMILY_FIRST_SEQ = 48, 16, 4, 250
SCENARIOS = 8


def family(seed=7):
    """The coverage family: 48 streams, 16 rounds, at most 4 samples per round, eight scenarios six times over with
    other rates and times.  Returns dict(samples, counts, times, records, states, first_seq).  The states are written
    directly (their layout is public): from a reset state AOF_TICK_NO_OFFSET cannot be reached, because the sample that
    first makes prev_time_usec non-zero also sets the offset -- it takes a caller that cleared the offset."""
    rng = np.random.default_rng(seed)
    S, K, M = FAMILY_S, FAMILY_K, FAMILY_M
    kinds = np.full((K, S), "p", dtype="<U1")
    counts = np.zeros((K, S), np.uint8)
    per_round = [[[] for _ in range(S)] for _ in range(K)]
    states = np.zeros(S, STATE_DTYPE)
    inf, nan = float("inf"), float("nan")
    for s in range(S):
        scenario = s % SCENARIOS
        clock = [1_000_000 + 977 * s]

        def tick(step=2500):
            clock[0] += step
            return clock[0]

        def rates():
            return tuple(float(v) for v in rng.normal(0, 1.5, 3).astype(np.float32))

        def normal(n):
            return [(tick(int(rng.integers(1800, 3300))),) + rates() for _ in range(n)]

        def put(k, samples, count=None, kind="p"):
            per_round[k][s] = samples
            counts[k, s] = len(samples) if count is None else count
            kinds[k, s] = kind

        if scenario == 0:
            # an ordinary camera: the offset learned from the first sample, a first frame that is sent, then the limiter's
            # rhythm (four held frames, one published), with sums left standing at the end
            put(0, normal(4), kind="f")
            for k in range(1, K):
                put(k, normal(3 + k % 2), kind="p" if k % 5 == 0 and k < 12 else "h")
        elif scenario == 1:
            # a first frame before any sample (stale), then a sent record; an idle round with samples; two takes with no
            # sample between them (stale) and a sent record behind them
            states[s]["offset_timestamp_usec"] = 5_000_000_000 + s
            put(0, [], kind="f")
            put(1, normal(4))
            put(2, normal(2), kind="i")
            put(3, normal(3))
            put(4, [])
            put(5, normal(1))
            for k in range(6, K):
                put(k, normal(int(rng.integers(0, M + 1))), kind="phi"[k % 3])
        elif scenario == 2:
            # the time edges: a step of exactly 50 000 us (rejected), 49 999 us (accepted), a time that runs backwards
            put(0, normal(2), kind="f")
            put(1, [(tick(50000),) + rates(), (tick(49999),) + rates()])
            put(2, [(tick(-30000),) + rates(), (tick(2500),) + rates()], kind="h")
            put(3, [(tick(60000),) + rates(), (tick(1),) + rates()])
            for k in range(4, K):
                put(k, normal(4), count=200 if k % 2 else M)      # counts above M count as M
        elif scenario == 3:
            # the rate edges, on each axis in turn: exactly 20 and -20 (rejected), the float below 20 (accepted), NaN, +-inf
            axis = (s // SCENARIOS) % 3

            def on_axis(v):
                r = list(rates())
                r[axis] = v
                return (tick(),) + tuple(r)

            put(0, normal(2), kind="f")
            put(1, [on_axis(20.0), on_axis(BELOW_20), on_axis(-20.0), on_axis(-BELOW_20)])
            put(2, [on_axis(nan), on_axis(inf), on_axis(-inf), on_axis(-19.5)])
            put(3, [on_axis(-nan), on_axis(1e30), on_axis(-0.0), on_axis(19.0)], kind="h")
            for k in range(4, K):
                put(k, normal(3), kind="ph"[k % 2])
        elif scenario == 4:
            # a sample with time 0 in front of everything: it changes nothing; and one in the middle: prev is 0 again, so
            # the sample behind it is rejected and the take behind that one is not stale
            put(0, [(0,) + rates()] + normal(3), kind="f")
            put(1, normal(2) + [(0,) + rates()])
            put(2, normal(3))
            for k in range(3, K):
                put(k, normal(int(rng.integers(1, M + 1))), kind="pih"[k % 3])
        elif scenario == 5:
            # a caller cleared the offset of a running stream (vehicle time lost): AOF_TICK_NO_OFFSET once, then the next
            # sample teaches a new offset
            states[s]["prev_time_usec"] = clock[0]
            states[s]["last_taken_time_usec"] = clock[0] - 2500
            states[s]["messages"] = 40 + s
            states[s]["gyro_x"], states[s]["gyro_y"], states[s]["gyro_z"] = rng.normal(0, 0.01, 3)
            put(0, [])
            put(1, normal(2))
            for k in range(2, K):
                put(k, normal(4), kind="hp"[k % 2])
        elif scenario == 6:
            # a preset offset and a record sent in every round: with first_seq 250 the sequence number wraps past 255
            states[s]["offset_timestamp_usec"] = (1 << 40) + 1000 * s
            put(0, normal(4), kind="f")
            for k in range(1, K):
                put(k, normal(1 + k % M))
        else:
            # long held stretches with full rounds (the sums of many samples, where the order of the additions shows),
            # idle rounds without samples
            states[s]["offset_timestamp_usec"] = 77
            put(0, normal(4), kind="f")
            for k in range(1, K):
                put(k, [] if k % 6 == 5 else normal(4), kind="i" if k % 6 == 5 else "p" if k == 9 else "h")
    records = synthetic_records(rng, kinds)
    times = (np.arange(K, dtype=np.uint64)[:, None] * np.uint64(13333) + np.arange(S, dtype=np.uint64)[None, :] * np.uint64(7))
    return dict(samples=pack_samples(per_round, M, S), counts=counts, times=times, records=records, states=states,
                first_seq=FAMILY_FIRST_SEQ)


def random_family(seed, S, K, M, counts="mixed", preset_every=3):
    """Random samples and records: rates from normal floats (a few beyond +-20), time steps from {1 .. 60 000} us, counts
    'mixed' (0 .. M and a few above), 'full' (None: M everywhere).  Streams start from reset states; every preset_every-th
    one has its offset preset."""
    rng = np.random.default_rng(seed)
    a = np.zeros((K, M, S), SAMPLE_DTYPE)
    steps = rng.integers(1, 60001, (K, M, S))
    short = rng.random((K, M, S)) < 0.8
    steps = np.where(short, rng.integers(1, 5000, (K, M, S)), steps)
    a["xgyro"], a["ygyro"], a["zgyro"] = (rng.normal(0, 6.0, (K, M, S)).astype(np.float32) for _ in range(3))
    a["reserved"] = rng.integers(0, 2 ** 32, (K, M, S), dtype=np.uint64).astype(np.uint32)
    c = None
    if counts == "mixed":
        c = rng.integers(0, M + 1, (K, S)).astype(np.uint8)
        c[rng.random((K, S)) < 0.05] = 255
    # times run on per stream over the samples that are really taken, so that most steps are short
    clock = rng.integers(1, 10 ** 9, S).astype(np.int64)
    for k in range(K):
        for s in range(S):
            n = M if c is None else min(int(c[k, s]), M)
            for j in range(M):
                if j < n:
                    clock[s] += steps[k, j, s]
                    a[k, j, s]["time_usec"] = clock[s]
                else:
                    a[k, j, s]["time_usec"] = GARBAGE[0]
    kinds = rng.choice(np.array(["p", "h", "i"]), (K, S), p=[0.45, 0.4, 0.15])
    kinds[0, rng.random(S) < 0.5] = "f"
    records = synthetic_records(rng, kinds)
    times = rng.integers(0, 2 ** 40, (K, S)).astype(np.uint64)
    states = np.zeros(S, STATE_DTYPE)
    states["offset_timestamp_usec"][::preset_every] = 1_600_000_000_000_000
    return dict(samples=a, counts=c, times=times, records=records, states=states, first_seq=int(rng.integers(0, 256)))
