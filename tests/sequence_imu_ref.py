"""The sequence pipeline's IMU call (include/aof_sequence_imu.h) as the SEQUENTIAL run it stands for: one stream of
tests/imu_ref.py (Stream, sample, take, frame -- the reference's highres_imu_msg_callback and send gates in plain Python
floats) walked frame by frame over a recording: the samples that arrived before a frame's callback, then, if calcFlow
published the frame, the take.  run() is that and nothing else; closed_form() is the parallel restatement the kernels use
("Sequence IMU"), written apart so that the two can be held against each other.  family() makes the
designed recordings whose census (OUTCOMES) covers every branch; designed() makes recordings of any size with numpy for
the device tests.  Nothing here touches the GPU or the library."""
import collections

import numpy as np

import imu_ref as imu
from imu_ref import BELOW_20, FRAME_BYTES, NO_OFFSET, SAMPLE_DTYPE, SENTINEL, STALE_GYRO, STATE_DTYPE

RECORD_DTYPE = np.dtype([("frame", "<u4"), ("quality", "<i4"), ("dt_us", "<i4"), ("flow_x", "<f4"), ("flow_y", "<f4"),
                         ("gyro_x", "<f4"), ("gyro_y", "<f4"), ("gyro_z", "<f4")])     # aof_seq_record
assert RECORD_DTYPE.itemsize == 32
SYSTEM_ID, COMPONENT_ID, FIRST_SEQ = 1, 100, 250
PRESET = (1 << 40) + 12345
LONG_WINDOW = 5000
M64 = imu.M64

# Everything the family must reach at least once; NO_OFFSET must never be reached (run() asserts it).
OUTCOMES = ("accepted", "rejected_prev_zero", "rejected_dt", "rejected_rate", "nan", "plus_inf", "minus_inf", "time_backwards",
            "time_zero", "offset_learned", "offset_preset_sent", "stale_before_any_sample", "stale_no_sample", "stale_equal_times",
            "sent_after_stale", "first_frame_sent", "seq_wrapped", "empty_window", "long_window", "sample_end_above_T")


def recording(n, published, samples, sample_end, offset0=0, first_seq=FIRST_SEQ, seed=0, name=""):
    """A recording as the call sees it: n frames, `published` the increasing frame indices calcFlow published (one record
    each, as a records-only aof_sequence_device call leaves them: zero gyro sums; the flow fields are arbitrary bits the
    call only carries), samples SAMPLE_DTYPE [T] or a list of (t, x, y, z), sample_end [n]."""
    rng = np.random.default_rng(seed)
    if not isinstance(samples, np.ndarray):
        a = np.zeros(len(samples), SAMPLE_DTYPE)
        for i, s in enumerate(samples):
            a[i] = (s[0], s[1], s[2], s[3], 0x5A5A5A5A)
        samples = a
    published = np.asarray(published, np.uint32)
    M = len(published)
    assert M <= n and (np.diff(published.astype(np.int64)) > 0).all() and (M == 0 or published[-1] < n)
    records = np.zeros(n, RECORD_DTYPE)
    records["frame"][:M] = published
    records["quality"][:M] = rng.integers(0, 256, M)
    records["dt_us"][:M] = rng.integers(1, 200000, M)
    records["flow_x"][:M], records["flow_y"][:M] = rng.normal(0, 0.02, (2, M)).astype(np.float32)
    if M and published[0] == 0:     # frame 0: calcFlow returned 0 with its outputs untouched
        records[0] = (0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
    times = (np.arange(n, dtype=np.uint64) * np.uint64(13333)) + np.uint64(rng.integers(0, 1000))
    sample_end = np.asarray(sample_end, np.uint32)
    assert sample_end.shape == (n,)
    return dict(name=name, n=n, M=M, times=times, samples=samples, sample_end=sample_end, records=records,
                offset0=int(offset0), first_seq=int(first_seq))


def run(r, tally=None):
    """The sequential run.  Returns dict(records [n] with the first M completed, frames u8 [n, 56] filled with SENTINEL behind
    every length and where nothing is sent, lengths u8 [n] (0 behind M too), sent, state STATE_DTYPE [1], tally)."""
    tally = collections.Counter() if tally is None else tally
    n, M, T = r["n"], r["M"], len(r["samples"])
    zero = np.zeros(1, STATE_DTYPE)
    zero["offset_timestamp_usec"] = r["offset0"]
    st = imu.Stream(zero[0])
    records = r["records"].copy()
    frames = np.full((n, FRAME_BYTES), SENTINEL, np.uint8)
    lengths = np.zeros(n, np.uint8)
    record_of = {int(f): m for m, f in enumerate(records["frame"][:M])}
    taken, since_take = 0, 0
    for k in range(n):
        end = int(r["sample_end"][k])
        tally["sample_end_above_T"] += end > T
        end = min(end, T)
        assert end >= taken, "sample_end must not decrease"
        for i in range(taken, end):
            s = r["samples"][i]
            imu.sample(st, int(s["time_usec"]), float(s["xgyro"]), float(s["ygyro"]), float(s["zgyro"]), tally)
        since_take += end - taken
        taken = end
        m = record_of.get(k)
        if m is None:
            continue        # calcFlow returned -1: nothing is taken, the sums run on
        before_any = st.prev == 0 and st.integrated + st.rejected == 0
        rec = records[m]
        f = imu.take(st, rec, int(r["times"][k]), r["first_seq"], SYSTEM_ID, COMPONENT_ID, tally, r["offset0"] != 0)
        tally["empty_window"] += since_take == 0
        tally["long_window"] += since_take >= LONG_WINDOW
        if int(rec["quality"]) == STALE_GYRO and not before_any:
            tally["stale_no_sample" if since_take == 0 else "stale_equal_times"] += 1
        tally["first_frame_sent"] += bool(f) and k == 0
        since_take = 0
        if f:
            frames[m, :len(f)] = np.frombuffer(f, np.uint8)
            lengths[m] = len(f)
    assert tally["no_offset"] == 0, "AOF_TICK_NO_OFFSET is unreachable from the reset state"
    state = np.zeros(1, STATE_DTYPE)
    st.store(state[0])
    return dict(records=records, frames=frames, lengths=lengths, sent=st.messages, state=state, tally=tally)


def closed_form(r):
    """The parallel restatement: every record from its own window alone.  Returns dict(quality [M], gyro float32 [M, 3], sent
    bool [M], seq [M], offset: the vehicle time each sent record used, state: dict of the final state's fields)."""
    n, M, T = r["n"], r["M"], len(r["samples"])
    t = [int(v) for v in r["samples"]["time_usec"]]
    rates = [tuple(float(s[a]) for a in ("xgyro", "ygyro", "zgyro")) for s in r["samples"]]
    E = lambda m: 0 if m < 0 else min(T, int(r["sample_end"][int(r["records"]["frame"][m])]))
    p = lambda e: t[e - 1] if e > 0 else 0
    first = next((i for i in range(T) if t[i] != 0), T)

    def accepted(i):        # pointwise: the sample and the time in front of it
        prev = t[i - 1] if i > 0 else 0
        dt = float((t[i] - prev) & M64) / 1e6
        return prev != 0 and dt < 0.05 and all(abs(v) < 20.0 for v in rates[i])

    def window(lo, hi):     # the accepted samples of [lo, hi), added in order from 0.0
        g = [0.0, 0.0, 0.0]
        for i in range(lo, hi):
            if accepted(i):
                dt = float((t[i] - t[i - 1]) & M64) / 1e6
                for a in range(3):
                    g[a] = g[a] + rates[i][a] * dt
        return g

    quality, gyro, sent, seq, offsets = [], [], [], [], []
    messages = 0
    for m in range(M):
        lo, hi = E(m - 1), E(m)
        gyro.append(np.array(window(lo, hi), "<f8").astype("<f4"))
        offset = r["offset0"] if r["offset0"] else (t[first] if first < hi else 0)
        q = int(r["records"]["quality"][m])
        if p(hi) == p(lo):
            q = STALE_GYRO
        elif offset == 0:
            q = NO_OFFSET
        quality.append(q)
        sent.append(q >= 0)
        seq.append((r["first_seq"] + messages) & 0xFF)
        offsets.append(offset)
        messages += q >= 0
    e_last = min(T, int(r["sample_end"][n - 1]))
    n_acc = sum(accepted(i) for i in range(e_last))
    state = dict(g=window(E(M - 1), e_last), prev_time_usec=p(e_last), last_taken_time_usec=p(E(M - 1)),
                 offset_timestamp_usec=r["offset0"] if r["offset0"] else (t[first] if first < e_last else 0),
                 messages=messages, samples_integrated=n_acc, samples_rejected=e_last - n_acc, dropped=M - messages)
    return dict(quality=np.array(quality, np.int32), gyro=np.array(gyro, np.float32).reshape(M, 3), sent=np.array(sent, bool),
                seq=np.array(seq, np.uint8), offset=offsets, state=state)


# ---- recordings ----

def _rates(rng):
    return tuple(float(v) for v in rng.normal(0, 1.5, 3).astype(np.float32))


def _steady(rng, start, count, step=4000):
    """`count` samples at 250 Hz with a little jitter, from time `start` on."""
    out, t = [], start
    for _ in range(count):
        t += int(rng.integers(step - 200, step + 200))
        out.append((t,) + _rates(rng))
    return out


def family(seed=11):
    """The designed recordings of the CPU tests and the sanitized program: small ones, one branch of the census each, one long
    window, and small designed() recordings of every sample design with both offset forms."""
    rng = np.random.default_rng(seed)
    inf, nan = float("inf"), float("nan")
    out = []
    # an ordinary flight: samples before frame 0 (the first frame is sent), the offset learnt from the first of them, every
    # other frame published
    s = _steady(rng, 1_000_000, 40)
    out.append(recording(8, [0, 2, 4, 6, 7], s, [3, 8, 13, 18, 23, 28, 33, 38], name="ordinary"))
    # a preset offset; frame 0 before any sample (stale), then sent; two takes with no sample between them; sent behind them
    s = _steady(rng, 2_000_000, 20)
    out.append(recording(7, [0, 1, 2, 3, 5, 6], s, [0, 4, 4, 9, 12, 12, 20], offset0=PRESET, name="preset-stale"))
    # the time and rate edges: steps of 50 000 us (rejected) and 49 999 us, time running backwards, 20 rad/s, NaN, +-inf
    t0 = 3_000_000
    s = [(t0, 0.1, 0.2, 0.3), (t0 + 4000, 0.1, -0.2, 0.3), (t0 + 54000, 1.0, 1.0, 1.0), (t0 + 103999, 1.0, 1.0, 1.0),
         (t0 + 73999, 0.5, 0.5, 0.5), (t0 + 77999, 20.0, 0.0, 0.0), (t0 + 81999, 0.0, -20.0, 0.0), (t0 + 85999, BELOW_20, 0.0, -BELOW_20),
         (t0 + 89999, nan, 0.0, 0.0), (t0 + 93999, 0.0, inf, 0.0), (t0 + 97999, 0.0, 0.0, -inf), (t0 + 101999, 1e30, 0.0, 0.0),
         (t0 + 105999, -0.0, 19.0, -19.5)]
    out.append(recording(5, [0, 1, 3, 4], s, [2, 5, 9, 11, 13], name="edges"))
    # times of 0: in front of everything (they teach nothing: a record behind them alone is stale although samples arrived),
    # and in the middle (prev is 0 again: the next sample is rejected, and the take behind a 0 is not stale)
    s = [(0,) + _rates(rng) for _ in range(3)] + _steady(rng, 4_000_000, 6) + [(0,) + _rates(rng)] + _steady(rng, 4_100_000, 6)
    out.append(recording(6, [0, 1, 2, 3, 4, 5], s, [2, 3, 7, 10, 12, 16], name="zero-times"))
    # duplicate times: the window's last sample carries the time of the previous window's last one -- stale by equal times
    s = _steady(rng, 5_000_000, 6)
    s += [(s[-1][0],) + _rates(rng) for _ in range(3)] + _steady(rng, s[-1][0], 5)
    out.append(recording(5, [0, 1, 2, 4], s, [4, 6, 9, 11, 14], offset0=PRESET, name="duplicates"))
    # a record sent for every frame: with first_seq 250 the sequence number wraps past 255
    s = _steady(rng, 6_000_000, 36)
    out.append(recording(12, list(range(12)), s, [3 * (k + 1) for k in range(12)], name="wrap"))
    # a stalled chain: one window of 6 000 samples, an empty one in front of it, sample_end above T, samples left in the tail
    s = _steady(rng, 7_000_000, 6100)
    out.append(recording(5, [0, 1, 2, 3], s, [10, 10, 6010, 6050, 9000], name="long-window"))
    # no sample at all, and no record published behind frame 0
    out.append(recording(3, [0, 2], [], [0, 0, 5], name="no-samples"))
    out.append(recording(4, [0], _steady(rng, 8_000_000, 9), [2, 4, 6, 9], name="one-record"))
    for design in DESIGNS:
        for offset0 in (0, PRESET):
            out.append(designed(23, 29, 160, design, offset0, seed=int(rng.integers(1 << 30))))
    return out


DESIGNS = ("steady", "edges", "duplicates", "stalled")


def designed(M, n, T, design, offset0, seed=0):
    """A recording of any size, made with numpy: M records over n frames (frame 0 among them), T samples at about 250 Hz.
      steady      plain samples, windows of random lengths (many empty where T < M), the last frames' sample_end above T
      edges       steps of 50 ms and more, steps back, rates at and beyond 20 rad/s, NaN and infinities
      duplicates  runs of equal times, times of 0 in front and in the middle
      stalled     the first half of the frames see no sample, the next frame sees all of them: one long window"""
    assert design in DESIGNS and 1 <= M <= n
    rng = np.random.default_rng([seed, M, n, T, DESIGNS.index(design), 1 if offset0 else 0])
    a = np.zeros(T, SAMPLE_DTYPE)
    step = rng.integers(3800, 4200, T)
    rates = rng.normal(0, 1.5, (T, 3)).astype(np.float32)
    if design == "edges":
        u = rng.random(T)
        step[u < 0.06] = rng.choice(np.array([50000, 49999, 60000, 500000]), int((u < 0.06).sum()))
        step[(u >= 0.06) & (u < 0.08)] = -30000
        v = rng.random(T)
        specials = np.array([20.0, -20.0, BELOW_20, -BELOW_20, np.nan, np.inf, -np.inf, 1e30], np.float32)
        hit = np.flatnonzero(v < 0.08)
        rates[hit, rng.integers(0, 3, hit.size)] = rng.choice(specials, hit.size)
    if design == "duplicates":
        step[rng.random(T) < 0.5] = 0
    time = 1_000_000 + 977 * (seed % 1000) + np.cumsum(step)
    if design == "duplicates" and T:
        time[:min(T, 1 + T // 50)] = 0
        time[rng.random(T) < 0.01] = 0
    a["time_usec"] = time.astype(np.int64).view(np.uint64)
    a["xgyro"], a["ygyro"], a["zgyro"] = rates[:, 0], rates[:, 1], rates[:, 2]
    a["reserved"] = 0x5A5A5A5A
    if design == "stalled":
        end = np.where(np.arange(n) <= n // 2, 0, T).astype(np.int64)
    else:
        end = np.sort(rng.integers(0, T + 1, n))
        end[n - 1 - n // 8:] = T + rng.integers(0, 3) * 7      # (non-decreasing: the sorted values are <= T)
    published = np.concatenate([[0], np.sort(rng.choice(np.arange(1, n), M - 1, replace=False))]) if n > 1 else np.array([0])
    return recording(n, published, a, end, offset0=offset0, seed=seed, name=f"{design}-M{M}-n{n}-T{T}-{'preset' if offset0 else 'learnt'}")


def random_recording(seed, max_per_frame=None):
    """A small random recording: duplicate times, leading zero times, gaps of 50 ms and more, rates of 20 rad/s and above,
    empty windows; max_per_frame bounds the samples that arrive between two frames."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    per_frame = rng.integers(0, (max_per_frame - 3 if max_per_frame else 24) + 1, n)    # (up to 3 more reach the last frame)
    per_frame[rng.random(n) < 0.3] = 0
    T_seen = int(per_frame.sum())
    T = T_seen + int(rng.integers(0, 4))            # a few samples behind the last frame
    step = rng.integers(1, 5000, T)
    step[rng.random(T) < 0.1] = rng.integers(50000, 200000)
    step[rng.random(T) < 0.15] = 0
    time = int(rng.integers(1, 10 ** 9)) + np.cumsum(step)
    time[:int(rng.integers(0, 4))] = 0
    rates = rng.normal(0, 7.0, (T, 3)).astype(np.float32)
    a = np.zeros(T, SAMPLE_DTYPE)
    a["time_usec"], a["xgyro"], a["ygyro"], a["zgyro"] = time, rates[:, 0], rates[:, 1], rates[:, 2]
    end = np.cumsum(per_frame)
    if rng.random() < 0.3:
        end[-1] = T + 5
    published = [k for k in range(n) if k == 0 or rng.random() < 0.4]
    return recording(n, published, a, end, offset0=PRESET if seed % 3 == 0 else 0, first_seq=int(rng.integers(0, 256)), seed=seed,
                     name=f"random-{seed}")
