"""The sequence pipeline's rate limiter as a host model (tests/test_sequence_limiter_ref.py, tests/test_gpu_sequence_limiter.py).
k_sequence.hip finds the frames that publish with a forward scan per frame, pointer quadrupling over sequence_rounds(n)
rounds and one lane per publication; this walks the chain one publication at a time, as the facade does, in plain
Python/numpy.  Here: the model (limiter_model, wire_of), the recording the tests feed (frame_ids, flows_of, gyro_of) and the
time-stamp DESIGNS -- named pure functions that build time stamps for a chain stated in advance, at the counts and gaps
where a round, a workgroup or the scan window changes.  Nothing here touches the GPU."""
from collections import namedtuple

import numpy as np

from mavlink_model import py_frame

WINDOW = 4096          # kLimitScanFrames: a publication must come within this many frames of the previous one
STALLED = 1            # AOF_SEQ_STATUS_STALLED
STEP = 66667           # us: the shortest whole step that passes the 15 Hz period, float32(1e6) / float32(15) = 66666.664
RATE = 15
RECORD_DTYPE = np.dtype([("frame", "<u4"), ("quality", "<i4"), ("dt_us", "<i4"), ("flow_x", "<f4"), ("flow_y", "<f4"),
                         ("gyro_x", "<f4"), ("gyro_y", "<f4"), ("gyro_z", "<f4")])
FLOW_DTYPE = np.dtype([("flow_x", "<f4"), ("flow_y", "<f4"), ("count", "<u4"), ("quality", "u1"), ("flags", "u1"),
                       ("pred_x", "i1"), ("pred_y", "i1")])          # aof_flow
DARK = 64              # frame id of the all-zero frame; ids 0..63 are the frames of one synth.make_sequence


# ---- the model -------------------------------------------------------------------------------------------------------
def period_of(rate):
    return np.float32(1e6) / np.float32(rate)


def _successor(t32, last_i, last_t, period):
    """First j in last_i + 1 .. min(last_i + WINDOW, n - 1) with float32(uint32(t_j - last_t)) > period, or None."""
    stop = min(last_i + WINDOW, len(t32) - 1) + 1
    lo, step = last_i + 1, 64
    while lo < stop:
        hi = min(lo + step, stop)
        hit = np.flatnonzero((t32[lo:hi] - t32.dtype.type(last_t)).astype(np.float32) > period)
        if hit.size:
            return lo + int(hit[0])
        lo, step = hi, step * 4
    return None


def chain_of(times, rate):
    """(frames that publish behind frame 0, status): the walk from (last_i, last_t) = (0, 0) -- the start has time 0, not
    frame 0's time."""
    n = len(times)
    if rate <= 0:
        return list(range(1, n)), 0
    t32 = (np.asarray(times, np.int64) & 0xFFFFFFFF).astype(np.uint32)
    period = period_of(rate)
    chain, last_i, last_t = [], 0, 0
    while True:
        j = _successor(t32, last_i, last_t, period)
        if j is None:
            return chain, (STALLED if last_i + 1 + WINDOW < n else 0)
        chain.append(j)
        last_i, last_t = j, int(t32[j])


def _in_order(values, dtype):
    """0 + v0 + v1 + ... with every add rounded to dtype, in this order (np.cumsum does not reassociate)."""
    return np.cumsum(np.concatenate([np.zeros((1,) + values.shape[1:], dtype), values.astype(dtype)]), axis=0, dtype=dtype)[-1]


def limiter_model(times, flows, gyro, rate, fx, fy, angle=None):
    """(records [RECORD_DTYPE], status) of a recording.  times int64 [n]; flows [n - 1] with flow_x, flow_y, quality
    (pair k = frames k, k + 1); gyro float32 [n, >= 3] or None; angle: orc.angle unless given."""
    if angle is None:
        from oracle import pyoracle
        angle = pyoracle.angle
    n = len(times)
    chain, status = chain_of(times, rate)
    recs = np.zeros(len(chain) + 1 if n else 0, RECORD_DTYPE)
    if n == 0:
        return recs, status
    t32 = (np.asarray(times, np.int64) & 0xFFFFFFFF).astype(np.uint32)
    g = np.zeros((n, 3), np.float32) if gyro is None else np.asarray(gyro, np.float32)[:, :3]
    recs[0] = (0, 0, 0, 0.0, 0.0) + tuple(g[0])
    fxs, fys, q = flows["flow_x"].astype(np.float32), flows["flow_y"].astype(np.float32), flows["quality"].astype(np.int64)
    last_i, last_t = 0, 0
    for m, k in enumerate(chain, 1):
        dt = (int(t32[k]) - last_t) & 0xFFFFFFFF               # the u32 difference, read as int32
        dt -= (dt >> 31) << 32
        if rate <= 0:
            px, py, quality = fxs[k - 1], fys[k - 1], int(q[k - 1])
        else:
            seg = slice(last_i, k)                              # pairs last_i .. k - 1 = frames last_i + 1 .. k
            valid = q[seg] > 0
            px, py = _in_order(fxs[seg][valid], np.float32), _in_order(fys[seg][valid], np.float32)
            count = int(valid.sum())
            quality = int(np.floor(np.float32(q[seg][valid].sum()) / np.float32(count))) if count else 0
        gsum = _in_order(g[last_i + 1:k + 1], np.float64)
        recs[m] = (k, quality, dt, np.float32(angle(float(px), fx)), np.float32(angle(float(py), fy)),
                   np.float32(gsum[0]), np.float32(gsum[1]), np.float32(gsum[2]))
        last_i, last_t = k, int(t32[k])
    return recs, status


def wire_of(recs, times, offset, first_seq):
    """The OPTICAL_FLOW_RAD frame of every record from the tests' own serializer; nothing is sent while offset == 0."""
    if not offset:
        return []
    return [py_frame(offset, int(times[int(r["frame"])]), int(r["dt_us"]), float(r["flow_x"]), float(r["flow_y"]),
                     (float(r["gyro_x"]), float(r["gyro_y"]), float(r["gyro_z"])), int(r["quality"]), (first_seq + m) & 0xFF)
            for m, r in enumerate(recs)]


def records_of_replay(recs):
    """sequence_ref.replay's record tuples as RECORD_DTYPE."""
    out = np.zeros(len(recs), RECORD_DTYPE)
    for m, r in enumerate(recs):
        out[m] = r
    return out


# ---- the recording ---------------------------------------------------------------------------------------------------
def default_dark(n):
    """A few dark stretches of a recording of n frames: three frames at a third, nine at two thirds."""
    if n < 24:
        return ()
    return ((n // 3, n // 3 + 3), (2 * n // 3, 2 * n // 3 + 9))


def frame_ids(n, dark=None):
    """Frame k of the recording is base[k % 64], or the all-zero frame (DARK) inside a dark stretch [a, b)."""
    ids = (np.arange(n) % 64).astype(np.int64)
    for a, b in default_dark(n) if dark is None else dark:
        ids[a:b] = DARK
    return ids


def frames_of(base, ids):
    return np.concatenate([base, np.zeros((1,) + base.shape[1:], base.dtype)])[ids]


def flows_of(orc, po, base, ids, memo):
    """The oracle's flow record of every pair of consecutive frames, memoised in memo by (id, id): at most 64 distinct
    textured pairs plus the ones with a dark frame."""
    codes = ids[:-1] * (DARK + 1) + ids[1:]
    full = frames_of(base, np.arange(DARK + 1))
    for code in np.unique(codes):
        key = (int(code) // (DARK + 1), int(code) % (DARK + 1))
        if key not in memo:
            memo[key] = np.frombuffer(orc.flow_pair(po, full[key[0]], full[key[1]])["flow"].tobytes(), FLOW_DTYPE)[0]
    table = np.zeros((DARK + 1) * (DARK + 1), FLOW_DTYPE)
    for key, f in memo.items():
        table[key[0] * (DARK + 1) + key[1]] = f
    return table[codes]


def gyro_of(n, seed=5):
    g = np.zeros((n, 4), np.float32)
    g[:, :3] = np.random.default_rng(seed).normal(0, 0.004, (n, 3)).astype(np.float32)
    g[:, 3] = np.float32(0.0133)
    return g


# ---- the designs -----------------------------------------------------------------------------------------------------
# times: int64 [n].  chain: the frames behind frame 0 the design was built to publish.  status: 0 or STALLED.
# census: records = len(chain) + 1 (frame 0's; the END node's rank), rounds = the smallest R with 4^R > n
# (sequence_rounds), largest_gap = the most frames from one chain node to the next (the start counts as frame 0),
# tail = frames behind the last publication.
Design = namedtuple("Design", "times rate chain status census")


def rounds_of(n):
    r = 0
    while 4 ** r <= n:
        r += 1
    return r


def census_of(chain, n):
    nodes = [0] + [int(k) for k in chain]
    return dict(records=len(nodes), rounds=rounds_of(n), largest_gap=max(np.diff(nodes), default=0), tail=n - 1 - nodes[-1])


def _design(times, rate, chain, status=0):
    times = np.asarray(times, np.int64)
    return Design(times, rate, [int(k) for k in chain], status, census_of(chain, len(times)))


def every_frame(n, rate=RATE):
    """n frames 66 667 us apart: at 15 Hz every frame passes the period -- through the scan, not the rate <= 0 shortcut."""
    return _design(np.arange(n, dtype=np.int64) * STEP, rate, range(1, n))


def strided(g, records, tail):
    """A publication every g frames: frame j g at j * 66 667 us, the frames behind it one microsecond apart; `records`
    records in all, `tail` unpublished frames behind the last."""
    n = (records - 1) * g + 1 + tail
    k = np.arange(n, dtype=np.int64)
    pubs = np.minimum(k // g, records - 1)
    return _design(pubs * STEP + (k - pubs * g), RATE, range(g, (records - 1) * g + 1, g))


def gap(i, frames, after):
    """Frames 1 .. i publish; then a gap of `frames` frames (i + 1 .. i + frames - 1 held one microsecond behind i) to
    frame i + frames, which passes the period and has `after` - 1 publishing frames behind it.  4096 frames are inside the
    scan window, 4097 are not: the chain ends at i and, with frames beyond the window, STALLED is raised."""
    n = i + frames + after
    t = np.empty(n, np.int64)
    t[:i + 1] = np.arange(i + 1) * STEP
    t[i + 1:i + frames] = i * STEP + 1
    t[i + frames:] = i * STEP + STEP * (1 + np.arange(after))
    found = frames <= WINDOW
    chain = list(range(1, i + 1)) + (list(range(i + frames, n)) if found else [])
    return _design(t, RATE, chain, 0 if found else STALLED)


def held_to_end(i, held):
    """Frames 1 .. i publish and the `held` frames behind i never pass the period, to the end of the recording: with
    n = i + 1 + 4096 the window reaches the end and no flag is raised, one frame more and it is."""
    n = i + 1 + held
    t = np.empty(n, np.int64)
    t[:i + 1] = np.arange(i + 1) * STEP
    t[i + 1:] = i * STEP + 1 + np.arange(held) // 64
    return _design(t, RATE, range(1, i + 1), STALLED if held > WINDOW else 0)


def off_chain_stall():
    """No chain node stalls, but 154 frames that are NOT on the chain (the first is frame 51) find no successor inside
    their own window and have frames beyond it.  The chain is 1 .. 10, 4001, 4301 .. 5999: status 0."""
    n = 6000
    t = np.empty(n, np.int64)
    k = np.arange(n, dtype=np.int64)
    t[:11] = 70000 * k[:11]
    T = int(t[10])
    t[11:4001] = T + 1 + (k[11:4001] - 11) // 40
    t[4001] = T + 66667
    t[4002:4301] = T + 66668
    t[4301:] = T + 133400 + 70000 * (k[4301:] - 4301)
    return _design(t, RATE, list(range(1, 11)) + [4001] + list(range(4301, n)))


def off_chain_stallers(times, rate):
    """The frames whose OWN window holds no successor although frames lie beyond it (the chain or not)."""
    t32 = (np.asarray(times, np.int64) & 0xFFFFFFFF).astype(np.uint32)
    n = len(t32)
    return [i for i in range(n) if i + 1 + WINDOW < n and _successor(t32, i, int(t32[i]) if i else 0, period_of(rate)) is None]


def irregular(seed, n=9000, low=1, high=300):
    """Seeded gaps of low .. high frames between publications."""
    rng = np.random.default_rng(seed)
    pubs = [0]
    while True:
        nxt = pubs[-1] + int(rng.integers(low, high + 1))
        if nxt >= n:
            break
        pubs.append(nxt)
    pubs = np.array(pubs, np.int64)
    k = np.arange(n, dtype=np.int64)
    j = np.searchsorted(pubs, k, side="right") - 1
    return _design(j * STEP + (k - pubs[j]), RATE, pubs[1:])


def _every_third(n):
    return np.arange(n, dtype=np.int64) * 30000           # 15 Hz: 30 000 and 60 000 us are held, 90 000 publish


def period_edges(n=300):
    """{name: Design}: the period's edge and the 32-bit time arithmetic.  b = 151 is the frame behind a publication."""
    k = np.arange(n, dtype=np.int64)
    b = 151
    out = {
        # float32(1e6) / float32(15) = 66666.664: 66 666 is held (every second frame publishes), 66 667 is not
        "gap-66666": _design(k * 66666, 15, range(2, n, 2)),
        "gap-66667": _design(k * 66667, 15, range(1, n)),
        # 1e6 / 10 = 100000 exactly, and the comparison is `>`
        "gap-100000-rate-10": _design(k * 100000, 10, range(2, n, 2)),
        # the start has time 0: frame 1 at 70 000 us publishes although it is 30 000 us behind frame 0
        "first-time-not-zero": _design(40000 + k * 30000, 15, range(1, n, 3)),
        "rate-0": _design(k * 13333, 0, range(1, n)),
        "rate-200": _design(k * 13333, 200, range(1, n)),            # 13 333 > 5 000: every frame
        "every-third": _design(_every_third(n), 15, range(3, n, 3)),
    }
    back = _every_third(n)
    back[b:] -= 1_000_000                                # time steps back: the u32 difference is huge, dt < 0
    out["backwards-step"] = _design(back, 15, list(range(3, b, 3)) + list(range(b, n, 3)))
    wrap = _every_third(n)
    wrap[b - 1:] += (1 << 32) - int(wrap[b - 1]) - 20000              # 150 publishes 20 ms before the u32 wraps
    out["u32-wrap"] = _design(wrap, 15, range(3, n, 3))
    jump = _every_third(n)
    jump[b:] += 1 << 31                                               # dt = int32(2^31 + 30 000) < 0
    out["jump-2-to-31"] = _design(jump, 15, list(range(3, b, 3)) + list(range(b, n, 3)))
    return out
