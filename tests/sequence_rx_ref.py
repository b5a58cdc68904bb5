"""The sequence pipeline's MAVLink receive (include/aof_sequence_mavlink_rx.h) as plain-Python models, written from the
header's text: the SEQUENTIAL model on tests/mavlink_rx_ref.Parser (one cap for the log, the delivery position of every
sample, sample_end, the 128 state bytes); the CLOSED FORM the kernels compute (the successor of an idle position, the set
reached from 0, a chunk's exit table, the entry chain by doubling over the tables); csrc/aof_sequence_rx_plan.hpp restated;
and the family of designed logs the tests share, with the census of the edges each one reaches."""
import functools
import struct

import numpy as np

import mavlink_rx_ref as rx
from mavlink_model import x25

C = 4096                  # the plan's chunk
FRAME_MAX = 280
TABLE = 288
END = 0xFFFF
SENTINEL = 0xEE
SAMPLE_DTYPE, STATE_DTYPE = rx.SAMPLE_DTYPE, rx.STATE_DTYPE
IN_PROGRESS = np.dtype([("time_usec", "<u8"), ("gyro", "<u4", (3,)), ("msgid", "<u4"), ("pos", "<u2"), ("crc", "<u2"), ("start", "u1"),
                        ("len", "u1"), ("incompat", "u1"), ("check", "u1"), ("reserved", "u1", (64,))])
assert IN_PROGRESS.itemsize == 96


# ---- the sequential model ---------------------------------------------------------------------------------------------
def in_progress(p):
    """The private 96 bytes of a parser's state: the frame being received, all zero when idle."""
    m = np.zeros(1, IN_PROGRESS)
    if p.phase == "idle":
        return m.tobytes()
    head, v2 = p.head, p.v2
    m["start"] = 0xFD if v2 else 0xFE
    m["pos"] = len(head) + len(p.payload) + len(p.check) + p.signature
    m["len"] = head[0] if head else 0
    m["incompat"] = head[1] if v2 and len(head) >= 2 else 0
    ids = head[6:9] if v2 else head[4:5]
    msgid = sum(b << (8 * i) for i, b in enumerate(ids))
    m["msgid"] = msgid
    crc = x25(bytes(head))
    if p.phase != "header" and msgid == rx.HIGHRES_IMU:      # only a wanted message's payload is looked at
        crc = x25(bytes(p.payload), crc)
        m["time_usec"] = int.from_bytes(bytes(p.payload[:8]), "little")
        gyro = bytearray(12)
        got = bytes(p.payload[20:32])
        gyro[:len(got)] = got
        m["gyro"] = struct.unpack("<3I", bytes(gyro))
        if p.check:
            crc = x25(bytes([rx.HIGHRES_IMU_EXTRA]), crc)
            ok = p.check[0] == (crc & 0xFF)
            if len(p.check) == 2:
                ok = ok and p.check[1] == (crc >> 8)
            m["check"] = int(ok)
    m["crc"] = crc
    return m.tobytes()


def model(log, byte_end, max_samples):
    """The call on a log (bytes) -> dict: samples SAMPLE_DTYPE [written], total (imu_samples), delivered (the position behind
    each sample's last byte, all of them), sample_start (where each of those frames began), sample_end uint32 [n], state (128
    bytes), parser."""
    log = bytes(log)
    p, out, delivered, started, start = rx.Parser(), [], [], [], 0
    for i in range(len(log)):
        before, idle = p.c["imu_samples"], p.phase == "idle"
        p.feed(log[i:i + 1], max_samples, out)
        if idle and p.phase != "idle":
            start = i
        if p.c["imu_samples"] != before:
            delivered.append(i + 1)
            started.append(start)
    samples = np.zeros(len(out), SAMPLE_DTYPE)
    for j, (t, x, y, z) in enumerate(out):
        samples[j]["time_usec"] = t
        samples[j:j + 1].view(np.uint32).reshape(6)[2:5] = (x, y, z)
    d = np.array(delivered, np.int64)
    q = np.minimum(np.asarray(byte_end, np.int64), len(log))
    sample_end = np.minimum(np.searchsorted(d, q, side="right"), max_samples).astype(np.uint32)
    state = np.zeros(1, STATE_DTYPE)
    for n in rx.COUNTERS:
        state[n] = p.c[n]
    return dict(samples=samples, total=p.c["imu_samples"], delivered=d, sample_start=np.array(started, np.int64), sample_end=sample_end,
                state=state.tobytes()[:32] + in_progress(p), parser=p)


# ---- the closed form --------------------------------------------------------------------------------------------------
def successor(log, p):
    """Where the idle machine is next after position p < N, or END where N cuts the frame that starts at p."""
    N, b = len(log), log[p]
    if b not in (0xFD, 0xFE):
        return p + 1
    if p + 1 >= N:
        return END
    size = 8 + log[p + 1]
    if b == 0xFD:
        if p + 2 >= N:
            return END
        if log[p + 2] & ~1:
            return p + 3
        size = 12 + log[p + 1] + (13 if log[p + 2] & 1 else 0)
    return p + size if p + size <= N else END


def reached(log):
    """(the positions reached from 0 in front of N, the position N cuts a frame at or None)."""
    out, p, N = [], 0, len(log)
    while p < N:
        out.append(p)
        nxt = successor(log, p)
        if nxt == END:
            return out, p
        p = nxt
    return out, None


def exit_table(log, c):
    """Chunk c's table: for entry offset o < TABLE the offset at which the chain enters chunk c + 1, or END."""
    N, base, table = len(log), c * C, []
    stop, leaves = min(base + C, N), {}          # leaves: position of the chunk -> where the chain from it leaves the chunk, or END
    for o in range(TABLE):
        p, path = base + o, []
        while p != END and p < stop and p not in leaves:
            path.append(p)
            p = successor(log, p)
        if p != END and p < stop:
            p = leaves[p]
        for q in path:
            leaves[q] = p
        table.append(END if p == END else min(max(p - base - C, 0), TABLE - 1))
    return table


def entry_chain(log):
    """entry[c] by the kernels' doubling over the tables, and the largest entry offset met."""
    chunks = -(-len(log) // C)
    if chunks == 0:
        return []
    F = [exit_table(log, c) for c in range(chunks)]
    entry = [0] + [None] * (chunks - 1)
    k = 0
    while (1 << k) < chunks:
        step = 1 << k
        for c in range(min(step, chunks - step)):
            entry[c + step] = END if entry[c] == END else F[c][entry[c]]
        F = [[v if v == END or c + step >= chunks else F[c + step][v] for v in F[c]] for c in range(chunks)]
        k += 1
    return entry


def entry_chain_serial(log):
    """entry[c] read off the reached set: the first idle position at or behind c * C, END behind the frame N cuts."""
    chunks = -(-len(log) // C)
    starts, cut = reached(log)
    pos = np.array(starts + ([] if cut is not None else [len(log)]), np.int64)
    entry = []
    for c in range(chunks):
        i = int(np.searchsorted(pos, c * C))
        entry.append(END if i == len(pos) else int(pos[i]) - c * C)
    return entry


# ---- the plan ------------------------------------------------------------------------------------------------------------
def plan(n_bytes):
    """csrc/aof_sequence_rx_plan.hpp: dict(chunks, rounds, scan_entries, total_bytes), or None for a refused N."""
    if n_bytes < 0 or n_bytes > 0x7FFFFFFF:
        return None
    r256 = lambda v: (v + 255) // 256 * 256
    chunks = -(-n_bytes // C)
    rounds = 0
    while (1 << rounds) < chunks:
        rounds += 1
    scan, e = [], chunks
    while e > 0:
        scan.append(e)
        if e <= 256 or len(scan) == 3:
            break
        e = -(-e // 256)
    sums = sum(r256(4 * (scan[l] if l < len(scan) else 0)) for l in range(3))
    total = r256(32) + r256(2 * chunks) + r256(4 * chunks) + sums + 2 * r256(chunks * TABLE * 2)
    return dict(chunks=chunks, rounds=rounds, scan_entries=scan, total_bytes=total, static_lds=20 * 1024)


# ---- the designed logs ---------------------------------------------------------------------------------------------------
SIG = bytes(range(1, 14))


def imu(i, **kw):
    return rx.imu_payload(1_000_000 + 4000 * i, 0.25 * (i % 7) - 0.5, -0.125 * (i % 5), 1.0 + i % 3, **kw)


def healthy(rng, n_bytes, start=0):
    """About n_bytes of a healthy connection: HIGHRES_IMU in both versions with other traffic between."""
    out, size, i = [], 0, start
    while size < n_bytes:
        c = int(rng.integers(0, 10))
        f = (rx.frame_v2(rx.HIGHRES_IMU, imu(i), seq=i & 255) if c < 5 else rx.frame_v1(rx.HIGHRES_IMU, imu(i), seq=i & 255) if c < 7 else
             rx.frame_v2(int(rng.choice([0, 30, 33, 74])), rng.integers(0, 256, int(rng.integers(1, 60)), dtype=np.uint8).tobytes(), seq=i & 255))
        out.append(f)
        size += len(f)
        i += 1
    return b"".join(out)


def placed(rng, frame, at, tail=600):
    """A log in which `frame` starts at position `at`: healthy traffic, junk that starts nothing up to `at`, the frame, traffic."""
    head = healthy(rng, max(at - 400, 0)) if at > 500 else b""
    assert len(head) <= at
    return head + rx.junk(rng, at - len(head)) + frame + healthy(rng, tail, start=500)


def mixed(rng, n_bytes, kind=4):
    items, size = [], 0
    while size < n_bytes:
        more = rx.stream_items(rng, kind, 40)
        items += more
        size += sum(len(i) for i in more)
    return b"".join(items)[:n_bytes]


def _logs():
    """(name, log, claimed edges, capacity rule, frame-count rule)."""
    rng = np.random.default_rng(2024)
    out = []
    add = lambda name, log, edges=(), cap="total+1", frames="edges": out.append((name, bytes(log), set(edges), cap, frames))
    f1 = rx.frame_v1(rx.HIGHRES_IMU, imu(0))
    f2 = rx.frame_v2(rx.HIGHRES_IMU, imu(1), signature=SIG)
    f3 = rx.frame_v2(rx.HIGHRES_IMU, imu(2))
    three, s2, body = f1 + f2 + f3, len(f1), len(f2) - 13 - 2 - 10
    for n in (0, 1, 2, 3):
        add(f"N={n}", three[:n], {f"N={n}", "cut v1 header"} if n in (1, 2, 3) else {f"N={n}"})
    cuts = {"N at a frame's last byte": s2, "N one short of a frame's last byte": s2 - 1, "cut v2 header in front of incompat": s2 + 2,
            "cut v2 header behind incompat": s2 + 3, "cut payload": s2 + 10 + 5, "cut behind the first check byte": s2 + 10 + body + 1,
            "cut behind the second check byte": s2 + 10 + body + 2, "cut signature": s2 + 10 + body + 2 + 6,
            "cut v2 at its start byte": s2 + 1}
    for edge, n in cuts.items():
        add(edge, three[:n], {edge})
    base = mixed(rng, C + 1)
    for n, name in ((C - 1, "N=C-1"), (C, "N=C"), (C + 1, "N=C+1")):
        add(name, base[:n], {name})
    # seams
    sample_v2 = rx.frame_v2(rx.HIGHRES_IMU, imu(7), seq=7)
    for back in (1, 2, 3):
        add(f"v2 start at C-{back}", placed(rng, sample_v2, C - back), {f"start at C-{back}"})
        add(f"v1 start at 2C-{back}", placed(rng, f1, 2 * C - back), {f"start at C-{back}"})
    hdr_and_body = len(sample_v2) - 2
    add("check bytes either side of the seam", placed(rng, sample_v2, C - hdr_and_body - 1), {"check bytes either side of the seam"})
    add("both check bytes behind the seam", placed(rng, sample_v2, C - hdr_and_body), {"check bytes behind the seam"})
    longest = rx.frame_v2(rx.HIGHRES_IMU, imu(9) + bytes(rng.integers(1, 256, 255 - 62, dtype=np.uint8)), truncate=False, signature=SIG)
    assert len(longest) == FRAME_MAX
    add("longest frame starts at C-1", placed(rng, longest, C - 1), {"entry offset 279"})
    rejected = rx.frame_v2(rx.HIGHRES_IMU, imu(3), incompat=2)
    add("rejected incompat at C+1", placed(rng, rejected, C - 1), {"rejected incompat at the seam"})
    add("rejected incompat at C", placed(rng, rejected, C - 2), {"rejected incompat at the seam"})
    add("frame ends at the seam", placed(rng, sample_v2, C - len(sample_v2)), {"entry offset 0"})
    # chains
    add("all zero", bytes(2 * C + 5), {"all zero"}, frames=1)
    add("all 0xFE", b"\xfe" * (2 * C + 5), {"all 0xFE"}, frames=1)
    add("all 0xFD", b"\xfd" * (2 * C + 5), {"all 0xFD"}, frames=1)
    add("start bytes inside payloads", mixed(rng, 3 * C - 9), {"start bytes inside payloads"})
    add("a false start swallows frames", rx.junk(rng, 37) + b"\xfe\xff" + healthy(rng, 900), {"false start of len 255"})
    add("second half junk", healthy(rng, C + 100) + rx.junk(rng, C + 200, starts=True), {"second half junk"})
    # chunk counts
    for chunks in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33):
        log = (healthy(rng, chunks * C) if chunks > 9 else mixed(rng, chunks * C, kind=4 if chunks % 2 else 3))[:chunks * C - 11 * (chunks % 3)]
        add(f"{chunks} chunks", log, {f"{chunks} chunks"}, frames="spread")
    # content
    add("every kind of frame", mixed(rng, 2 * C + 777),
        {"bad check", "105 with len 0", "105 with len < 32", "105 with 63 bytes", "v1 sample", "v2 sample", "signed sample",
         "other message len 0", "other message len 255"})
    add("dense short samples", mixed(rng, C + 300, kind=1), {"105 with len 0", "105 with len < 32"})
    # capacity
    cap_log = healthy(rng, C + 500)
    for cap in ("total-1", "total", "total+1", "1"):
        add(f"max_samples {cap}", cap_log, {f"max_samples {cap}"}, cap=cap)
    # frame counts of the last pass, and a byte_end in no order
    for n in (0, 1, 63, 64, 65, 257):
        add(f"n_frames {n}", cap_log, {f"n_frames {n}"}, frames=n)
    add("decreasing byte_end", healthy(rng, 3 * C), {"decreasing byte_end"}, frames="decreasing")
    return out


def _byte_end(rule, N, delivered, rng):
    d = [int(v) for v in delivered]
    if rule == "edges":
        picks = d[:2] + d[len(d) // 2:len(d) // 2 + 1] + d[-1:]
        vals = [0, N, N + 5, 0xFFFFFFFF] + [v for p in picks for v in (p, p - 1, p, p + 1)] + [N // 2, N // 2]
        return np.array(sorted(min(v, 0xFFFFFFFF) for v in vals), np.uint32)
    if rule == "spread":
        return np.linspace(0, N + 3, 40).astype(np.uint32)
    if rule == "decreasing":
        vals = np.concatenate([np.linspace(N + 40, 0, 90), rng.integers(0, 2 * N + 2, 60), [0xFFFFFFFF, 0, N, 0xFFFFFFF0]])
        return vals.astype(np.uint32)
    return np.linspace(0, N, int(rule)).astype(np.uint32) if int(rule) > 1 else np.array([N // 2] * int(rule), np.uint32)


@functools.lru_cache(maxsize=None)
def cases():
    """The family: dicts with name, log (uint8 array), byte_end (uint32 [n]), max_samples, claimed (edge names), want (the
    sequential model's result)."""
    rng = np.random.default_rng(7)
    out = []
    for name, log, claimed, cap, frames in _logs():
        free = model(log, [], 1 << 30)
        total = free["total"]
        M = max(1, {"total-1": total - 1, "total": total, "total+1": total + 1, "1": 1}[cap])
        byte_end = _byte_end(frames, len(log), free["delivered"], rng)
        out.append(dict(name=name, log=np.frombuffer(log, np.uint8).copy(), byte_end=byte_end, max_samples=M, claimed=claimed,
                        want=model(log, byte_end, M)))
    return out


EDGES = (["N=0", "N=1", "N=2", "N=3", "N at a frame's last byte", "N one short of a frame's last byte", "cut v1 header",
          "cut v2 at its start byte", "cut v2 header in front of incompat", "cut v2 header behind incompat", "cut payload", "cut behind the first check byte",
          "cut behind the second check byte", "cut signature", "N=C-1", "N=C", "N=C+1", "start at C-1", "start at C-2", "start at C-3",
          "check bytes either side of the seam", "check bytes behind the seam", "entry offset 279", "rejected incompat at the seam", "entry offset 0", "all zero",
          "all 0xFE", "all 0xFD", "start bytes inside payloads", "false start of len 255", "second half junk", "bad check",
          "105 with len 0", "105 with len < 32", "105 with 63 bytes", "v1 sample", "v2 sample", "signed sample", "other message len 0",
          "other message len 255", "max_samples total-1", "max_samples total", "max_samples total+1", "max_samples 1", "byte_end 0",
          "byte_end N", "byte_end above N", "byte_end at a delivery", "byte_end one short of a delivery", "byte_end repeated",
          "decreasing byte_end"] + [f"{c} chunks" for c in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33)] +
         [f"n_frames {n}" for n in (0, 1, 63, 64, 65, 257)])


def census(case):
    """The edges a case reaches, found on the model and the closed form (not taken from its name)."""
    log, want, N = bytes(case["log"]), case["want"], len(case["log"])
    p, ev, got = want["parser"], want["parser"].events, set()
    starts, cut = reached(log)
    chunks = -(-N // C)
    entry = entry_chain_serial(log)
    if N <= 3:
        got.add(f"N={N}")
    for n, name in ((C - 1, "N=C-1"), (C, "N=C"), (C + 1, "N=C+1")):
        if N == n:
            got.add(name)
    got.add(f"{chunks} chunks")
    if cut is not None:
        v2, taken = log[cut] == 0xFD, N - cut
        if not v2 and taken <= 5:
            got.add("cut v1 header")
        if v2 and taken == 1:
            got.add("cut v2 at its start byte")
        if v2 and taken == 2:
            got.add("cut v2 header in front of incompat")
        if v2 and taken == 3:
            got.add("cut v2 header behind incompat")
        if p.phase == "payload" and p.payload:
            got.add("cut payload")
        if p.phase == "check" and len(p.check) == 1:
            got.add("cut behind the first check byte")
        if p.phase == "signature" and p.signature == 0:
            got.add("cut behind the second check byte")
        if p.phase == "signature" and p.signature > 0:
            got.add("cut signature")
        if taken >= 3 and successor(log + b"\x00", cut) == N + 1:     # (one more byte, whatever it is, ends the frame)
            got.add("N one short of a frame's last byte")
    frames_at = [s for s in starts if log[s] in (0xFD, 0xFE)]
    if cut is None and frames_at and successor(log, frames_at[-1]) == N and N - frames_at[-1] > 3:
        got.add("N at a frame's last byte")
    for s in frames_at:
        for back in (1, 2, 3):
            if s % C == C - back and s + 12 < N:
                got.add(f"start at C-{back}")
        nxt = successor(log, s)
        if nxt != END and nxt - s > 3:
            if nxt % C == 1 and nxt - s > 8:
                got.add("check bytes either side of the seam") if not (log[s] == 0xFD and log[s + 2] & 1) else None
            if nxt % C == 2 and nxt - s > 8 and not (log[s] == 0xFD and log[s + 2] & 1):
                got.add("check bytes behind the seam")
            if nxt % C == 0:
                got.add("entry offset 0")
        if nxt != END and nxt - s == 3 and log[s] == 0xFD and (s + 2) % C in (0, 1):
            got.add("rejected incompat at the seam")
        if log[s] == 0xFE and s + 1 < N and log[s + 1] == 0xFF and nxt != END and sum(1 for q in range(s + 1, nxt) if log[q] in (0xFD, 0xFE)) > 4:
            got.add("false start of len 255")
        if nxt != END and any(log[q] in (0xFD, 0xFE) for q in range(s + 1, nxt)):
            got.add("start bytes inside payloads")
    if 279 in entry:
        got.add("entry offset 279")
    if N > C and not any(log):
        got.add("all zero")
    if N > C and set(log) == {0xFE}:
        got.add("all 0xFE")
    if N > C and set(log) == {0xFD}:
        got.add("all 0xFD")
    if N > 2 * C and p.c["skipped"] > C // 2 and p.c["frames"] > 10:
        got.add("second half junk")
    for event, edge in (("bad check", "bad check"), ("len < 32 sample", "105 with len < 32"), ("extended sample", "105 with 63 bytes"),
                        ("sample v1", "v1 sample"), ("sample v2", "v2 sample")):
        if event in ev:
            got.add(edge)
    got |= _content(log, frames_at)
    total, M = want["total"], case["max_samples"]
    for name, value in (("total-1", total - 1), ("total", total), ("total+1", total + 1), ("1", 1)):
        if M == value and total >= 2:
            got.add(f"max_samples {name}")
    be, d = case["byte_end"].astype(np.int64), set(int(v) for v in want["delivered"])
    got.add(f"n_frames {len(be)}")
    if (be == 0).any():
        got.add("byte_end 0")
    if (be == N).any():
        got.add("byte_end N")
    if (be > N).any():
        got.add("byte_end above N")
    if any(int(v) in d for v in be):
        got.add("byte_end at a delivery")
    if any(int(v) + 1 in d for v in be):
        got.add("byte_end one short of a delivery")
    if len(be) > len(set(be.tolist())):
        got.add("byte_end repeated")
    if len(be) > 2 and (np.diff(be) < 0).any():
        got.add("decreasing byte_end")
    return got


def _content(log, frames_at):
    """Edges of single frames, read off the reached frames' headers."""
    got, N = set(), len(log)
    for s in frames_at:
        nxt = successor(log, s)
        if nxt == END or nxt - s == 3:
            continue
        v2 = log[s] == 0xFD
        ln = log[s + 1]
        msgid = log[s + 7] | log[s + 8] << 8 | log[s + 9] << 16 if v2 else log[s + 5]
        if msgid == rx.HIGHRES_IMU:
            if ln == 0:
                got.add("105 with len 0")
            if v2 and log[s + 2] & 1:
                got.add("signed sample")
        else:
            if ln == 0:
                got.add("other message len 0")
            if ln == 255:
                got.add("other message len 255")
    return got


# ---- the deep family: more than one trip of a workgroup's lanes, full lists, more than one scan group ---------------------------
FREE = 1 << 30            # a capacity no log of the family reaches
GROUP = 256               # chunks per workgroup of a scan level (kSeqRxThreads)
LIST = 512                # kSeqRxChunkSamples


def capped(free, N, byte_end, M):
    """The result at capacity M from the result of the same N bytes without a cap.  The header's rule is one cap for the log: sample j
    is kept iff j < M, the others are counted in `overflowed`, sample_end is clipped to M, and nothing else depends on M."""
    q = np.minimum(np.asarray(byte_end, np.int64), N)
    sample_end = np.minimum(np.searchsorted(free["delivered"], q, side="right"), M).astype(np.uint32)
    state = np.frombuffer(free["state"], STATE_DTYPE).copy()
    state["overflowed"] = max(0, free["total"] - M)
    return dict(free, samples=free["samples"][:M], sample_end=sample_end, state=state.tobytes())


@functools.lru_cache(maxsize=None)
def _free(log):
    return model(log, [], FREE)


def tiled_expectation(tile, N, byte_end, M):
    """The TILE RULE: what model(log, byte_end, M) gives for log = the tile repeated and cut at N, without walking the log.  The tile
    is whole frames, so the machine is idle at both of its ends (asserted) and every repeat is parsed as the first one was: with
    m = the model of one tile, J = N // T whole tiles and the model of the cut one behind them, every counter is J times m's plus the
    cut one's, the deliveries and the samples are m's at j * T for every j and then the cut one's, and the state in progress is the cut
    one's.  tests/test_sequence_rx_ref.py holds the rule to the sequential model on a log of three tiles and a cut."""
    tile = bytes(tile)
    T = len(tile)
    J, r = divmod(N, T)
    m, t = _free(tile), _free(tile[:r])
    assert m["parser"].phase == "idle", "a tile is whole frames"
    at = np.arange(J, dtype=np.int64)[:, None] * T
    every = lambda key: np.concatenate([(at + m[key][None, :]).reshape(-1), J * T + t[key]])
    whole, state = np.frombuffer(m["state"], STATE_DTYPE), np.frombuffer(t["state"], STATE_DTYPE).copy()
    for n in rx.COUNTERS:
        state[n] = J * int(whole[n][0]) + int(state[n][0])
    free = dict(samples=np.concatenate([np.tile(m["samples"], J), t["samples"]]), total=J * m["total"] + t["total"],
                delivered=every("delivered"), sample_start=every("sample_start"), state=state.tobytes(), parser=t["parser"])
    return capped(free, N, byte_end, M)


def tiled_log(tile, N):
    """The tile repeated and cut at N, as a uint8 array."""
    t = np.frombuffer(bytes(tile), np.uint8)
    return np.tile(t, N // len(t) + 1)[:N]


def _odd(rng, tile):
    """(an odd tile meets the chunk grid at another phase every time)"""
    return tile if len(tile) % 2 else tile + rx.junk(rng, 1)


def sparse_tile(rng, n_bytes):
    """About n_bytes of whole frames: MAVLink 2 frames of other messages with 200 to 255 payload bytes, a HIGHRES_IMU frame about
    every 2 KiB, one frame with a bad check, one start with an incompat flag the parser cannot size, a few junk bytes; odd."""
    parts, size, due, k = [], 0, 0, 0
    while size < n_bytes:
        if k == 3:
            f = rx.frame_v2(rx.HIGHRES_IMU, imu(5), seq=5, bad=True)
        elif k == 7:
            f = rx.frame_v2(rx.HIGHRES_IMU, imu(3), incompat=2) + rx.junk(rng, 5)
        elif size >= due:
            f = rx.frame_v2(rx.HIGHRES_IMU, imu(k), seq=k & 255)
            due += 2048
        else:
            f = rx.frame_v2(int(rng.choice([0, 30, 33, 74])), rng.integers(0, 256, int(rng.integers(200, 256)), dtype=np.uint8).tobytes(),
                            seq=k & 255, truncate=False)
        parts.append(f)
        size += len(f)
        k += 1
    return _odd(rng, b"".join(parts))


@functools.lru_cache(maxsize=None)
def _short(seq):
    return rx.frame_v1(rx.HIGHRES_IMU, b"", seq=seq)


def dense(first, n):
    """n HIGHRES_IMU frames of len 0, 8 bytes each, back to back: each delivers a sample of zeros."""
    return b"".join(_short(i & 255) for i in range(first, first + n))


def _seam_frames():
    rng = np.random.default_rng(99)
    longest = rx.frame_v2(rx.HIGHRES_IMU, imu(9) + bytes(rng.integers(1, 256, 255 - 62, dtype=np.uint8)), truncate=False, signature=SIG)
    assert len(longest) == FRAME_MAX
    return (("v2 sample", rx.frame_v2(rx.HIGHRES_IMU, imu(7), seq=7)), ("longest frame", longest), ("v1 sample", rx.frame_v1(rx.HIGHRES_IMU, imu(0))))


def _one_chunk_of(n):
    def build(rng):
        head = healthy(rng, C - 400)
        assert len(head) <= C
        return head + rx.junk(rng, C - len(head)) + dense(0, n) + rx.junk(rng, C - 8 * n) + healthy(rng, C, start=700)
    return build


def _chunks_of_healthy(chunks):
    n = chunks * C - 11 * (chunks % 3)
    if chunks * C <= 1 << 20 or chunks == 257:       # the sequential model is the expectation up to about 1 MiB
        return lambda rng: healthy(rng, chunks * C)[:n]
    return lambda rng: (_odd(rng, healthy(rng, 6 * C + 1000)), n)


@functools.lru_cache(maxsize=None)
def _deep_specs():
    """name -> (claimed edges, build(rng) -> the log's bytes or (tile, N), capacity rule, byte_end rule); nothing is built here."""
    out = {}

    def add(name, edges, build, cap="total+1", ends="every"):
        assert name not in out
        out[name] = (set(edges), build, cap, ends)
    every = "byte_end at every delivery"
    add("512 per chunk, aligned", {"512 samples start in one chunk", "two full lists side by side", every, "byte_end in no order",
                                   "byte_end = c*C with a delivery at c*C", "3 chunks"}, lambda rng: dense(0, 1027), ends="every, shuffled")
    add("512 per chunk, last one crosses the seam",
        {"full list and a delivery behind the seam", every, "byte_end between a seam and a delivery behind it of a frame that began in front of it"},
        lambda rng: rx.junk(rng, 5) + dense(0, 1027))
    add("256 in a chunk", {"samples of a chunk = one trip", every}, _one_chunk_of(256))
    add("257 in a chunk", {"samples of a chunk = one trip + 1", every}, _one_chunk_of(257))
    add("full chunk between empty ones", {"count 0 next to count 512", every}, lambda rng: bytes(C) + dense(0, LIST) + bytes(C) + dense(LIST, LIST))
    for cap, edge in ((256, "capacity = one trip"), (257, "capacity ends inside the second trip"), (511, "capacity ends inside the second trip"),
                      (512, "capacity = one full list"), (513, "capacity one past a full list"), (512 + 300, "capacity ends inside the second trip"),
                      ("total-1", None)):
        add(f"512 per chunk, max_samples {cap}", {every} | ({edge} if edge else set()), lambda rng: dense(0, 1027), cap=cap)
    between = "byte_end between a seam and a delivery behind it of a frame that began in front of it"
    behind = {0: {"a frame from in front of a seam delivered at it", "byte_end = c*C with a delivery at c*C"},
              1: {"a frame from in front of a seam delivered one behind it", between}, 279: {"a delivery 279 behind a seam"}}
    for what, frame in _seam_frames():
        for seam in (1, 2):
            for off in (0, 1, 279):
                edges = behind[off] | {every} | ({"a frame from in front of a seam delivered 279 behind it", between} if len(frame) == FRAME_MAX and off == 279 else set())
                add(f"{what} delivered at {seam if seam > 1 else ''}C+{off}", edges,
                    lambda rng, frame=frame, at=seam * C + off - len(frame): placed(rng, frame, at))
    add("N cuts a frame that began in the chunk in front", {"entry END for a chunk with bytes in front of N", "state in progress with pos >= 100", every},
        lambda rng: placed(rng, _seam_frames()[1][1], C - 1)[:C + 100])
    second, sums1 = "a chunk with samples in the second group", "sample_end read through sums[1]"
    add("256 chunks", {"256 chunks"}, _chunks_of_healthy(256), ends="groups")
    add("257 chunks", {"257 chunks", "two scan levels", second}, _chunks_of_healthy(257), ends="groups")
    add("512 chunks", {"512 chunks", "two scan levels", second, sums1}, _chunks_of_healthy(512), ends="groups")
    add("513 chunks", {"513 chunks", "two scan levels", second, sums1, "a chunk with samples in the third group"}, _chunks_of_healthy(513), ends="groups")
    return out


# the largest, on one buffer: three scan levels and 17 entry rounds; two levels with every group full and 16 rounds; and one chunk
# more than the first, since the last pass reads the scan at the chunk IN FRONT of byte_end's: with 65 537 chunks (as with 257) only
# the pack pass reads the second entry of the top level
BIG = {"65537 chunks less 1234 bytes": (65537 * C - 1234, {"three scan levels", "a chunk with samples behind 65536 chunks", "17 entry rounds", "65537 chunks"}),
       "65536 chunks": (65536 * C, {"two scan levels", "16 entry rounds, every group full", "65536 chunks"}),
       "65538 chunks less 1234 bytes": (65538 * C - 1234, {"three scan levels", "sample_end read through sums[2]", "17 entry rounds", "65538 chunks"})}


def deep_names():
    return list(_deep_specs())


@functools.lru_cache(maxsize=1)
def big_log():
    """(the tile, the tile repeated up to the larger of the two N)."""
    tile = sparse_tile(np.random.default_rng(65537), 7 * C)
    return tile, tiled_log(tile, max(n for n, _ in BIG.values()))


def _deep_ends(rule, N, delivered, rng, span):
    d = np.asarray(delivered, np.int64)
    if rule.startswith("every"):           # every delivery, the position in front of it and the one behind it; the ends; every seam
        vals = np.concatenate([d - 1, d, d + 1, [0, N, N + 5], np.arange(0, N + 1, C)])
        vals = rng.permutation(vals) if rule.endswith("shuffled") else np.sort(vals)
        return vals.astype(np.uint32)
    # "groups": spread over the log; around every multiple of `span` bytes, a chunk behind it (from there on the last pass reads the
    # scan of the chunk in front through the next group's entry), and around the first delivery behind each of those
    marks = np.array([g * span + at + k for g in range(N // span + 1) for at in (0, C) for k in (-1, 0, 1)], np.int64)
    marks = marks[marks >= 0]
    i = np.searchsorted(d, marks, side="right")
    nxt = d[i[i < len(d)]]
    n_lin = 600 - 2 * len(marks) if span > GROUP * C else 300 - 2 * len(marks)
    return np.concatenate([np.linspace(0, N + 3, n_lin).astype(np.int64), marks, nxt - 1, nxt, nxt + 1]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def deep_case(name):
    """One case of the deep family, in the shape of cases()'s: name, log, byte_end, max_samples, claimed, want -- the sequential
    model's result where the log is small, tiled_expectation's elsewhere (want["tiled"])."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name in BIG:
        N, claimed = BIG[name]
        tile, log = big_log()
        built, log, cap, ends, span = (tile, N), log[:N], "total+1", "groups", GROUP * GROUP * C
    else:
        claimed, build, cap, ends = _deep_specs()[name]
        built, span = build(rng), GROUP * C
        log = tiled_log(*built) if isinstance(built, tuple) else np.frombuffer(built, np.uint8).copy()
    tiled = isinstance(built, tuple)
    free = tiled_expectation(built[0], built[1], [], FREE) if tiled else model(built, [], FREE)
    total, N = free["total"], len(log)
    M = max(1, {"total-1": total - 1, "total+1": total + 1}.get(cap, cap))
    byte_end = _deep_ends(ends, N, free["delivered"], rng, span)
    return dict(name=name, log=log, byte_end=byte_end, max_samples=M, claimed=claimed, want=capped(free, N, byte_end, M),
                tile=built[0] if tiled else None)


def deep_cases():
    """The deep family up to 513 chunks (the two of BIG are built by name: deep_case(name))."""
    return [deep_case(name) for name in deep_names()]


DEEP_EDGES = (["512 samples start in one chunk", "two full lists side by side", "full list and a delivery behind the seam",
               "samples of a chunk = one trip", "samples of a chunk = one trip + 1", "count 0 next to count 512", "capacity = one trip",
               "capacity ends inside the second trip", "capacity = one full list", "capacity one past a full list", "byte_end at every delivery",
               "byte_end between a seam and a delivery behind it of a frame that began in front of it", "byte_end = c*C with a delivery at c*C",
               "byte_end in no order", "a frame from in front of a seam delivered at it", "a frame from in front of a seam delivered one behind it",
               "a frame from in front of a seam delivered 279 behind it", "a delivery 279 behind a seam",
               "entry END for a chunk with bytes in front of N", "state in progress with pos >= 100", "two scan levels",
               "a chunk with samples in the second group", "a chunk with samples in the third group", "sample_end read through sums[1]",
               "three scan levels", "a chunk with samples behind 65536 chunks", "sample_end read through sums[2]", "17 entry rounds",
               "16 entry rounds, every group full"] + [f"{c} chunks" for c in (3, 256, 257, 512, 513, 65536, 65537, 65538)])


def deep_census(case):
    """The edges a deep case reaches, found on its expectation (where every sample's frame starts and is delivered, the state in
    progress) and the plan, not taken from its name."""
    N, want, M = len(case["log"]), case["want"], case["max_samples"]
    P = plan(N)
    chunks, levels = P["chunks"], len(P["scan_entries"])
    d, s, total = want["delivered"], want["sample_start"], want["total"]
    counts = np.bincount(s // C, minlength=chunks)          # samples whose frames start in chunk c: the kernels' count[c]
    first = np.concatenate([[0], np.cumsum(counts)])        # and in front of chunk c: the scan
    be = case["byte_end"].astype(np.int64)
    got = {f"{chunks} chunks"}
    full, none = counts == LIST, counts == 0
    assert counts.max() <= LIST
    if full.any():
        got.add("512 samples start in one chunk")
    if (full[:-1] & full[1:]).any():
        got.add("two full lists side by side")
    if (none[:-1] & full[1:]).any() and (full[:-1] & none[1:]).any():
        got.add("count 0 next to count 512")
    if (counts == GROUP).any():
        got.add("samples of a chunk = one trip")
    if (counts == GROUP + 1).any():
        got.add("samples of a chunk = one trip + 1")
    if any(d[first[c + 1] - 1] > (c + 1) * C for c in np.flatnonzero(full)):
        got.add("full list and a delivery behind the seam")
    if M < total:
        c = int(np.searchsorted(first, M, side="right")) - 1       # the chunk of the first sample that is not kept
        j = M - int(first[c])                                      # and its place in that chunk's list
        if j > GROUP:
            got.add("capacity ends inside the second trip")
        if j == GROUP:
            got.add("capacity = one trip")
        if j == 0 and c > 0 and full[c - 1]:
            got.add("capacity = one full list")
        if j == 1 and c > 0 and full[c - 1]:
            got.add("capacity one past a full list")
    ends = set(be.tolist())
    if len(d) and all(v in ends for v in np.concatenate([d - 1, d, d + 1]).tolist()):
        got.add("byte_end at every delivery")
    if len(be) > 2 and (np.diff(be) < 0).any():
        got.add("byte_end in no order")
    seam = (s // C + 1) * C                                  # the seam behind each sample's start
    ordered = np.sort(be)
    i = np.searchsorted(ordered, seam)                       # the first byte_end at or behind that seam: in front of the delivery?
    if (ordered[np.minimum(i, len(ordered) - 1)] < d)[i < len(ordered)].any():
        got.add("byte_end between a seam and a delivery behind it of a frame that began in front of it")
    if any(int(v) in ends for v in d[d % C == 0]):
        got.add("byte_end = c*C with a delivery at c*C")
    for off, edge in ((0, "at it"), (1, "one behind it"), (279, "279 behind it")):
        if (d - seam == off).any():
            got.add("a frame from in front of a seam delivered " + edge)
    if (d % C == 279).any():
        got.add("a delivery 279 behind a seam")
    rest = np.frombuffer(want["state"][32:], IN_PROGRESS)[0]
    if rest["start"]:
        cut = N - int(rest["pos"]) - 1                        # where the frame that N cuts began (pos: the bytes behind its start byte)
        if cut // C < (N - 1) // C:
            got.add("entry END for a chunk with bytes in front of N")
        if rest["pos"] >= 100:
            got.add("state in progress with pos >= 100")
    got |= {2: {"two scan levels"}, 3: {"three scan levels"}}.get(levels, set())
    if P["rounds"] == 17:
        got.add("17 entry rounds")
    if P["rounds"] == 16 and chunks == GROUP * GROUP:
        got.add("16 entry rounds, every group full")
    if levels > 1:
        groups = np.add.reduceat(counts, np.arange(0, chunks, GROUP))
        assert (groups[:chunks // GROUP] > 0).all(), "every full group holds samples: a dropped group term would go unseen otherwise"
        q = np.minimum(be, N)
        c0 = np.maximum(np.minimum(q // C, chunks - 1) - 1, 0)          # the first of the two chunks the last pass searches
        unclipped = want["sample_end"] < M
        if counts[GROUP:2 * GROUP].any():
            got.add("a chunk with samples in the second group")
        if counts[2 * GROUP:3 * GROUP].any():
            got.add("a chunk with samples in the third group")
        if ((c0 >= GROUP) & unclipped).any():
            got.add("sample_end read through sums[1]")
        if levels > 2 and counts[GROUP * GROUP:].any():
            got.add("a chunk with samples behind 65536 chunks")
        if levels > 2 and ((c0 >= GROUP * GROUP) & unclipped).any():
            got.add("sample_end read through sums[2]")
    return got
