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
    each sample's last byte, all of them), sample_end uint32 [n], state (128 bytes), parser."""
    log = bytes(log)
    p, out, delivered = rx.Parser(), [], []
    for i in range(len(log)):
        before = p.c["imu_samples"]
        p.feed(log[i:i + 1], max_samples, out)
        if p.c["imu_samples"] != before:
            delivered.append(i + 1)
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
    return dict(samples=samples, total=p.c["imu_samples"], delivered=d, sample_end=sample_end,
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
    for o in range(TABLE):
        p = base + o
        while p < min(base + C, N):
            p = successor(log, p)
            if p == END:
                break
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
