"""A plain-Python model of the stream bank's MAVLink receive as include/aof.h words it ("the stream bank's MAVLink
receive"), written from the text and not from the C++ step: a parser with named phases, one byte at a time.  Beside it
the generators the tests share: HIGHRES_IMU frames of both wire versions (truncated, extended, signed), frames of other
messages, junk, and the coverage family -- per-stream byte streams cut into rounds at every staging edge."""
import struct

import numpy as np

from mavlink_model import x25

HIGHRES_IMU, HIGHRES_IMU_EXTRA = 105, 93
PIECE = 128          # what the kernel stages per stream at a time: lengths around its multiples are edges
SENTINEL = 0xA5

SAMPLE_DTYPE = np.dtype([("time_usec", "<u8"), ("xgyro", "<f4"), ("ygyro", "<f4"), ("zgyro", "<f4"), ("reserved", "<u4")])
PUBLIC_DTYPE = np.dtype([("bytes", "<u8"), ("frames", "<u4"), ("imu_samples", "<u4"), ("bad_check", "<u4"),
                         ("overflowed", "<u4"), ("skipped", "<u4"), ("rejected_flags", "<u4")])
STATE_DTYPE = np.dtype(PUBLIC_DTYPE.descr + [("in_progress", "u1", (96,))])
assert SAMPLE_DTYPE.itemsize == 24 and PUBLIC_DTYPE.itemsize == 32 and STATE_DTYPE.itemsize == 128
COUNTERS = PUBLIC_DTYPE.names


# ---- generators ----------------------------------------------------------------------------------------------------
def imu_payload(t, x, y, z, rest=0.0, ext=None):
    """HIGHRES_IMU's 62 bytes (63 with the `id` extension): time, acc x/y/z, gyro x/y/z, mag x/y/z, abs and diff
    pressure, pressure altitude, temperature, fields_updated; `rest` fills what the receive does not read."""
    p = struct.pack("<Q13fH", t, rest, rest, rest, x, y, z, rest, rest, rest, rest, rest, rest, rest, 0)
    return p if ext is None else p + bytes([ext])


def frame_v1(msgid, payload, seq=0, sysid=1, compid=1, extra=HIGHRES_IMU_EXTRA, bad=False):
    body = bytes([len(payload), seq, sysid, compid, msgid]) + bytes(payload)
    crc = x25(body + bytes([extra])) ^ (0x0100 if bad else 0)
    return b"\xfe" + body + bytes([crc & 0xFF, crc >> 8])


def frame_v2(msgid, payload, seq=0, sysid=1, compid=1, extra=HIGHRES_IMU_EXTRA, incompat=0, compat=0, truncate=True,
             signature=None, bad=False):
    """A MAVLink 2 frame; truncate: trailing zero bytes of the payload are cut (at least one byte stays);
    signature: 13 bytes, sent with incompat bit 0 set."""
    payload = bytes(payload)
    if truncate:
        while len(payload) > 1 and payload[-1] == 0:
            payload = payload[:-1]
    if signature is not None:
        incompat |= 1
    body = bytes([len(payload), incompat, compat, seq, sysid, compid, msgid & 0xFF, (msgid >> 8) & 0xFF, msgid >> 16]) + payload
    crc = x25(body + bytes([extra])) ^ (0x0001 if bad else 0)
    out = b"\xfd" + body + bytes([crc & 0xFF, crc >> 8])
    return out + (bytes(signature) if signature is not None else b"")


def junk(rng, n, starts=False):
    """n bytes that are no frame; starts=False: none of them a start byte."""
    b = rng.integers(0, 256, n, dtype=np.uint8)
    if not starts:
        b[b >= 0xFD] = 0x55
    return b.tobytes()


# ---- the model -----------------------------------------------------------------------------------------------------
class Parser:
    """One stream's receive state: the six counters and `bytes`, the frame in progress, and `events`, the names of
    the transitions taken so far (what the coverage test counts)."""

    def __init__(self):
        self.c = dict.fromkeys(COUNTERS, 0)
        self.events = set()
        self.phase = "idle"

    def _start(self, v2):
        self.phase, self.v2, self.head, self.payload, self.check, self.signature = "header", v2, [], [], [], 0
        self.events.add("start v2" if v2 else "start v1")

    def feed(self, data, M, out):
        """Takes `data` in order; appends the samples (t, x, y, z: the floats as uint32 bits) the round keeps to `out`,
        which holds the round's samples so far."""
        n = len(data)
        for i, b in enumerate(bytes(data)):
            self.c["bytes"] += 1
            last = False
            if self.phase == "idle":
                if b in (0xFD, 0xFE):
                    self._start(b == 0xFD)
                else:
                    self.c["skipped"] += 1
                continue
            if self.phase == "header":
                self.head.append(b)
                if self.v2 and len(self.head) == 2 and b & ~1:
                    self.c["rejected_flags"] += 1
                    self.events.add("rejected incompat")
                    self.phase = "idle"
                    continue
                if len(self.head) == (9 if self.v2 else 5):
                    self.len = self.head[0]
                    self.msgid = self.head[6] | self.head[7] << 8 | self.head[8] << 16 if self.v2 else self.head[4]
                    self.signed = bool(self.v2 and self.head[1] & 1)
                    self.phase = "payload" if self.len else "check"
                    if self.len == 0:
                        self.events.add("len 0")
                    if self.len == 255:
                        self.events.add("len 255")
                continue
            if self.phase == "payload":
                self.payload.append(b)
                if len(self.payload) == self.len:
                    self.phase = "check"
                continue
            if self.phase == "check":
                self.check.append(b)
                if len(self.check) == 2:
                    if self.signed:
                        self.phase = "signature"
                    else:
                        last = True
                if not last:
                    continue
            elif self.phase == "signature":
                self.signature += 1
                if self.signature < 13:
                    continue
                self.events.add("signature")
            # the frame's last byte
            self.phase = "idle"
            self.c["frames"] += 1
            if i == n - 1:
                self.events.add("frame ends at len")
            if self.msgid != HIGHRES_IMU:
                self.events.add("other message")
                continue
            crc = x25(bytes(self.head) + bytes(self.payload) + bytes([HIGHRES_IMU_EXTRA]))
            if [crc & 0xFF, crc >> 8] != self.check:
                self.c["bad_check"] += 1
                self.events.add("bad check")
                continue
            self.c["imu_samples"] += 1
            self.events.add("sample v2" if self.v2 else "sample v1")
            if self.len < 32:
                self.events.add("len < 32 sample")
            if self.len == 63:
                self.events.add("extended sample")
            p = (bytes(self.payload) + bytes(32))[:32]
            sample = (struct.unpack_from("<Q", p, 0)[0],) + struct.unpack_from("<3I", p, 20)
            if len(out) < M:
                out.append(sample)
            else:
                self.c["overflowed"] += 1
                self.events.add("overflow")
        if self.phase != "idle" and n:
            self.events.add("cut in " + self.phase)

    def public(self):
        return np.array([tuple(self.c[n] for n in COUNTERS)], PUBLIC_DTYPE)[0]


def run(data, lengths, M, parsers):
    """The call on data uint8 [K, S, B], lengths [K, S] or None, with one Parser per stream (stepped in place).
    Returns (samples SAMPLE_DTYPE [K, M, S] -- slots nobody wrote hold SENTINEL bytes --, counts uint8 [K, S])."""
    K, S, B = data.shape
    samples = np.full((K, M, S, 24), SENTINEL, np.uint8).view(SAMPLE_DTYPE).reshape(K, M, S)
    counts = np.zeros((K, S), np.uint8)
    for s in range(S):
        for k in range(K):
            n = B if lengths is None else min(int(lengths[k, s]), B)
            out = []
            parsers[s].feed(data[k, s, :n].tobytes(), M, out)
            counts[k, s] = len(out)
            for j, (t, x, y, z) in enumerate(out):
                samples[k, j, s] = np.array([(t, 0, 0, 0, 0)], SAMPLE_DTYPE)[0]
                samples[k, j, s:s + 1].view(np.uint32).reshape(6)[2:5] = (x, y, z)
    return samples, counts


def publics(parsers):
    return np.array([p.public() for p in parsers], PUBLIC_DTYPE)


def decode(stream_bytes):
    """The samples of one byte stream taken whole, as (time_usec, xgyro, ygyro, zgyro) with float values."""
    out = []
    Parser().feed(stream_bytes, 1 << 30, out)
    return [(t,) + struct.unpack("<3f", struct.pack("<3I", x, y, z)) for t, x, y, z in out]


# ---- the coverage family ---------------------------------------------------------------------------------------------
def _imu(rng, i, **kw):
    t = 1_000_000 + 4000 * i
    x, y, z = (float(v) for v in rng.uniform(-3, 3, 3).astype(np.float32))
    return imu_payload(t, x, y, z, **kw)


def stream_items(rng, kind, n_items):
    """A list of byte strings (whole frames, junk runs) for one stream; `kind` picks the mix."""
    sig = bytes(range(1, 14))
    items = []
    for i in range(n_items):
        c = int(rng.integers(0, 100))
        if kind == 1 and c < 30:   # four 8-byte frames in a row: two samples in any 16 bytes of them
            items.append(frame_v1(HIGHRES_IMU, b"", seq=i & 255) * 4)
        elif kind == 1:    # dense short HIGHRES_IMU frames: a long round overflows M
            items.append(frame_v2(HIGHRES_IMU, _imu(rng, i)[:int(rng.choice([9, 24, 32]))], seq=i & 255))
        elif kind == 2:    # junk with start bytes in it: false starts, frames sized by junk
            items.append(junk(rng, int(rng.integers(1, 60)), starts=True) if c < 70 else frame_v1(HIGHRES_IMU, _imu(rng, i), seq=i & 255))
        elif kind == 3:    # mostly other messages of every length: the bulk skip
            if c < 75:
                ln = int(rng.choice([0, 1, 15, 16, 17, 100, 127, 128, 129, 254, 255]))
                body = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
                mid = int(rng.choice([0, 1, 30, 104, 106, 105 + 256, 105 + 65536]))
                items.append(frame_v2(mid, body, truncate=False, signature=sig if c < 20 else None) if c % 2 else frame_v1(mid & 255 if mid & 255 != 105 else 33, body))
            else:
                items.append(frame_v2(HIGHRES_IMU, _imu(rng, i, rest=1.5), seq=i & 255))
        else:              # everything
            if c < 12:
                items.append(frame_v1(HIGHRES_IMU, _imu(rng, i, rest=2.5), seq=i & 255))
            elif c < 22:
                items.append(frame_v2(HIGHRES_IMU, _imu(rng, i, rest=2.5, ext=7), seq=i & 255, truncate=False))
            elif c < 32:
                items.append(frame_v2(HIGHRES_IMU, _imu(rng, i), seq=i & 255, signature=sig))
            elif c < 40:
                items.append(frame_v2(HIGHRES_IMU, _imu(rng, i)[:int(rng.integers(1, 32))], truncate=False))
            elif c < 46:   # a frame of another message whose payload holds a whole valid HIGHRES_IMU frame
                items.append(frame_v2(33, frame_v1(HIGHRES_IMU, _imu(rng, i)) + b"\x01", truncate=False))
            elif c < 52:
                items.append(frame_v1(HIGHRES_IMU, _imu(rng, i), bad=True) if c % 2 else frame_v2(HIGHRES_IMU, _imu(rng, i), bad=True))
            elif c < 58:   # an incompat flag this parser cannot size; the rest of that frame is scanned in idle
                items.append(frame_v2(HIGHRES_IMU, _imu(rng, i), incompat=int(rng.choice([2, 3, 0x80]))))
            elif c < 64:
                items.append(frame_v1(0, b"") if c % 2 else frame_v2(0, b"", truncate=False))
            elif c < 70:   # the longest frames: another message, and HIGHRES_IMU padded to 255 bytes
                pad = _imu(rng, i) + bytes(rng.integers(0, 256, 255 - 62, dtype=np.uint8))
                items.append(frame_v2(HIGHRES_IMU if c % 2 else 77, pad, truncate=False, signature=sig if c < 67 else None))
            elif c < 76:
                items.append(frame_v1(HIGHRES_IMU, b""))          # len 0 with a matching checksum: a sample of zeros
            elif c < 88:
                items.append(junk(rng, int(rng.integers(1, 40))))
            else:
                items.append(frame_v2(HIGHRES_IMU, _imu(rng, i), seq=i & 255))
    return items


def edge_lengths(B):
    return [0, 1, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE - 1, 2 * PIECE, 2 * PIECE + 1, B - 1, B, B + 7, 0xFFFF]


def coverage_family(seed, S, K, B, calls=1):
    """`calls` successive calls of K rounds for S streams: a list of (data uint8 [K, S, B], lengths uint16 [K, S]).
    Every stream has a byte stream of its own kind; round after round takes the next bytes of it, with lengths that
    walk the staging edges (0, 1, around the multiples of the piece, B - 1, B, above B) or end exactly at a frame's
    last byte.  Behind a round's length the slot holds valid HIGHRES_IMU frames that must not be parsed.  Long rounds
    are few, so that the model stays quick."""
    rng = np.random.default_rng(seed)
    edges = edge_lengths(B)
    small = [e for e in edges if e <= 2 * PIECE + 1]
    big = [e for e in edges if e > 2 * PIECE + 1]
    decoy = frame_v1(HIGHRES_IMU, imu_payload(77, 1.0, 2.0, 3.0)) + frame_v2(HIGHRES_IMU, imu_payload(78, 1.0, 2.0, 3.0))
    decoy = np.frombuffer((decoy * (B // len(decoy) + 2))[:B], np.uint8)
    streams, ends, pos = [], [], [0] * S
    for s in range(S):
        items = stream_items(rng, s % 4, 20 + int(calls * K * min(B, 300) / 40))
        streams.append(np.frombuffer(b"".join(items), np.uint8))
        ends.append(np.cumsum([len(i) for i in items]))
    out = []
    for c in range(calls):
        data = np.empty((K, S, B), np.uint8)
        lengths = np.zeros((K, S), np.uint16)
        for k in range(K):
            for s in range(S):
                r = (c * K + k) * 7 + s * 3
                if r % 13 == 0:      # end exactly at the last byte of the frame under way (where the slot holds it)
                    nxt = ends[s][np.searchsorted(ends[s], pos[s], side="right")] if pos[s] < ends[s][-1] else pos[s]
                    n = int(nxt - pos[s]) if nxt - pos[s] <= B else B
                elif r % 29 == 0 or (s % 4 == 1 and k == K - 1):
                    n = big[r % len(big)]
                else:
                    n = small[r % len(small)]
                take = min(n, B, len(streams[s]) - pos[s])
                if take < min(n, B):     # the stream ran dry: the length says so
                    n = take
                lengths[k, s] = n
                data[k, s] = decoy
                data[k, s, :take] = streams[s][pos[s]:pos[s] + take]
                pos[s] += take
        out.append((data, lengths))
    return out
