"""The stream bank's MAVLink receive on the host (aof_bank_mavlink_rx_host) against the plain-Python model of the
header's text (tests/mavlink_rx_ref.py): the hand vector, split invariance, the coverage family in which every
transition and every counter fires, and 100 000 random bytes seeded with frame fragments.  CPU only.

The hand vector's bytes are literals.  The issue that asked for them words the MAVLink 1 frame as "... + 16 zero bytes +
the gyro floats + 30 zero bytes + c636" and, in the same sentence, as 70 bytes with a 62-byte payload and the floats at
payload offsets 20-31: only 12 zero bytes agree with the three figures and with the check bytes c6 36 (the MAVLink 2
frame of the same message is worded with 12), so 12 it is."""
import numpy as np
import pytest

import mavlink_rx_ref as ref

V1 = bytes.fromhex("fe3e0701016940420f0000000000" + "00" * 12 + "0000003f000080be00000040" + "00" * 30 + "c636")
V2 = bytes.fromhex("fd20000008010169000040420f0000000000" + "00" * 12 + "0000003f000080be0000004020cd")
SAMPLE = (1000000, 0.5, -0.25, 2.0)


def slot(stream_bytes, B=None):
    """(data [1, 1, B], lengths [1, 1]) holding one stream's bytes."""
    B = B or max(16, (len(stream_bytes) + 15) // 16 * 16)
    data = np.zeros((1, 1, B), np.uint8)
    data[0, 0, :len(stream_bytes)] = np.frombuffer(stream_bytes, np.uint8)
    return data, np.array([[len(stream_bytes)]], np.uint16)


def host(aof, calls, M, S, states=None):
    """aof_bank_mavlink_rx_host over successive calls [(data, lengths)] -> ([samples], [counts], states); sample slots
    nobody wrote hold the model's sentinel."""
    states = np.zeros(S, aof.MAVLINK_RX_STATE_DTYPE) if states is None else states
    all_samples, all_counts = [], []
    for data, lengths in calls:
        K = data.shape[0]
        samples = np.full((K, M, S, 24), ref.SENTINEL, np.uint8).view(aof.IMU_SAMPLE_DTYPE).reshape(K, M, S)
        counts = np.full((K, S), ref.SENTINEL, np.uint8)
        aof.bank_mavlink_rx_host(data, lengths, states, M, samples, counts)
        all_samples.append(samples)
        all_counts.append(counts)
    return all_samples, all_counts, states


def model(calls, M, S):
    parsers = [ref.Parser() for _ in range(S)]
    out = [ref.run(data, lengths, M, parsers) for data, lengths in calls]
    return [o[0] for o in out], [o[1] for o in out], parsers


def host_samples(aof, stream_bytes, M=16):
    """The samples of one stream's bytes taken in one call, as tuples, and the final state."""
    samples, counts, states = host(aof, [slot(stream_bytes)], M, 1)
    n = int(counts[0][0, 0])
    return [tuple(samples[0][0, j, 0][f].item() for f in ("time_usec", "xgyro", "ygyro", "zgyro")) for j in range(n)], states


def assert_same(aof, calls, M, S):
    hs, hc, states = host(aof, calls, M, S)
    ms, mc, parsers = model(calls, M, S)
    for c in range(len(calls)):
        assert np.array_equal(hc[c], mc[c]), c
        assert hs[c].tobytes() == ms[c].tobytes(), c       # samples up to the counts, the sentinel behind them
    pub = ref.publics(parsers)
    for n in ref.COUNTERS:
        assert np.array_equal(states[n], pub[n]), n
    idle = np.array([p.phase == "idle" for p in parsers])
    assert not states["in_progress"][idle].any(), "an idle stream's private bytes are all zero"
    assert states["in_progress"][~idle].any(axis=1).all()
    return states, parsers


def test_the_checksum_routine_is_the_one_the_vector_was_made_with():
    assert ref.x25(b"123456789") == 0x6F91
    assert len(V1) == 70 and len(V2) == 44
    assert ref.frame_v1(105, ref.imu_payload(*SAMPLE), seq=7) == V1
    assert ref.frame_v2(105, ref.imu_payload(*SAMPLE), seq=8) == V2


@pytest.mark.parametrize("frame", [V1, V2], ids=["v1", "v2 truncated"])
def test_the_hand_vector_yields_its_sample(aof, frame):
    got, states = host_samples(aof, frame)
    assert got == [SAMPLE] and ref.decode(frame) == [SAMPLE]
    assert (states["bytes"][0], states["frames"][0], states["imu_samples"][0]) == (len(frame), 1, 1)
    assert states["bad_check"][0] == states["skipped"][0] == states["overflowed"][0] == states["rejected_flags"][0] == 0
    assert not states["in_progress"].any()


@pytest.mark.parametrize("frame", [V1, V2], ids=["v1", "v2 truncated"])
def test_any_flipped_bit_behind_the_start_byte_yields_no_sample(aof, frame):
    for bit in range(8, 8 * len(frame)):
        flipped = bytearray(frame)
        flipped[bit // 8] ^= 1 << (bit % 8)
        got, _ = host_samples(aof, bytes(flipped))
        assert got == [] and ref.decode(bytes(flipped)) == [], bit


def split_stream():
    rng = np.random.default_rng(5)
    inner = ref.frame_v1(105, ref.imu_payload(9, 9.0, 9.0, 9.0))
    parts = [ref.frame_v1(105, ref.imu_payload(1000, 0.1, 0.2, 0.3, rest=4.0), seq=1), ref.junk(rng, 11),
             ref.frame_v2(105, ref.imu_payload(2000, -0.1, -0.2, -0.3, rest=4.0), seq=2, signature=bytes(range(13))),
             ref.frame_v2(33, inner + b"\x07", seq=3, truncate=False),
             ref.frame_v2(105, ref.imu_payload(3000, 1.0, 2.0, 3.0), seq=4)]
    return b"".join(parts)


def test_every_cut_into_two_calls_leaves_the_same_samples_and_state(aof):
    stream = split_stream()
    whole, state1 = host_samples(aof, stream)
    assert [s[0] for s in whole] == [1000, 2000, 3000] and whole == ref.decode(stream)
    assert state1["frames"][0] == 4 and state1["skipped"][0] == 11 and not state1["in_progress"].any()
    B = (len(stream) + 15) // 16 * 16
    for cut in range(len(stream) + 1):
        calls = [slot(stream[:cut], B), slot(stream[cut:], B)]
        samples, counts, states = host(aof, calls, 16, 1)
        got = [samples[c][0, j, 0] for c in range(2) for j in range(int(counts[c][0, 0]))]
        assert [tuple(g[f].item() for f in ("time_usec", "xgyro", "ygyro", "zgyro")) for g in got] == whole, cut
        assert states.tobytes() == state1.tobytes(), cut
        assert_same(aof, calls, 16, 1)


EVENTS = {"start v1", "start v2", "rejected incompat", "len 0", "len 255", "len < 32 sample", "extended sample", "signature",
          "other message", "bad check", "sample v1", "sample v2", "overflow", "frame ends at len", "cut in header",
          "cut in payload", "cut in check", "cut in signature"}


@pytest.mark.parametrize("K,B,M,calls", [(1, 16, 1, 24), (5, 272, 4, 2), (16, 4096, 16, 1)])
def test_the_coverage_family_fires_everything_and_host_equals_model(aof, K, B, M, calls):
    S = 65
    fam = ref.coverage_family(3, S, K, B, calls)
    edges = {min(e, B) for e in ref.edge_lengths(B)}
    seen = {min(int(v), B) for _, lengths in fam for v in lengths.ravel()}
    assert edges <= seen and any(int(v) > B for _, lengths in fam for v in lengths.ravel()), sorted(edges - seen)
    states, parsers = assert_same(aof, fam, M, S)
    fired = set().union(*(p.events for p in parsers))
    assert fired >= EVENTS, sorted(EVENTS - fired)
    for n in ref.COUNTERS:
        assert states[n].sum() > 0, n


def test_null_lengths_mean_every_byte_of_the_slot(aof):
    fam = ref.coverage_family(4, 9, 3, 272)
    calls = [(data, None) for data, _ in fam]
    assert_same(aof, calls, 4, 9)
    full = [(data, np.full(data.shape[:2], 272, np.uint16)) for data, _ in fam]
    assert host(aof, calls, 4, 9)[2].tobytes() == host(aof, full, 4, 9)[2].tobytes()


def test_valid_frames_behind_the_length_are_not_parsed(aof):
    data, lengths = slot(V2 + V1 + V2, 160)
    lengths[0, 0] = len(V2) + 30                     # the second frame is cut, the third lies behind the length
    samples, counts, states = host(aof, [(data, lengths)], 4, 1)
    assert counts[0][0, 0] == 1 and states["bytes"][0] == len(V2) + 30 and states["in_progress"].any()
    assert_same(aof, [(data, lengths)], 4, 1)


def test_a_hundred_thousand_random_bytes_seeded_with_fragments(aof):
    rng = np.random.default_rng(11)
    S, K, B, M = 7, 4, 4096, 16
    frags = [V1, V2, V1[:9], V2[:13], V2[:-1], b"\xfd", b"\xfe", b"\xfd\x00\x00", b"\xfe\x00", ref.frame_v2(0, b"", truncate=False),
             ref.frame_v2(105, ref.imu_payload(5, 1.0, 1.0, 1.0), signature=bytes(13))]
    data = rng.integers(0, 256, (K, S, B), dtype=np.uint8)
    for k in range(K):
        for s in range(S):
            at = 0
            while True:
                f = frags[int(rng.integers(0, len(frags)))]
                at += int(rng.integers(0, 90))
                if at + len(f) > B:
                    break
                data[k, s, at:at + len(f)] = np.frombuffer(f, np.uint8)
                at += len(f)
    assert data.size >= 100_000
    states, parsers = assert_same(aof, [(data, None)], M, S)
    assert states["imu_samples"].sum() > 100 and states["rejected_flags"].sum() > 0 and states["frames"].sum() > states["imu_samples"].sum()
