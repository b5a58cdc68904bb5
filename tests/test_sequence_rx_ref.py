"""aof_sequence_mavlink_rx_host (include/aof_sequence_mavlink_rx.h) against the sequential model of tests/sequence_rx_ref.py,
byte for byte, on the family of designed logs; the closed form the kernels compute against the same model; the host function
against aof_bank_mavlink_rx_host fed the log in rounds; the census of the family; the refusals; and the scratch size against
the plan's model; and the same on the DEEP family (sequence_rx_ref.deep_cases: full lists, a second trip of a workgroup's lanes, two
and three scan levels, byte_end at every delivery), whose largest logs take their expectation from the tile rule, held to the
sequential model here.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import sequence_rx_ref as ref
import sequence_rx_rig as rig

CASES = ref.cases()
IDS = [c["name"] for c in CASES]
DEEP, BIG = ref.deep_names(), list(ref.BIG)
BURST_MAX, SLOTS_MAX, ROUND_BYTES = 16, 16, 4096


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_closed_form_reaches_what_the_sequential_model_parses(case):
    log, p = bytes(case["log"]), case["want"]["parser"]
    starts, cut = ref.reached(log)
    frames = [s for s in starts if log[s] in (0xFD, 0xFE)]
    assert p.c["bytes"] == len(log)
    assert len(starts) - len(frames) == p.c["skipped"]
    assert len(frames) == p.c["frames"] + p.c["rejected_flags"] + (cut is not None)
    assert (cut is not None) == (p.phase != "idle")
    entry = ref.entry_chain(log)
    assert entry == ref.entry_chain_serial(log)
    assert all(e == ref.END or e < ref.FRAME_MAX for e in entry)
    assert len(entry) == ref.plan(len(log))["chunks"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_host_function_equals_the_model_byte_for_byte(aof, case):
    want, M = case["want"], case["max_samples"]
    samples, sample_end, state = rig.run_host(aof, case["log"], case["byte_end"], M, ref.SENTINEL)
    written = len(want["samples"])
    assert written == min(want["total"], M)
    assert samples[:written].tobytes() == want["samples"].tobytes()
    assert (samples[written:] == ref.SENTINEL).all(), "slots behind the written samples are not written"
    assert sample_end.tobytes() == want["sample_end"].tobytes()
    assert state.tobytes() == want["state"]
    overflowed = np.frombuffer(state.tobytes(), ref.STATE_DTYPE)["overflowed"][0]
    assert overflowed == max(0, want["total"] - M)


def rounds_of(N, byte_end, delivered):
    """The log cut at byte_end into rounds of at most ROUND_BYTES bytes and SLOTS_MAX samples: [(lo, hi)], and for every k the
    number of rounds in front of byte_end[k]."""
    cuts = sorted(set(min(int(v), N) for v in byte_end) | {N})
    rounds, lo = [], 0
    d = np.asarray(delivered, np.int64)
    for cut in cuts:
        while lo < cut:
            hi = min(cut, lo + ROUND_BYTES)
            first = int(np.searchsorted(d, lo, side="right"))       # samples delivered in (lo, hi]
            if first + SLOTS_MAX < len(d):
                hi = min(hi, int(d[first + SLOTS_MAX]) - 1)
            rounds.append((lo, hi))
            lo = hi
    return rounds


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_host_function_equals_a_one_stream_bank_fed_the_log_in_rounds(aof, case):
    log, N = case["log"], len(case["log"])
    free = ref.model(bytes(log), [], 1 << 30)
    total = free["total"]
    byte_end = np.sort(np.minimum(case["byte_end"].astype(np.int64), N)).astype(np.uint32)
    samples, sample_end, state = rig.run_host(aof, log, byte_end, total + 1, ref.SENTINEL)
    rounds = rounds_of(N, byte_end, free["delivered"])
    states = np.zeros(1, aof.MAVLINK_RX_STATE_DTYPE)
    got, per_round = [], []
    for r0 in range(0, len(rounds), BURST_MAX):
        burst = rounds[r0:r0 + BURST_MAX]
        data = np.zeros((len(burst), 1, ROUND_BYTES), np.uint8)
        lengths = np.zeros((len(burst), 1), np.uint16)
        for k, (lo, hi) in enumerate(burst):
            data[k, 0, :hi - lo] = log[lo:hi]
            lengths[k, 0] = hi - lo
        s, counts = aof.bank_mavlink_rx_host(data, lengths, states, SLOTS_MAX)
        for k in range(len(burst)):
            got.append(s[k, :counts[k, 0], 0])
            per_round.append(int(counts[k, 0]))
    got = np.concatenate(got) if got else np.zeros(0, aof.IMU_SAMPLE_DTYPE)
    assert len(got) == total and got.tobytes() == samples[:total].tobytes()
    assert states.tobytes() == state.tobytes(), "the same 128 state bytes (no round overflowed)"
    # per-round counts add up to the differences of sample_end
    ends = np.array([hi for _, hi in rounds], np.int64)
    cum = np.concatenate([[0], np.cumsum(per_round)])
    for k, q in enumerate(byte_end):
        assert cum[int(np.searchsorted(ends, int(q), side="right"))] == sample_end[k], (k, q)


def test_every_edge_is_reached_and_every_case_meets_its_condition():
    reached = set()
    for case in CASES:
        got = ref.census(case)
        assert case["claimed"] <= got, (case["name"], sorted(case["claimed"] - got))
        reached |= got
    missing = [e for e in ref.EDGES if e not in reached]
    assert not missing, missing


def test_refused_calls_write_nothing(aof):
    case = next(c for c in CASES if c["name"] == "2 chunks")
    log, byte_end, N, n = case["log"], case["byte_end"], len(case["log"]), len(case["byte_end"])
    samples = np.full((8, 24), ref.SENTINEL, np.uint8)
    sample_end = np.full(n, 0xEEEEEEEE, np.uint32)
    state = np.full(128, ref.SENTINEL, np.uint8)
    P = rig.params
    refused = [dict(rp=None), dict(log=None), dict(samples=None), dict(byte_end=None), dict(sample_end=None), dict(rp=P(-1, 8)),
               dict(rp=P(1 << 31, 8)), dict(rp=P(N, 0)), dict(rp=P(N, 1 << 31)), dict(n=-1), dict(n=0x7FFFFFF0)]
    for kw in refused:
        a = dict(rp=P(N, 8), n=n, log=log, byte_end=byte_end, samples=samples, sample_end=sample_end)
        a.update(kw)
        assert rig.host(aof, a["rp"], a["n"], a["log"], a["byte_end"], a["samples"], a["sample_end"], state) == rig.EINVAL, kw
    assert (samples == ref.SENTINEL).all() and (sample_end == 0xEEEEEEEE).all() and (state == ref.SENTINEL).all()
    # no frames: the two arrays may be absent, samples and state are produced
    assert rig.host(aof, P(N, 8), 0, log, None, samples, None, state) == 0
    assert state.tobytes() == ref.model(bytes(log), [], 8)["state"]
    # no bytes: a reset state, sample_end 0
    assert rig.host(aof, P(0, 8), n, None, byte_end, samples, sample_end, state) == 0
    assert not state.any() and not sample_end.any()
    # the device call without a context is refused first
    call = rig.bind(aof).aof_sequence_mavlink_rx_device
    assert call(None, C.byref(P(N, 8)), n, None, None, None, None, None, None, 0, None) == rig.EINVAL


def test_the_scratch_size_is_the_plans(aof):
    sizes = [0, 1, ref.C - 1, ref.C, ref.C + 1, 2 * ref.C, 256 * ref.C, 256 * ref.C + 1, 65536 * ref.C, 65536 * ref.C + 1, 20_000_000,
             (1 << 31) - 1]
    for n in sizes:
        assert rig.scratch_bytes(aof, n) == ref.plan(n)["total_bytes"], n
    assert rig.scratch_bytes(aof, -1) == 0 and rig.scratch_bytes(aof, 1 << 31) == 0
    big = ref.plan((1 << 31) - 1)
    assert big["chunks"] == 1 << 19 and big["rounds"] == 19 and big["scan_entries"] == [1 << 19, 2048, 8]
    assert ref.plan(20_000_000)["total_bytes"] < 0.30 * 20_000_000, "two tables of 288 u16 per chunk: about 28 % of N"


# ---- the deep family ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DEEP)
def test_the_closed_form_reaches_what_the_expectation_holds_on_the_deep_family(name):
    case = ref.deep_case(name)
    log, want = bytes(case["log"]), case["want"]
    counters = np.frombuffer(want["state"], ref.STATE_DTYPE)[0]
    starts, cut = ref.reached(log)
    frames = [s for s in starts if log[s] in (0xFD, 0xFE)]
    assert counters["bytes"] == len(log)
    assert len(starts) - len(frames) == counters["skipped"]
    assert len(frames) == counters["frames"] + counters["rejected_flags"] + (cut is not None)
    assert (cut is not None) == (want["parser"].phase != "idle")
    assert set(want["sample_start"].tolist()) <= set(frames), "every sample's frame starts at a reached position"
    entry = ref.entry_chain(log)
    assert entry == ref.entry_chain_serial(log)
    assert all(e == ref.END or e < ref.FRAME_MAX for e in entry)
    assert len(entry) == ref.plan(len(log))["chunks"]


def host_equals(aof, case):
    want, M = case["want"], case["max_samples"]
    samples, sample_end, state = rig.run_host(aof, case["log"], case["byte_end"], M, ref.SENTINEL)
    written = len(want["samples"])
    assert written == min(want["total"], M)
    assert samples[:written].tobytes() == want["samples"].tobytes()
    assert (samples[written:] == ref.SENTINEL).all(), "slots behind the written samples are not written"
    assert sample_end.tobytes() == want["sample_end"].tobytes()
    assert state.tobytes() == want["state"]
    overflowed = np.frombuffer(state.tobytes(), ref.STATE_DTYPE)["overflowed"][0]
    assert overflowed == max(0, want["total"] - M)


@pytest.mark.parametrize("name", DEEP)
def test_the_host_function_equals_the_expectation_on_the_deep_family(aof, name):
    host_equals(aof, ref.deep_case(name))


@pytest.mark.parametrize("name", BIG)
def test_the_host_function_equals_the_tile_rule_on_the_largest_logs(aof, name):
    case = ref.deep_case(name)
    assert case["tile"] is not None and len(case["tile"]) % 2 == 1 and 6 * ref.C <= len(case["tile"]) <= 8 * ref.C
    assert case["want"]["total"] > 120_000 and 580 <= len(case["byte_end"]) <= 640
    host_equals(aof, case)


def test_the_tile_rule_equals_the_sequential_model():
    """Three tiles and a cut, about 100 KB, at a capacity below the total, for both kinds of tile; with it capped() is held too."""
    rng = np.random.default_rng(3)
    for tile in (ref.big_log()[0], ref.deep_case("513 chunks")["tile"]):
        T = len(tile)
        assert T % 2 == 1
        for N in (3 * T + 5000, 3 * T, 2 * T + 1, T - 1):
            byte_end = np.concatenate([rng.integers(0, N + 9, 200), [0, N, T, 2 * T, 3 * T]]).astype(np.uint32)
            want = ref.model(ref.tiled_log(tile, N).tobytes(), byte_end, 1 << 30)
            for M in (want["total"] + 1, want["total"] - 3):
                want = ref.model(ref.tiled_log(tile, N).tobytes(), byte_end, M) if M < want["total"] else want
                got = ref.tiled_expectation(tile, N, byte_end, M)
                for key in ("samples", "delivered", "sample_start", "sample_end"):
                    assert got[key].tobytes() == want[key].tobytes() and got[key].dtype == want[key].dtype, (N, M, key)
                assert got["total"] == want["total"] and got["state"] == want["state"], (N, M)


def test_every_deep_edge_is_reached():
    reached = set()
    for name in DEEP + BIG:
        case = ref.deep_case(name)
        got = ref.deep_census(case)
        assert case["claimed"] <= got, (name, sorted(case["claimed"] - got))
        reached |= got
    missing = [e for e in ref.DEEP_EDGES if e not in reached]
    assert not missing, missing
    assert [c["name"] for c in ref.deep_cases()] == DEEP and len(ref.cases()) == 58


def test_the_scratch_size_is_the_plans_at_the_deep_chunk_counts(aof):
    shapes = {"256 chunks": (8, [256]), "257 chunks": (9, [257, 2]), "512 chunks": (9, [512, 2]), "513 chunks": (10, [513, 3]),
              "65536 chunks": (16, [65536, 256]), "65537 chunks less 1234 bytes": (17, [65537, 257, 2]),
              "65538 chunks less 1234 bytes": (17, [65538, 257, 2])}
    for name, (rounds, scan) in shapes.items():
        n = ref.BIG[name][0] if name in ref.BIG else len(ref.deep_case(name)["log"])
        P = ref.plan(n)
        assert rig.scratch_bytes(aof, n) == P["total_bytes"], name
        assert (P["rounds"], P["scan_entries"]) == (rounds, scan), name
    assert ref.plan(ref.BIG["65537 chunks less 1234 bytes"][0])["total_bytes"] < 0.29 * 65537 * ref.C
