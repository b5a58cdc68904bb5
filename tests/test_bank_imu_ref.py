"""The stream bank's IMU on the host: the model (imu_ref.py) reaches every outcome on its coverage family, the
sample-by-sample order of the additions is visible in the sums, and aof_bank_imu_host equals the model byte for byte --
records, frames up to their lengths, lengths, the whole 64-byte states -- on the family, on 100 000 random samples and
on the edges one by one.  CPU only."""
import numpy as np
import pytest

import imu_ref as ref


@pytest.fixture(scope="module")
def fam():
    f = ref.family()
    f["want"] = ref.run(f["samples"], f["counts"], f["times"], f["records"], f["states"], first_seq=f["first_seq"])
    return f


def host(aof, f, **kw):
    """aof_bank_imu_host on the inputs of a family -> dict like ref.run's (frames filled with the model's sentinel)."""
    states = f["states"].copy()
    records, frames, lengths = aof.bank_imu_host(f["samples"], f["counts"], f["times"], f["records"].copy(), states,
                                                 first_seq=f["first_seq"], fill=ref.SENTINEL, **kw)
    return dict(records=records, frames=frames, lengths=lengths, states=states)


def assert_same(got, want, what=""):
    for name in ("records", "lengths", "frames", "states"):
        if got.get(name) is None:
            continue
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name, np.flatnonzero(g.view(np.uint8).ravel() != w.view(np.uint8).ravel())[:8])


def test_the_models_dtypes_are_the_bindings(aof):
    assert aof.IMU_SAMPLE_DTYPE == ref.SAMPLE_DTYPE and aof.IMU_STATE_DTYPE == ref.STATE_DTYPE and aof.TICK_DTYPE == ref.RECORD_DTYPE
    assert (aof.TICK_HELD, aof.TICK_IDLE, aof.TICK_STALE_GYRO, aof.TICK_NO_OFFSET) == (ref.HELD, ref.IDLE, ref.STALE_GYRO, ref.NO_OFFSET)
    assert (aof.IMU_SLOTS_MAX, aof.BANK_BURST_MAX, aof.SEQ_FRAME_BYTES) == (ref.SLOTS_MAX, ref.BURST_MAX, ref.FRAME_BYTES)


def test_the_family_reaches_every_outcome(fam):
    assert fam["samples"].shape == (ref.FAMILY_K, ref.FAMILY_M, ref.FAMILY_S) and ref.FAMILY_S == 48
    tally = fam["want"]["tally"]
    missing = [o for o in ref.OUTCOMES if tally[o] < 1]
    assert not missing, (missing, dict(tally))
    assert set(tally) <= set(ref.OUTCOMES), set(tally) - set(ref.OUTCOMES)
    want = fam["want"]
    q = want["records"]["quality"]
    assert {ref.HELD, ref.IDLE, ref.STALE_GYRO, ref.NO_OFFSET} <= set(q.ravel().tolist()) and (q >= 0).any()
    # a frame exactly where a record is sent, and never behind a dropped one
    assert ((want["lengths"] > 0) == (q >= 0)).all()
    assert (want["states"]["dropped"] == ((q == ref.STALE_GYRO) | (q == ref.NO_OFFSET)).sum(axis=0)).all()
    # slots behind a round's count are never taken: every sample taken is counted once
    taken = np.minimum(fam["counts"], ref.FAMILY_M).sum(axis=0)
    st0, st1 = fam["states"], want["states"]
    assert ((st1["samples_integrated"] - st0["samples_integrated"]) + (st1["samples_rejected"] - st0["samples_rejected"]) == taken).all()


def test_the_order_of_the_additions_shows_in_the_sums(fam):
    """((acc + s1) + s2) + s3 against acc + ((s1 + s2) + s3): for at least one stream of the family the final doubles
    differ in their bits -- the condition that makes the sample-by-sample rule testable at all."""
    st = fam["want"]["states"]
    real = np.stack([st["gyro_x"], st["gyro_y"], st["gyro_z"]], axis=1)
    alt = fam["want"]["alt"]
    differ = (real.view(np.uint64) != np.ascontiguousarray(alt).view(np.uint64)).any(axis=1)
    assert differ.any()
    assert np.allclose(real, alt, rtol=0, atol=1e-12), "the two orders are the same sums up to rounding"


def test_the_serializer_agrees_with_the_facades(aof):
    import os
    if not os.path.exists(aof.FACADE_PATH):
        import __graft_entry__ as ge
        ge.build()
    rng = np.random.default_rng(11)
    for k in range(50):
        g = tuple(float(v) for v in rng.normal(0, 0.01, 3))
        fx, fy = (np.float32(v) for v in rng.normal(0, 0.02, 2))
        q = int(rng.integers(1, 256)) if k % 4 else 0
        t, off, dt = int(rng.integers(0, 2 ** 32)), int(rng.integers(1, 2 ** 40)), int(rng.integers(0, 200000))
        assert ref.frame(off + t, dt, fx, fy, g, q, k, 1, 100) == aof.pack_optical_flow_rad(off, t, dt, float(fx), float(fy), g, q, k)


def test_host_equals_the_model_on_the_family(aof, fam):
    got = host(aof, fam)
    assert_same(got, fam["want"], "family")
    # bytes behind a frame's length, and frames of length 0, keep the fill
    idx = np.arange(ref.FRAME_BYTES)[None, None, :] >= got["lengths"][:, :, None]
    assert (got["frames"][idx] == ref.SENTINEL).all() and (got["lengths"] > 0).any() and (got["lengths"] == 0).any()


def test_in_place_records_give_the_same_bytes(aof, fam):
    states, records = fam["states"].copy(), fam["records"].copy()
    out, frames, lengths = aof.bank_imu_host(fam["samples"], fam["counts"], fam["times"], records, states,
                                             first_seq=fam["first_seq"], fill=ref.SENTINEL, records_out=records)
    assert out is records
    assert_same(dict(records=records, frames=frames, lengths=lengths, states=states), fam["want"], "in place")


def test_without_frames_decisions_and_counters_are_the_same(aof, fam):
    got = host(aof, fam, mavlink=False)
    assert got["frames"] is None and got["lengths"] is None
    assert_same(got, fam["want"], "no frames")


def test_rounds_one_by_one_equal_one_call(aof, fam):
    states = fam["states"].copy()
    K = ref.FAMILY_K
    parts = []
    for k in range(K):
        f = dict(samples=fam["samples"][k:k + 1], counts=fam["counts"][k:k + 1], times=fam["times"][k:k + 1],
                 records=fam["records"][k:k + 1], states=states, first_seq=fam["first_seq"])
        r = host(aof, f)
        states = r["states"]
        parts.append(r)
    got = dict(records=np.concatenate([p["records"] for p in parts]), frames=np.concatenate([p["frames"] for p in parts]),
               lengths=np.concatenate([p["lengths"] for p in parts]), states=states)
    assert_same(got, fam["want"], "round by round")


def test_host_equals_the_model_on_100000_random_samples(aof):
    """Rates from normal floats, time steps from {1 .. 60 000} us, every slot taken (counts NULL): 16 x 16 x 400 samples."""
    f = ref.random_family(seed=3, S=400, K=16, M=16, counts="full")
    assert f["samples"].size >= 100000 and f["counts"] is None
    want = ref.run(f["samples"], None, f["times"], f["records"], f["states"], first_seq=f["first_seq"])
    t = want["tally"]
    assert t["accepted"] > 50000 and t["rejected_dt"] > 1000 and t["rejected_rate"] > 50 and t["sent"] > 1000
    assert_same(host(aof, f), want, "random, full")


@pytest.mark.parametrize("S,K,M", [(1, 1, 1), (63, 5, 4), (65, 16, 16), (257, 1, 16)])
def test_host_equals_the_model_on_random_families_with_mixed_counts(aof, S, K, M):
    f = ref.random_family(seed=100 + S + K + M, S=S, K=K, M=M)
    want = ref.run(f["samples"], f["counts"], f["times"], f["records"], f["states"], first_seq=f["first_seq"])
    assert_same(host(aof, f), want, (S, K, M))


def one_stream(samples, kinds, counts=None, offset0=0, M=4, state=None, first_seq=0):
    """A family of one stream from per-round sample lists and record kinds."""
    K = len(kinds)
    rng = np.random.default_rng(5)
    states = np.zeros(1, ref.STATE_DTYPE)
    states["offset_timestamp_usec"] = offset0
    for name, v in (state or {}).items():
        states[name] = v
    c = np.array([[len(r)] for r in samples], np.uint8) if counts is None else np.array(counts, np.uint8).reshape(K, 1)
    return dict(samples=ref.pack_samples([[r] for r in samples], M, 1), counts=c,
                times=np.arange(K, dtype=np.uint64).reshape(K, 1) * np.uint64(13333) + np.uint64(5),
                records=ref.synthetic_records(rng, np.array(list(kinds)).reshape(K, 1)), states=states, first_seq=first_seq)


NAN, INF = float("nan"), float("inf")
T = 10_000_000
EDGES = {
    # name: (family of one stream, the outcomes it must show)
    "accepted": (one_stream([[(T, .1, .2, .3), (T + 2500, .1, -.2, .3)]], "p"), ("accepted", "rejected_prev_zero", "sent")),
    "dt 50000 rejected": (one_stream([[(T, 1, 1, 1), (T + 50000, 1, 1, 1)]], "p"), ("dt_exactly_50000", "rejected_dt")),
    "dt 49999 accepted": (one_stream([[(T, 1, 1, 1), (T + 49999, 1, 1, 1)]], "p"), ("dt_exactly_49999", "accepted")),
    "time backwards": (one_stream([[(T, 1, 1, 1), (T - 1, 1, 1, 1), (T + 10, 1, 1, 1)]], "p"), ("time_backwards", "rejected_dt", "accepted")),
    "rate 20 rejected": (one_stream([[(T, 0, 0, 0), (T + 9, 0, 20.0, 0)]], "p"), ("rate_exactly_20", "rejected_rate")),
    "rate below 20 accepted": (one_stream([[(T, 0, 0, 0), (T + 9, 0, 0, ref.BELOW_20)]], "p"), ("rate_just_below_20", "accepted")),
    "negative rates": (one_stream([[(T, 0, 0, 0), (T + 9, -19.5, 0, 0), (T + 18, -20.0, 0, 0)]], "p"),
                       ("negative_rate_accepted", "negative_rate_rejected")),
    "nan": (one_stream([[(T, 0, 0, 0), (T + 9, NAN, 0, 0), (T + 18, 0, 0, -NAN)]], "p"), ("nan", "rejected_rate")),
    "infinities": (one_stream([[(T, 0, 0, 0), (T + 9, INF, 0, 0), (T + 18, 0, -INF, 0)]], "p"), ("plus_inf", "minus_inf")),
    "time zero": (one_stream([[(0, 1, 1, 1), (T, 1, 1, 1), (T + 9, 1, 1, 1)], [(0, 1, 1, 1), (T + 99, 1, 1, 1)]], "pp"),
                  ("time_zero", "offset_learned", "rejected_prev_zero")),
    "offset preset": (one_stream([[(T, 1, 1, 1)]], "f", offset0=1 << 50), ("offset_preset_sent", "sent_first_frame")),
    "first frame before any sample": (one_stream([[], [(T, 1, 1, 1)]], "fp", offset0=9), ("stale_before_any_sample", "sent_after_stale")),
    "two takes, no sample between": (one_stream([[(T, 1, 1, 1)], [], [(T + 9, 1, 1, 1)]], "ppp"),
                                     ("stale_no_sample_between_takes", "sent_after_stale")),
    "no offset": (one_stream([[], [(T, 1, 1, 1)]], "pp", state=dict(prev_time_usec=T - 9, last_taken_time_usec=T - 99)),
                  ("no_offset", "offset_learned", "sent")),
    "sequence wraps": (one_stream([[(T + 9 * k, 1, 1, 1)] for k in range(4)], "pppp", offset0=9, first_seq=254), ("seq_wrapped",)),
    "counts 0, M, above M": (one_stream([[], [(T + k, 1, 1, 1) for k in range(4)], [(T + 9 + k, 1, 1, 1) for k in range(4)]], "hhp",
                                        counts=[0, 4, 255]), ("count_zero", "count_full", "count_above_max")),
    "idle round with samples": (one_stream([[(T, 1, 1, 1), (T + 9, 1, 1, 1)], [(T + 18, 1, 1, 1)]], "ip"), ("idle_round_with_samples", "idle")),
    "held": (one_stream([[(T, 1, 1, 1), (T + 9, 1, 1, 1)], [(T + 18, 1, 1, 1)]], "hp"), ("held", "sent")),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_host_equals_the_model_on_each_edge(aof, name):
    f, outcomes = EDGES[name]
    want = ref.run(f["samples"], f["counts"], f["times"], f["records"], f["states"], first_seq=f["first_seq"])
    assert all(want["tally"][o] >= 1 for o in outcomes), (name, dict(want["tally"]))
    assert_same(host(aof, f), want, name)
