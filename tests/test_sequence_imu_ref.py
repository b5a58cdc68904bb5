"""aof_sequence_imu_host (include/aof_sequence_imu.h) against the sequential model of tests/sequence_imu_ref.py, byte for
byte; the model against a window worked by hand and against the closed form the kernels use; the host function against
aof_bank_imu_host driven as one stream, a tick per frame; every refusal.  CPU only."""
import collections

import numpy as np
import pytest

import imu_ref as imu
import sequence_imu_ref as ref
import sequence_imu_rig as rig

FILL = 0xEE


@pytest.fixture(scope="module")
def family():
    out = ref.family()
    tally = collections.Counter()
    for r in out:
        r["want"] = ref.run(r, tally)
    return out, tally


def host_run(aof, r):
    """The host function on sentinel-filled outputs -> dict(rc, records, count, frames, lengths, state)."""
    n = r["n"]
    records = r["records"].copy()
    count = np.array([r["M"], 0xEEEEEEEE, 0x77, 0x55], np.uint32)
    frames = np.full((n, ref.FRAME_BYTES), ref.SENTINEL, np.uint8)
    lengths = np.full(n, FILL, np.uint8)
    state = np.full(64, FILL, np.uint8).view(ref.STATE_DTYPE)
    ip = rig.params(len(r["samples"]), r["offset0"], ref.SYSTEM_ID, ref.COMPONENT_ID, r["first_seq"])
    rc = rig.host(aof, ip, n, r["times"], r["samples"], r["sample_end"], records, count, frames, lengths, state)
    return dict(rc=rc, records=records, count=count, frames=frames, lengths=lengths, state=state)


def same_as_model(got, want, r):
    M = r["M"]
    assert got["rc"] == 0, r["name"]
    assert got["records"].tobytes() == want["records"].tobytes(), (r["name"], "records")
    assert got["lengths"][:M].tobytes() == want["lengths"][:M].tobytes(), (r["name"], "lengths")
    assert (got["lengths"][M:] == FILL).all(), (r["name"], "a length behind the last record was written")
    assert got["frames"].tobytes() == want["frames"].tobytes(), (r["name"], "frames, the sentinel behind every length included")
    assert got["count"].tolist() == [M, want["sent"], 0x77, 0x55], (r["name"], "count words")
    assert got["state"].tobytes() == want["state"].tobytes(), (r["name"], "final state", got["state"], want["state"])


def test_one_window_worked_by_hand():
    """Steps of 31 250 us and 15 625 us are 2^-5 s and 2^-6 s: every product and sum below is exact."""
    t0 = 1_000_000
    samples = [(t0, 9.0, 9.0, 9.0),                     # the first sample: no time in front of it, rejected; it sets the offset
               (t0 + 31250, 0.5, -0.25, 2.0),           # + (0.015625, -0.0078125, 0.0625)
               (t0 + 46875, 1.0, 4.0, -1.0),            # + (0.015625, 0.0625, -0.015625)
               (t0 + 96875, 1.0, 1.0, 1.0),             # 50 000 us: not < 0.05 s, rejected
               (t0 + 112500, 20.0, 0.0, 0.0),           # 20 rad/s: rejected
               (t0 + 128125, -2.0, 0.0, 0.5)]           # behind the take: the tail, (-0.03125, 0, 0.0078125)
    r = ref.recording(3, [0, 1], samples, [0, 5, 6], first_seq=7)
    got = ref.run(r)
    rec = got["records"]
    assert int(rec[0]["quality"]) == ref.STALE_GYRO and got["lengths"][0] == 0, "frame 0 before any sample"
    assert (rec[1]["gyro_x"], rec[1]["gyro_y"], rec[1]["gyro_z"]) == (0.03125, 0.0546875, 0.046875)
    assert int(rec[1]["quality"]) == int(r["records"][1]["quality"]) and got["sent"] == 1
    frame = imu.frame(t0 + int(r["times"][1]), int(rec[1]["dt_us"]), rec[1]["flow_x"], rec[1]["flow_y"], (0.03125, 0.0546875, 0.046875),
                      int(rec[1]["quality"]), 7, ref.SYSTEM_ID, ref.COMPONENT_ID)
    assert bytes(got["frames"][1, :got["lengths"][1]]) == frame and (got["frames"][1, len(frame):] == ref.SENTINEL).all()
    s = got["state"][0]
    assert (s["gyro_x"], s["gyro_y"], s["gyro_z"]) == (-0.03125, 0.0, 0.0078125)
    assert (int(s["prev_time_usec"]), int(s["last_taken_time_usec"]), int(s["offset_timestamp_usec"])) == (t0 + 128125, t0 + 112500, t0)
    assert [int(s[n]) for n in ("messages", "samples_integrated", "samples_rejected", "dropped")] == [1, 3, 3, 1]


def test_the_family_reaches_every_outcome_and_never_no_offset(family):
    _, tally = family
    missing = [o for o in ref.OUTCOMES if tally[o] < 1]
    assert not missing, missing
    assert tally["no_offset"] == 0


def test_the_host_function_equals_the_model_on_the_family(aof, family):
    recordings, _ = family
    for r in recordings:
        same_as_model(host_run(aof, r), r["want"], r)


def test_the_host_function_without_a_state_and_with_no_frames(aof):
    r = ref.family()[0]
    want = ref.run(r)
    n = r["n"]
    records, count = r["records"].copy(), np.array([r["M"], 9, 9, 9], np.uint32)
    frames, lengths = np.full((n, 56), ref.SENTINEL, np.uint8), np.zeros(n, np.uint8)
    ip = rig.params(len(r["samples"]), r["offset0"], ref.SYSTEM_ID, ref.COMPONENT_ID, r["first_seq"])
    assert rig.host(aof, ip, n, r["times"], r["samples"], r["sample_end"], records, count, frames, lengths, None) == 0
    assert records.tobytes() == want["records"].tobytes() and frames.tobytes() == want["frames"].tobytes()
    before = records.copy()
    assert rig.host(aof, ip, 0, r["times"], r["samples"], r["sample_end"], records, count, frames, lengths, None) == 0
    assert records.tobytes() == before.tobytes(), "no frames: nothing to do"


def as_one_bank_stream(aof, r):
    """The same recording through aof_bank_imu_host: one stream, K = 1 per frame, unpublished frames as AOF_TICK_HELD records."""
    n, T = r["n"], len(r["samples"])
    states = np.zeros(1, aof.IMU_STATE_DTYPE)
    states["offset_timestamp_usec"] = r["offset0"]
    record_of = {int(f): m for m, f in enumerate(r["records"]["frame"][:r["M"]])}
    out, taken = [], 0
    for k in range(n):
        end = min(T, int(r["sample_end"][k]))
        assert end - taken <= 16
        samples = np.zeros((1, 16, 1), aof.IMU_SAMPLE_DTYPE)
        samples[0, :end - taken, 0] = r["samples"][taken:end]
        tick = np.zeros((1, 1), aof.TICK_DTYPE)
        tick["frame"] = k + 1
        m = record_of.get(k)
        if m is None:
            tick["quality"] = imu.HELD
        else:
            for name in ("quality", "dt_us", "flow_x", "flow_y"):
                tick[name] = r["records"][m][name]
        rec, frames, lengths = aof.bank_imu_host(samples, np.array([[end - taken]], np.uint8), r["times"][k].reshape(1, 1), tick, states,
                                                 ref.SYSTEM_ID, ref.COMPONENT_ID, r["first_seq"], fill=ref.SENTINEL)
        taken = end
        if m is not None:
            out.append((rec[0, 0], frames[0, 0], int(lengths[0, 0])))
    return out, states


def test_the_host_function_equals_the_bank_host_function_driven_as_one_stream(aof):
    records = 0
    for seed in range(60):
        r = ref.random_recording(5000 + seed, max_per_frame=16)
        got = host_run(aof, r)
        bank, states = as_one_bank_stream(aof, r)
        assert got["rc"] == 0 and len(bank) == r["M"]
        for m, (rec, frame, length) in enumerate(bank):
            g = got["records"][m]
            assert int(g["quality"]) == int(rec["quality"]), (seed, m)
            assert all(g[a].tobytes() == rec[a].tobytes() for a in ("gyro_x", "gyro_y", "gyro_z")), (seed, m)
            assert int(got["lengths"][m]) == length and got["frames"][m].tobytes() == frame.tobytes(), (seed, m)
        assert got["state"].tobytes() == states.tobytes(), seed
        records += r["M"]
    assert records > 300


def test_the_closed_form_equals_the_sequential_model_on_400_random_recordings():
    records, stale, sent = 0, 0, 0
    for seed in range(400):
        r = ref.random_recording(seed)
        want, got = ref.run(r), ref.closed_form(r)
        M = r["M"]
        rec = want["records"][:M]
        assert (rec["quality"] == got["quality"]).all(), seed
        assert np.stack([rec["gyro_x"], rec["gyro_y"], rec["gyro_z"]], 1).tobytes() == got["gyro"].tobytes(), seed
        assert ((want["lengths"][:M] > 0) == got["sent"]).all(), seed
        for m in np.flatnonzero(got["sent"]):
            assert want["frames"][m, 4] == got["seq"][m], (seed, m, "sequence number")
            assert int(want["frames"][m, 10:18].view("<u8")[0]) == (got["offset"][m] + int(r["times"][rec["frame"][m]])) & ref.M64
        s = want["state"][0]
        assert [float(s[a]) for a in ("gyro_x", "gyro_y", "gyro_z")] == got["state"]["g"], seed
        for name in ("prev_time_usec", "last_taken_time_usec", "offset_timestamp_usec", "messages", "samples_integrated",
                     "samples_rejected", "dropped"):
            assert int(s[name]) == got["state"][name], (seed, name)
        records += M
        stale += int((got["quality"] == ref.STALE_GYRO).sum())
        sent += int(got["sent"].sum())
    assert records > 3000 and stale > 300 and sent > 1000, (records, stale, sent)


REFUSALS = {
    "null params": dict(ip=None),
    "null times": dict(times=None),
    "null sample_end": dict(sample_end=None),
    "null records": dict(records=None),
    "null count": dict(count=None),
    "null frames": dict(frames=None),
    "null frame_len": dict(lengths=None),
    "null samples with T > 0": dict(samples=None),
    "n_samples negative": dict(n_samples=-1),
    "n_samples 2^32": dict(n_samples=1 << 32),
    "n_frames negative": dict(n=-1),
    "n_frames 2^31 - 16": dict(n=0x7FFFFFF0),
    "more records than frames": dict(count0=9),
    "a record of a frame behind the recording": dict(frame1=8),
    "a decreasing sample_end": dict(decreasing=True),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_the_host_function_refuses_and_writes_nothing(aof, name):
    change = REFUSALS[name]
    r = ref.family()[0]
    n = r["n"]
    a = dict(times=r["times"], samples=r["samples"], sample_end=r["sample_end"].copy(), records=r["records"].copy(),
             count=np.array([change.get("count0", r["M"]), 0xEE, 0xEE, 0xEE], np.uint32),
             frames=np.full((n, 56), FILL, np.uint8), lengths=np.full(n, FILL, np.uint8))
    state = np.full(64, FILL, np.uint8).view(ref.STATE_DTYPE)
    ip = rig.params(change.get("n_samples", len(r["samples"])), r["offset0"], first_seq=r["first_seq"])
    if "frame1" in change:
        a["records"]["frame"][1] = change["frame1"]
    if "decreasing" in change:
        a["sample_end"][3] = a["sample_end"][2] - 1
    before = {k: v.copy() for k, v in a.items()}
    for k in ("times", "samples", "sample_end", "records", "count", "frames", "lengths"):
        if k in change:
            a[k] = None
    rc = rig.host(aof, None if "ip" in change else ip, change.get("n", n), a["times"], a["samples"], a["sample_end"], a["records"],
                  a["count"], a["frames"], a["lengths"], state)
    assert rc == rig.EINVAL
    assert all(v is None or v.tobytes() == before[k].tobytes() for k, v in a.items()) and (state.view(np.uint8) == FILL).all()
