"""The CPU side of tests/test_gpu_sequence_limiter.py: the host model of the sequence limiter (tests/sequence_limiter_ref.py)
against the ORACLE's calcFlow chain driven frame by frame (sequence_ref.replay), records and wire frames byte for byte, on
the period's edges and the 32-bit time arithmetic; and every time-stamp design against the chain and the census it was
built for -- on the model, before any device sees it."""
import numpy as np
import pytest

import sequence_limiter_ref as lr
from mavlink_model import py_frame
from sequence_ref import replay

FX, FY = 216.6677, 216.2457
OFFSET = 5_000_000
EDGES = lr.period_edges()
DARK_SEGMENTS = ((28, 41), (100, 103))      # every-third: the segments (30, 33], (33, 36] and (36, 39] are dark throughout


@pytest.fixture(scope="module")
def recording(aof, orc, synth):
    base, _ = synth.make_sequence(64, 64, 64, 4, seed=31, max_step=3)
    return dict(base=base, po=orc.params_from(aof.px4flow_params(64, 64)), memo={})


def check_design(d):
    n = len(d.times)
    chain, status = lr.chain_of(d.times, d.rate)
    assert chain == d.chain, "the model walks the chain the design was built for"
    assert status == d.status
    assert lr.census_of(chain, n) == d.census
    return chain


@pytest.mark.parametrize("name", sorted(EDGES))
def test_model_equals_the_oracle_chain(orc, recording, name):
    d = EDGES[name]
    n = len(d.times)
    check_design(d)
    ids = lr.frame_ids(n, DARK_SEGMENTS)
    frames = lr.frames_of(recording["base"], ids)
    gyro = lr.gyro_of(n)
    o = orc.Px4(recording["po"], FX, FY, d.rate)
    want, wire = replay(o.calc_flow, frames, d.times, gyro, OFFSET, 250, py_frame)
    flows = lr.flows_of(orc, recording["po"], recording["base"], ids, recording["memo"])
    for k in (0, 29, 30, 63, 150):
        assert flows[k].tobytes() == orc.flow_pair(recording["po"], frames[k], frames[k + 1])["flow"].tobytes(), k
    recs, status = lr.limiter_model(d.times, flows, gyro, d.rate, FX, FY, angle=orc.angle)
    assert status == 0
    assert recs.tobytes() == lr.records_of_replay(want).tobytes()
    assert lr.wire_of(recs, d.times, OFFSET, 250) == wire
    assert len(recs) == d.census["records"] >= 100
    if name in ("backwards-step", "jump-2-to-31", "u32-wrap"):
        assert (recs["dt_us"] < 0).sum() == 1, "one publication behind a time step of 2^31 or more, read as int32"
    if name == "every-third":
        dark = recs[(recs["frame"] >= 33) & (recs["frame"] <= 39)]
        assert len(dark) == 3 and (dark["quality"] == 0).all(), "whole segments without a valid frame publish quality 0"
        assert (recs["quality"] > 0).sum() > 50


def test_model_without_an_offset_or_a_gyro_and_on_short_recordings(orc, recording):
    d = EDGES["every-third"]
    assert lr.wire_of(np.zeros(3, lr.RECORD_DTYPE), d.times, 0, 250) == []
    for n in (1, 2, 3):
        ids = lr.frame_ids(n)
        flows = lr.flows_of(orc, recording["po"], recording["base"], ids, recording["memo"])
        assert len(flows) == n - 1
        for rate in (0, 15):
            times = np.arange(n, dtype=np.int64) * lr.STEP
            frames = lr.frames_of(recording["base"], ids)
            o = orc.Px4(recording["po"], FX, FY, rate)
            want, wire = replay(o.calc_flow, frames, times, lr.gyro_of(n), OFFSET, 254, py_frame)
            recs, status = lr.limiter_model(times, flows, lr.gyro_of(n), rate, FX, FY, angle=orc.angle)
            assert status == 0 and recs.tobytes() == lr.records_of_replay(want).tobytes()
            assert lr.wire_of(recs, times, OFFSET, 254) == wire


# ---- the census of every design ----------------------------------------------------------------------------------------
COUNTS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385)
STRIDES = (2, 3, 5, 7, 64, 255, 256, 257)


def test_every_frame_designs_change_the_round_at_each_power_of_four():
    for n in COUNTS:
        d = every_frame = lr.every_frame(n)
        check_design(d)
        assert d.census == dict(records=n, rounds=lr.rounds_of(n), largest_gap=1 if n > 1 else 0, tail=0)
        assert lr.chain_of(every_frame.times, 0) == (list(range(1, n)), 0)
    assert [lr.rounds_of(n) for n in (1, 3, 4, 15, 16, 255, 256, 4095, 4096, 16383, 16384)] == [1, 1, 2, 2, 3, 4, 5, 6, 7, 7, 8]


@pytest.mark.parametrize("g", STRIDES)
def test_strided_designs(g):
    for r in (1, 2, 3, 4):
        for records in (4 ** r - 1, 4 ** r, 4 ** r + 1):
            for tail in (0, 1, g - 1):
                d = lr.strided(g, records, tail)
                check_design(d)
                n = (records - 1) * g + 1 + tail
                assert len(d.times) == n and np.all(np.diff(d.times) > 0)
                assert d.census == dict(records=records, rounds=lr.rounds_of(n), largest_gap=g, tail=tail)


@pytest.mark.parametrize("i", [0, 37])
def test_scan_window_designs(i):
    found = lr.gap(i, 4096, 3)
    check_design(found)
    assert found.status == 0 and found.census["largest_gap"] == 4096 and found.census["records"] == i + 4 and found.census["tail"] == 0
    lost = lr.gap(i, 4097, 3)
    check_design(lost)
    assert lost.status == lr.STALLED and lost.census["records"] == i + 1 and lost.census["tail"] == 4097 + 2
    fits = lr.held_to_end(i, 4096)
    check_design(fits)
    assert fits.status == 0 and len(fits.times) == i + 1 + 4096 and fits.census["tail"] == 4096
    over = lr.held_to_end(i, 4097)
    check_design(over)
    assert over.status == lr.STALLED and len(over.times) == i + 2 + 4096 and over.census["records"] == i + 1


def test_off_chain_stall_design():
    d = lr.off_chain_stall()
    chain = check_design(d)
    assert d.status == 0 and d.census["records"] == 1711 and d.census["largest_gap"] == 3991 and len(d.times) == 6000
    assert np.all(np.diff(d.times) >= 0), "monotonic time stamps"
    lone = lr.off_chain_stallers(d.times, d.rate)
    assert len(lone) == 154 and lone[0] == 51 and not set(lone) & set([0] + chain), "only frames that are NOT on the chain stall"


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_irregular_designs(seed):
    d = lr.irregular(seed)
    check_design(d)
    gaps = np.diff([0] + d.chain)
    assert len(d.times) == 9000 and gaps.min() >= 1 and 250 < gaps.max() <= 300 and len(set(gaps.tolist())) > 40
    assert d.census["rounds"] == 7 and d.census["tail"] < 300
