"""The host-side compaction the stream bank's outbox is held to (tests/outbox_ref.py), on the oracle chain of the test
recipe: the input provably holds an empty tick, ticks above a capacity of 8 and ticks below it, and compact() follows
the header's rules.  CPU only."""
import numpy as np
import pytest

import outbox_ref as ob


@pytest.fixture(scope="module")
def recipe(aof, orc, synth):
    return ob.recipe_run(aof, orc, synth)


def test_the_recipe_publishes_what_the_census_says(aof, orc, synth, recipe):
    run, recs, wire, lens, frames = recipe
    assert recs.shape == (24, 37) and recs.size == ob.RECORDS
    per_tick = [int((recs[k]["quality"] >= 0).sum()) for k in range(run.T)]
    assert per_tick == ob.CENSUS_15HZ and sum(per_tick) == ob.PUBLISHED_15HZ
    assert per_tick[10] == 0 and max(per_tick) > 8 > min(c for c in per_tick if c)
    assert [k for k, c in enumerate(per_tick) if c > 8] == [1, 2, 3, 6, 7, 8, 12, 20]
    # every published record was sent, nothing else was
    assert ((lens > 0) == (recs["quality"] >= 0)).all()
    _, recs0, _, _, _ = ob.recipe_run(aof, orc, synth, rate=0)
    assert int((recs0["quality"] >= 0).sum()) == ob.PUBLISHED_RATE0


def test_compact_follows_the_rules_tick_by_tick(aof, recipe):
    run, recs, wire, lens, frames = recipe
    S = run.S
    for k in range(run.T):
        box = ob.compact(recs[k], frames[k], lens[k], None, None, S, 0, tag=k + 1)
        assert box.size == 64 + 128 * S
        header, messages, exposures = aof.outbox_view(box)
        want = np.flatnonzero(recs[k]["quality"] >= 0)
        assert int(header["tag"]) == k + 1 and int(header["n_messages"]) == int(header["messages_found"]) == len(want)
        assert int(header["n_exposures"]) == int(header["exposures_found"]) == 0 and not header["reserved"].any() and len(exposures) == 0
        assert list(messages["stream"]) == list(want) and not messages["round"].any()
        assert messages["record"].tobytes() == recs[k][want].tobytes()
        for m, s in zip(messages, want):
            assert bytes(m["mavlink"][:m["mavlink_len"]]) == wire[k][s] and not m["mavlink"][m["mavlink_len"]:].any()
            assert m["reserved0"] == 0 and not m["reserved1"].any() and not m["derotated"].any()
        assert (box[64 + 128 * len(want):] == ob.FILL).all(), "nothing behind the stored entries"


def test_compact_overflow_null_inputs_and_bursts(aof, recipe):
    run, recs, wire, lens, frames = recipe
    S = run.S
    for k in range(run.T):
        box = ob.compact(recs[k], frames[k], lens[k], None, None, 8, 0)
        full = ob.compact(recs[k], frames[k], lens[k], None, None, S, 0)
        header, messages, _ = aof.outbox_view(box)
        assert int(header["messages_found"]) == ob.CENSUS_15HZ[k] and int(header["n_messages"]) == min(ob.CENSUS_15HZ[k], 8)
        n = int(header["n_messages"])
        assert box[64:64 + 128 * n].tobytes() == full[64:64 + 128 * n].tobytes() and (box[64 + 128 * n:] == ob.FILL).all()
    # the whole run as one [T][S] array (what a burst leaves): round-major order, rounds filled in
    der = np.arange(run.T * S * 2, dtype=np.float32).reshape(run.T, S, 2)
    exp = np.zeros((run.T, S), aof.EXPOSURE_DTYPE)
    exp["due"][::3, ::2] = 1
    exp["msv"] = np.arange(run.T * S, dtype=np.float32).reshape(run.T, S)
    box = ob.compact(recs[:16], frames[:16], lens[:16], exp[:16], der[:16], 200, 50)
    header, messages, exposures = aof.outbox_view(box, 200, 50)
    o = np.flatnonzero(recs[:16]["quality"].reshape(-1) >= 0)
    assert len(messages) == len(o) < 200 and list(messages["round"]) == list(o // S) and list(messages["stream"]) == list(o % S)
    assert messages["derotated"].tobytes() == der[:16].reshape(-1, 2)[o].tobytes()
    oe = np.flatnonzero(exp[:16]["due"].reshape(-1))
    assert int(header["exposures_found"]) == len(oe) > 50 and len(exposures) == 50
    assert exposures["exposure"].tobytes() == exp[:16].reshape(-1)[oe[:50]].tobytes()
    assert list(exposures["round"]) == list(oe[:50] // S) and list(exposures["stream"]) == list(oe[:50] % S)
    # without frames (or without their lengths) the entries carry length 0 and an all-zero frame
    for mav, ln in ((None, None), (None, lens[3]), (frames[3], None)):
        _, messages, _ = aof.outbox_view(ob.compact(recs[3], mav, ln, None, None, S, 0))
        assert len(messages) == ob.CENSUS_15HZ[3] and not messages["mavlink_len"].any() and not messages["mavlink"].any()
