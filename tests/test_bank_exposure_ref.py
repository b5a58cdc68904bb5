"""aof_exposure_control_host (include/aof.h, "the stream bank's auto-exposure control") against the numpy float32 model of
tests/exposure_control_ref.py, bit for bit: on the coverage family (all 17 outcomes of the step, asserted on the model's
tally), on more than 10^5 random steps and on hand-made edges.  CPU only: the function needs no device."""
import numpy as np
import pytest

import exposure_control_ref as xref


def control_of(aof, **kw):
    ec = aof.exposure_control_default()
    for name, value in kw.items():
        setattr(ec, name, value)
    return ec


def same(got_states, got_commands, want_states, want_commands, what):
    for got, want, name in ((got_states, want_states, "states"), (got_commands, want_commands, "commands")):
        if got.tobytes() == want.tobytes():
            continue
        g, w = got.reshape(-1), want.reshape(-1)
        bad = [i for i in range(len(g)) if g[i].tobytes() != w[i].tobytes()]
        raise AssertionError((what, name, "first of", len(bad), "at", bad[0], g[bad[0]], w[bad[0]]))


def host_in_chunks(aof, records, states, ec=None):
    """The host function over [U][S] records, AOF_BANK_BURST_MAX rounds per call; returns (states, commands)."""
    states = states.copy()
    out = [aof.exposure_control_host(records[u:u + aof.BANK_BURST_MAX], states, ec) for u in range(0, len(records), aof.BANK_BURST_MAX)]
    return states, np.concatenate(out)


def test_defaults_are_the_references_constants(aof):
    ec = aof.exposure_control_default()
    assert {n: getattr(ec, n) for n in xref.DEFAULTS} == xref.DEFAULTS      # mainloop.cpp:53-63
    assert aof.lib.aof_exposure_control_default(None) == -22


def test_the_coverage_family_reaches_all_17_outcomes_and_the_host_function_equals_the_model(aof):
    states, msv = xref.family()
    assert msv.shape == (24, 48)
    records = xref.records_of(msv)
    want_states, want_commands, tally = xref.control(records, states)
    assert len(tally) == 17 and all(tally[name] > 0 for name in xref.OUTCOMES), tally      # a condition on the INPUT
    for shape in ((12, 12), (24, 16)):                                                      # (why it is not smaller)
        st, m = xref.family(*shape)
        assert not all(xref.control(xref.records_of(m), st)[2].values()), shape
    got_states, got_commands = host_in_chunks(aof, records, states)
    same(got_states, got_commands, want_states, want_commands, "family")
    assert (want_states["updates"] == 24).all() and (want_commands["update"][-1] == 24).all()
    flags = want_commands["flags"]
    assert (flags & 1).all() and (flags & 2).any() and (flags & 4).any() and (flags == 1).any() and not (flags & 6 == 6).any()


def test_gaps_and_streams_that_are_never_due(aof):
    """Records that are not due change nothing and get an all-zero command; the histogram is never read."""
    states, msv = xref.family()
    rng = np.random.default_rng(11)
    due = rng.random(msv.shape) < 0.6
    due[:, 5] = False
    due[:, 17] = False
    records = xref.records_of(msv, due)
    want_states, want_commands, _ = xref.control(records, states)
    got_states, got_commands = host_in_chunks(aof, records, states)
    same(got_states, got_commands, want_states, want_commands, "gaps")
    assert not got_commands.view(np.uint8).reshape(24, 48, 16)[~due].any()
    assert got_states[5].tobytes() == states[5].tobytes() and got_states[17].tobytes() == states[17].tobytes()
    assert (got_states["updates"] == due.sum(0)).all()
    other = records.copy()
    other["hist"] = 7
    assert host_in_chunks(aof, other, states)[1].tobytes() == got_commands.tobytes()


def test_more_than_1e5_random_steps_equal_the_model(aof):
    """400 streams x 256 updates, every record due: scenes around the target with sigma 0.02, 0.2 and 2, cameras that start
    anywhere in 1..1727 x 1..127."""
    S, U = 400, 256
    rng = np.random.default_rng(2024)
    sigma = rng.choice([0.02, 0.2, 2.0], S)
    centre = rng.choice([5.0, 5.0, 3.5, 6.5], S)
    msv = np.clip(centre + sigma * rng.normal(size=(U, S)), 0, 10).astype(np.float32)
    states = xref.new_states(rng.integers(1, 1728, S), rng.integers(1, 128, S))
    states["gain"][::3] = 1
    records = xref.records_of(msv)
    want_states, want_commands, tally = xref.control(records, states)
    assert sum(tally[n] for n in xref.OUTCOMES[:3]) == S * U >= 100_000
    got_states, got_commands = host_in_chunks(aof, records, states)
    same(got_states, got_commands, want_states, want_commands, "random")


# proportional terms only, in exact binary fractions: e = ce + exposure_p * err and g = cg + gain_p * err without rounding
EXACT = dict(exposure_i=0.0, exposure_d=0.0, gain_i=0.0, gain_d=0.0, gain_p=10.0)
EDGES = [
    # (constants, exposure, gain, msv, flags, exposure behind, gain behind, what)
    (EXACT, 1701, 1, 4.75, 1, 1701, 1, "e = 1726 exactly: not above exposure_max - 1, the step of 25 below the threshold"),
    (EXACT, 1702, 1, 4.75, 3, 1727, 1, "e = 1727 exactly: not clamped, set by the high rule alone"),
    (EXACT, 1727, 1, 5.0, 1, 1727, 1, "ce = e = 1727: saturated, the gain branch, g = 1: nothing to set"),
    (dict(EXACT, exposure_p=96.0), 400, 1, 4.6875, 1, 400, 1, "|e - ce| = 30 exactly: not above the threshold"),
    (dict(EXACT, exposure_p=96.0), 400, 1, 4.65625, 3, 433, 1, "|e - ce| = 33: set"),
    (dict(EXACT, exposure_p=96.0), 400, 1, 5.3125, 1, 400, 1, "|e - ce| = 30 exactly, downwards"),
    (EXACT, 900, 121, 4.5, 1, 900, 121, "g = 126 exactly: not above gain_max - 1"),
    (EXACT, 900, 122, 4.5, 5, 900, 127, "g = 127 exactly: not clamped, set by the high rule alone"),
    (EXACT, 900, 127, 4.5, 1, 900, 127, "cg = gain_max: clamped, nothing to set"),
    (EXACT, 900, 1, 5.0625, 1, 900, 1, "cg = 1: the exposure branch (a step of 6.25 sets nothing)"),
    (EXACT, 900, 2, 5.0625, 5, 900, 1, "cg = 2: the gain branch, g = 1.375 < 2: the low rule sets gain 1"),
    (EXACT, 1727, 1, 4.96875, 1, 1727, 1, "cg = 1 in the gain branch by saturation, g = 1.3125 < 2 but cg is not above 1"),
    (EXACT, 2, 1, 5.0078125, 3, 1, 1, "e = 1.21875 < 2 and ce > 1: the low rule sets exposure 1"),
    (EXACT, 1, 1, 5.5, 1, 1, 1, "e clamped to 1 from ce = 1: nothing to set"),
]


@pytest.mark.parametrize("edge", EDGES, ids=[e[-1].split(":")[0] for e in EDGES])
def test_hand_made_edges(aof, edge):
    constants, exposure, gain, msv, flags, exposure_after, gain_after, what = edge
    ec = control_of(aof, **constants)
    states = xref.new_states([exposure], [gain])
    records = xref.records_of([[msv]])
    want_states, want_commands, _ = xref.control(records, states, xref.constants_of(ec))
    got_states = states.copy()
    got_commands = aof.exposure_control_host(records, got_states, ec)
    same(got_states, got_commands, want_states, want_commands, what)
    c = got_commands[0, 0]
    assert (int(c["flags"]), int(c["exposure"]), int(c["gain"]), int(c["update"])) == (flags, exposure_after, gain_after, 1), what
    assert c["msv_error"] == np.float32(5.0) - np.float32(msv) == c["msv_error_int"]


def test_a_nan_sets_nothing_and_the_integral_has_no_anti_windup(aof):
    states = xref.new_states([400, 1727], [1, 127])
    records = xref.records_of(np.full((16, 2), [np.nan, 0.0], np.float32))
    want_states, want_commands, _ = xref.control(records, states)
    got_states = states.copy()
    got_commands = aof.exposure_control_host(records, got_states)
    same(got_states, got_commands, want_states, want_commands, "nan / windup")
    assert (got_commands["flags"][:, 0] == 1).all() and (got_commands["exposure"][:, 0] == 400).all()
    assert got_states["msv_error_int"][1] == 80.0 and got_states["gain"][1] == 127


def test_what_the_host_function_refuses(aof):
    import ctypes as C
    EINVAL = -22
    call = aof.lib.aof_exposure_control_host
    ec = aof.exposure_control_default()
    records, states = xref.records_of(np.full((2, 3), 4.0)), xref.new_states([5, 6, 7], [1, 1, 1])
    commands = np.full((2, 3), 0xEE, np.uint8).repeat(16).view(xref.COMMAND_DTYPE).reshape(2, 3)
    before = states.copy()
    r, s, c = records.ctypes.data, states.ctypes.data, commands.ctypes.data
    assert call(None, 3, 2, r, s, c) == call(C.byref(ec), 3, 2, None, s, c) == call(C.byref(ec), 3, 2, r, None, c) == EINVAL
    assert call(C.byref(ec), 3, 2, r, s, None) == call(C.byref(ec), 0, 2, r, s, c) == call(C.byref(ec), 3, 0, r, s, c) == EINVAL
    assert call(C.byref(ec), 3, aof.BANK_BURST_MAX + 1, r, s, c) == EINVAL
    for kw in (dict(msv_target=float("nan")), dict(gain_d=float("inf")), dict(exposure_max=0.5), dict(exposure_max=65536.0),
               dict(gain_max=0.0), dict(gain_max=256.0), dict(exposure_change_threshold=float("-inf"))):
        assert call(C.byref(control_of(aof, **kw)), 3, 2, r, s, c) == EINVAL, kw
    assert states.tobytes() == before.tobytes() and (commands.view(np.uint8) == 0xEE).all(), "a refused call writes nothing"
    assert call(C.byref(control_of(aof, exposure_max=65535.0, gain_max=255.0)), 3, 2, r, s, c) == 0
    assert (commands["update"] == [[1] * 3, [2] * 3]).all()
