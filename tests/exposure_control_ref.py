"""The auto-exposure controller of include/aof.h ("the stream bank's auto-exposure control"; the reference's
_exposure_update, mainloop.cpp:222-271) restated in numpy float32 scalars: every operation rounded on its own, in the
order the header gives.  control() runs [K][S] exposure records over S states and returns the states, the commands and a
tally of which outcomes occurred; family() makes the inputs that reach all of them.  Nothing here touches the GPU or the
library (the dtypes are restated, so that the library's are checked against them)."""
import numpy as np

F = np.float32

STATE_DTYPE = np.dtype([("msv_error_old", "<f4"), ("msv_error_int", "<f4"), ("exposure", "<u2"), ("gain", "u1"),
                        ("reserved", "u1"), ("updates", "<u4")])
COMMAND_DTYPE = np.dtype([("exposure", "<u2"), ("gain", "u1"), ("flags", "u1"), ("msv_error", "<f4"), ("msv_error_int", "<f4"),
                          ("update", "<u4")])
RECORD_DTYPE = np.dtype([("hist", "<u4", (10,)), ("msv", "<f4"), ("due", "<u4")])
UPDATED, SET_EXPOSURE, SET_GAIN = 1, 2, 4

DEFAULTS = dict(msv_target=5.0, exposure_p=100.0, exposure_i=0.5, exposure_d=0.5, gain_p=50.0, gain_i=0.5, gain_d=0.5,
                exposure_change_threshold=30.0, exposure_max=1727.0, gain_change_threshold=15.0, gain_max=127.0)

# Which way a step went.  The branch taken (3), and per branch where the clamp left the value (3) and which rule, tried in
# the order of the condition, set it -- the change threshold, else the low rule alone, else the high rule alone -- or none (4).
OUTCOMES = (("branch_gain_by_gain", "branch_gain_by_saturation", "branch_exposure") +
            tuple(f"{v}_{o}" for v in ("gain", "exposure")
                  for o in ("clamped_high", "clamped_low", "unclamped", "set_by_threshold", "set_by_low_alone", "set_by_high_alone",
                            "not_set")))
assert len(OUTCOMES) == 17


class Constants:
    def __init__(self, **kw):
        for name, value in {**DEFAULTS, **kw}.items():
            setattr(self, name, F(value))


def constants_of(ec):
    """From the library's ExposureControl structure (or anything with the same attributes)."""
    return Constants(**{name: getattr(ec, name) for name in DEFAULTS})


def step(c, st, msv, tally):
    """One step on the state record st (a numpy void of STATE_DTYPE, changed in place); returns the command fields."""
    msv = F(msv)
    err = F(c.msv_target - msv)
    d = F(err - st["msv_error_old"])
    integral = F(st["msv_error_int"] + err)
    ce, cg = F(st["exposure"]), F(st["gain"])
    e = F(ce + F(F(F(c.exposure_p * err) + F(c.exposure_i * integral)) + F(c.exposure_d * d)))
    flags = UPDATED
    one, two = F(1), F(2)
    by_gain = cg > one
    if by_gain or (e > F(c.exposure_max - one) and ce > F(c.exposure_max - one)):
        tally["branch_gain_by_gain" if by_gain else "branch_gain_by_saturation"] += 1
        g = F(cg + F(F(F(c.gain_p * err) + F(c.gain_i * integral)) + F(c.gain_d * d)))
        if g > c.gain_max:
            g = c.gain_max
            tally["gain_clamped_high"] += 1
        elif g < one:
            g = one
            tally["gain_clamped_low"] += 1
        else:
            tally["gain_unclamped"] += 1
        rules = (np.abs(F(g - cg)) > c.gain_change_threshold, g < two and cg > one, g > F(c.gain_max - one) and cg < c.gain_max)
        if any(rules):
            st["gain"] = np.uint8(int(g))      # truncation
            flags |= SET_GAIN
        tally["gain_" + ("set_by_threshold" if rules[0] else "set_by_low_alone" if rules[1] else "set_by_high_alone" if rules[2]
                         else "not_set")] += 1
    else:
        tally["branch_exposure"] += 1
        if e > c.exposure_max:
            e = c.exposure_max
            tally["exposure_clamped_high"] += 1
        elif e < one:
            e = one
            tally["exposure_clamped_low"] += 1
        else:
            tally["exposure_unclamped"] += 1
        rules = (np.abs(F(e - ce)) > c.exposure_change_threshold, e < two and ce > one,
                 e > F(c.exposure_max - one) and ce < c.exposure_max)
        if any(rules):
            st["exposure"] = np.uint16(int(e))
            flags |= SET_EXPOSURE
        tally["exposure_" + ("set_by_threshold" if rules[0] else "set_by_low_alone" if rules[1] else "set_by_high_alone" if rules[2]
                             else "not_set")] += 1
    st["msv_error_old"] = err
    st["msv_error_int"] = integral
    st["updates"] = np.uint32((int(st["updates"]) + 1) & 0xFFFFFFFF)
    return (st["exposure"], st["gain"], flags, err, integral, st["updates"])


def control(records, states, constants=None):
    """records: RECORD_DTYPE [K, S] (or [S]); states: STATE_DTYPE [S] (not changed).  Returns (states behind the call,
    commands in the shape of records, tally {outcome: count})."""
    c = constants or Constants()
    records = np.asarray(records)
    shape = records.shape
    recs = records.reshape(-1, shape[-1])
    K, S = recs.shape
    states = np.array(states, dtype=STATE_DTYPE, copy=True)
    assert states.shape == (S,)
    commands = np.zeros((K, S), COMMAND_DTYPE)
    tally = {name: 0 for name in OUTCOMES}
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(K):
            for s in range(S):
                if recs[k, s]["due"]:
                    commands[k, s] = step(c, states[s], recs[k, s]["msv"], tally)
    return states, commands.reshape(shape), tally


def new_states(exposure, gain):
    """States as aof_bank_exposure_reset_device leaves them."""
    exposure = np.asarray(exposure)
    st = np.zeros(exposure.shape, STATE_DTYPE)
    st["exposure"], st["gain"] = exposure, gain
    return st


def records_of(msv, due=None):
    """RECORD_DTYPE in the shape of msv: due records carry their msv (and a histogram the controller must not read),
    records that are not due are all zero, as a camera push writes them."""
    msv = np.asarray(msv, dtype=np.float32)
    r = np.zeros(msv.shape, RECORD_DTYPE)
    due = np.ones(msv.shape, bool) if due is None else np.asarray(due, bool)
    r["msv"] = np.where(due, msv, 0)
    r["due"] = due
    r["hist"][due] = 0xDEAD
    return r


# ---- the coverage family ---------------------------------------------------------------------------------------------
# Six kinds of camera repeat over the streams: where the camera starts, and the scene's mean sample value, which flips
# to 10 - base half way through (a dark scene turns bright and back), under Gaussian noise of sigma 0.15.
KINDS = (((1, 1), 7.5), ((20, 1), 4.9), ((400, 1), 5.02), ((1700, 1), 3.0), ((1727, 1), 2.0), ((1727, 90), 8.0))


def family(n_streams=48, n_updates=24, seed=7):
    """(states [S], msv [U, S] float32): 48 x 24 with seed 7 reaches all 17 outcomes (12 x 12 and 24 x 16 do not)."""
    rng = np.random.default_rng(seed)
    kind = np.arange(n_streams) % len(KINDS)
    base = np.array([KINDS[k][1] for k in kind])
    level = np.where(np.arange(n_updates)[:, None] < n_updates // 2, base[None, :], 10.0 - base[None, :])
    msv = np.clip(level + rng.normal(0.0, 0.15, (n_updates, n_streams)), 0.0, 10.0).astype(np.float32)
    states = new_states([KINDS[k][0][0] for k in kind], [KINDS[k][0][1] for k in kind])
    return states, msv
