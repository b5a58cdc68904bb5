"""The stream bank's motion field (include/aof.h, "the stream bank's motion field") as a numpy model: per stream and tick the
gate on the tick record, the pair's fit (field_ref.model: what aof_field_host must give byte for byte), the window's sums in
float64 with one addition each, the float32 casts of a published window and its angles -- what aof_bank_field_host and
k_bank_field.hip must both give byte for byte --, and the builders of the designed runs the tests walk.  Nothing here
imports the product: parameters come as any object or dict with aof_params' field names, and the angle function
(aof_flow_angle of the library: the one fixed sequence of double operations) is handed in."""
import numpy as np

import field_ref as fr
from bank_field_rig import BAD_SENSOR, HELD, IDLE, NO_OFFSET, RECORD_DTYPE, STALE_GYRO, STATE_DTYPE

TICK_DTYPE = np.dtype([("quality", "<i4"), ("dt_us", "<i4"), ("flow_x", "<f4"), ("flow_y", "<f4"), ("gyro_x", "<f4"),
                       ("gyro_y", "<f4"), ("gyro_z", "<f4"), ("frame", "<u4"), ("pixel", fr.FLOW_DTYPE)])
assert TICK_DTYPE.itemsize == 48
SUMS = (("sum_zoom", "zoom"), ("sum_rotation", "rotation"), ("sum_centre_x", "centre_x"), ("sum_centre_y", "centre_y"))
COUNTS = ("pairs", "fits", "used")


def no_frame(q):
    return q in (IDLE, BAD_SENSOR)


def ran_pair(rec):
    return not no_frame(int(rec["quality"])) and int(rec["frame"]) >= 2


def published(q):
    return q >= 0 or q in (STALE_GYRO, NO_OFFSET)


def step_stream(rec, f, focal, state, angle):
    """One stream that has a frame: f the pair's fit (None without a pair); `state` one STATE_DTYPE record, stepped in
    place -> one RECORD_DTYPE record."""
    if f is not None:
        state["pairs"] += 1
        if int(f["flags"]) & fr.VALID:
            state["fits"] += 1
            state["used"] += f["used"]
            for total, part in SUMS:
                state[total] = np.float64(state[total]) + np.float64(f[part])
    out = np.zeros((), RECORD_DTYPE)
    out["status"], out["frame"] = HELD, rec["frame"]
    if published(int(rec["quality"])):
        out["status"], out["dt_us"] = state["fits"], rec["dt_us"]
        for total, part in SUMS:
            out[part] = np.float32(state[total])
            state[total] = 0.0
        out["flow_x"] = angle(float(out["centre_x"]), float(focal[0]))
        out["flow_y"] = angle(float(out["centre_y"]), float(focal[1]))
        for n in COUNTS:
            out[n] = state[n]
            state[n] = 0
        state["published"] += 1
    return out


def step(p, focals, blocks, subdirs, records, state, angle, fp=None):
    """One tick of S streams: blocks [S, nb], subdirs [S, nb] or None (looked at only with a sub-pixel configuration),
    records TICK_DTYPE [S], focals float32 [S, 2], state STATE_DTYPE [S] stepped in place -> (fields [S], out [S])."""
    S = len(records)
    fields, out = np.zeros(S, fr.FIELD_DTYPE), np.zeros(S, RECORD_DTYPE)
    if not fr.vf.par(p, "subpixel"):
        subdirs = None
    for s in range(S):
        rec = records[s]
        f = None
        if ran_pair(rec):
            f = fr.model(p, blocks[s], None if subdirs is None else subdirs[s], rec["pixel"], fp)
            fields[s] = f
        if no_frame(int(rec["quality"])):
            out[s]["status"] = rec["quality"]
            continue
        out[s] = step_stream(rec, f, focals[s], state[s], angle)
    return fields, out


# ---- designed runs -----------------------------------------------------------------------------------------------------
QUALITIES = (200, HELD, HELD, 0, IDLE, 97, STALE_GYRO, HELD, NO_OFFSET, BAD_SENSOR, HELD, 255)


def designed_run(p, S, T, seed=0):
    """T ticks of S streams whose tick records and block records are made up: every quality code on every stream, first
    frames (frame 1, and a frame counter that starts over), every design of field_ref.DESIGNS -- `skipped`, `few` and
    `reach` give invalid fits --, every predictor.  -> (blocks [T, S, nb], subdirs [T, S, nb], records [T, S]).  The
    blocks of a stream without a pair are a design all the same: reading them would show."""
    names = list(fr.DESIGNS)
    nb = fr.coordinates(p)[0].size
    blocks, subdirs = np.zeros((T, S, nb), fr.BLOCK_DTYPE), np.zeros((T, S, nb), np.uint8)
    records = np.zeros((T, S), TICK_DTYPE)
    frame = np.zeros(S, np.int64)
    for t in range(T):
        for s in range(S):
            rng = np.random.default_rng([nb, seed, t, s])
            blocks[t, s], subdirs[t, s] = fr.DESIGNS[names[(t * S + s + seed) % len(names)]](p, rng)
            q = QUALITIES[(3 * s + t + seed) % len(QUALITIES)]
            rec = records[t, s]
            rec["quality"] = q
            if no_frame(q):
                continue                                   # an otherwise zero record
            if (s + 2 * t + seed) % 11 == 10:
                frame[s] = 0                               # the stream was reset: this frame is its first
            frame[s] += 1
            if frame[s] == 1 and q == HELD:
                rec["quality"] = q = 0                     # (a first frame is always published, with quality 0)
            rec["frame"] = frame[s]
            if published(q):
                rec["dt_us"] = int(rng.integers(1, 200000))
            if q >= 0:
                rec["flow_x"], rec["flow_y"] = rng.uniform(-0.02, 0.02, 2)
                rec["gyro_x"], rec["gyro_y"], rec["gyro_z"] = rng.uniform(-0.1, 0.1, 3)
            if frame[s] >= 2:
                px = rec["pixel"]
                px["flow_x"], px["flow_y"] = rng.uniform(-4, 4, 2)
                px["count"], px["quality"], px["flags"] = rng.integers(0, nb + 1), rng.integers(0, 256), rng.integers(0, 4)
                px["pred_x"], px["pred_y"] = fr.PREDICTORS[(s + t) % len(fr.PREDICTORS)]
    return blocks, subdirs, records


def focal_table(S, seed=0):
    """float32 [S, 2]: a focal length pair per stream."""
    rng = np.random.default_rng([7, seed])
    return rng.uniform(80.0, 700.0, (S, 2)).astype(np.float32)
