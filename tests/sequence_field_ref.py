"""The sequence pipeline's motion field (include/aof_sequence_field.h) as a numpy model: the SEQUENTIAL rule -- one
aof_bank_field_state walked frame by frame with the stream bank's step (bank_field_ref.step_stream) over the per-pair fits
(field_ref.model) --, the CLOSED FORM the kernels compute (a window per record, read straight from the record frames), and the
builders of the record lists and recordings the tests walk.  Nothing here imports the product: parameters come as any object
or dict with aof_params' field names, and the angle function (aof_flow_angle of the library) is handed in."""
import numpy as np

import bank_field_ref as bf
import field_ref as fr
from bank_field_rig import HELD, NO_OFFSET, RECORD_DTYPE, STALE_GYRO, STATE_DTYPE

SEQ_RECORD_DTYPE = np.dtype([("frame", "<u4"), ("quality", "<i4"), ("dt_us", "<i4"), ("flow_x", "<f4"), ("flow_y", "<f4"),
                             ("gyro_x", "<f4"), ("gyro_y", "<f4"), ("gyro_z", "<f4")])      # aof_seq_record
assert SEQ_RECORD_DTYPE.itemsize == 32
WINDOW_LENGTHS = (1, 2, 5, 63, 64, 65, 4096)
QUALITIES = (200, 0, STALE_GYRO, 97, NO_OFFSET, 255)      # what a record's quality may be once the IMU call has run


# ---- the rule ------------------------------------------------------------------------------------------------------------
def integrate(fields, records, n, focal, angle):
    """The sequential rule on given fits: fields FIELD_DTYPE [n - 1], records SEQ_RECORD_DTYPE [M] -> (out RECORD_DTYPE [M],
    state STATE_DTYPE [1])."""
    state = np.zeros(1, STATE_DTYPE)
    out = np.zeros(len(records), RECORD_DTYPE)
    tick = np.zeros((), bf.TICK_DTYPE)
    m = 0
    for j in range(n):
        record = m < len(records) and int(records[m]["frame"]) == j
        tick["quality"], tick["dt_us"] = (records[m]["quality"], records[m]["dt_us"]) if record else (HELD, 0)
        tick["frame"] = j
        assert not record or bf.published(int(tick["quality"]))
        o = bf.step_stream(tick, fields[j - 1] if j >= 1 else None, focal, state[0], angle)
        if record:
            out[m] = o
            m += 1
    assert m == len(records), "record frames must increase and lie inside the recording"
    return out, state


def _window(fields, lo, hi):
    """(sums [4] float64, pairs, fits, used) of the pairs lo <= k < hi: the valid fits added in pair order from 0.0."""
    sums, fits, used = [np.float64(0.0)] * 4, 0, 0
    for k in range(lo, hi):
        f = fields[k]
        if int(f["flags"]) & fr.VALID:
            fits += 1
            used += int(f["used"])
            sums = [s + np.float64(f[name]) for s, (_, name) in zip(sums, bf.SUMS)]
    return sums, hi - lo, fits, used & 0xFFFFFFFF


def closed_form(fields, records, n, focal, angle):
    """The same without a walk over the frames: window m is the pairs F(m-1) <= k < F(m), F(-1) = 0; the tail window behind
    the last record is the state."""
    M = len(records)
    F = [0] + [int(f) for f in records["frame"]]
    out = np.zeros(M, RECORD_DTYPE)
    for m in range(M):
        sums, pairs, fits, used = _window(fields, F[m], F[m + 1])
        o = out[m]
        o["status"], o["dt_us"], o["frame"] = fits, records[m]["dt_us"], F[m + 1]
        for s, (_, name) in zip(sums, bf.SUMS):
            o[name] = np.float32(s)
        o["flow_x"], o["flow_y"] = angle(float(o["centre_x"]), float(focal[0])), angle(float(o["centre_y"]), float(focal[1]))
        o["pairs"], o["fits"], o["used"] = pairs, fits, used
    state = np.zeros(1, STATE_DTYPE)
    sums, pairs, fits, used = _window(fields, F[M], n - 1) if n >= 1 else ([0.0] * 4, 0, 0, 0)
    for s, (total, _) in zip(sums, bf.SUMS):
        state[total] = s
    state["pairs"], state["fits"], state["used"], state["published"] = pairs, fits, used, M
    return out, state


def run(p, blocks, subdirs, flows, records, n, focal, angle, fp=None):
    """The whole rule: the fits of the n - 1 pairs, then the walk -> (fields, out, state)."""
    if not fr.vf.par(p, "subpixel"):
        subdirs = None
    fields = fr.model_batch(p, blocks, subdirs, flows, fp) if n > 1 else np.zeros(0, fr.FIELD_DTYPE)
    out, state = integrate(fields, records, n, focal, angle)
    return fields, out, state


# ---- record lists ----------------------------------------------------------------------------------------------------------
def record_list(windows, tail, seed=0):
    """Record 0 at frame 0, then one record per window length; `tail` pairs behind the last -> (records [1 + len(windows)], n)."""
    frames = np.concatenate([[0], np.cumsum(np.asarray(windows, np.int64))]).astype(np.int64)
    rng = np.random.default_rng([11, seed, len(frames)])
    rec = np.zeros(len(frames), SEQ_RECORD_DTYPE)
    rec["frame"] = frames
    rec["quality"] = np.array(QUALITIES)[rng.integers(0, len(QUALITIES), len(frames))]
    rec["dt_us"] = rng.integers(1, 300000, len(frames))
    rec["flow_x"], rec["flow_y"] = rng.uniform(-0.02, 0.02, (2, len(frames))).astype(np.float32)
    rec["gyro_x"], rec["gyro_y"], rec["gyro_z"] = rng.uniform(-0.1, 0.1, (3, len(frames))).astype(np.float32)
    return rec, int(frames[-1]) + int(tail) + 1


def random_windows(rng, count, longest=6):
    return rng.integers(1, longest + 1, count).tolist()


def random_fields(n_pairs, seed=0, invalid=0.3):
    """Made-up fits: `invalid` of them without AOF_FIELD_VALID (their floats and counts are there all the same: adding them
    would show)."""
    rng = np.random.default_rng([13, seed, n_pairs])
    f = np.zeros(n_pairs, fr.FIELD_DTYPE)
    f["zoom"], f["rotation"] = rng.normal(0, 0.01, (2, n_pairs)).astype(np.float32)
    f["centre_x"], f["centre_y"] = rng.normal(0, 3.0, (2, n_pairs)).astype(np.float32)
    f["used"], f["fitted"] = rng.integers(8, 26, n_pairs), 25
    f["accepted"] = 25
    f["det"], f["num_zoom"], f["num_rot"] = rng.integers(1, 1 << 40, (3, n_pairs))
    f["flags"] = np.where(rng.random(n_pairs) < invalid, 0, fr.VALID) | np.where(rng.random(n_pairs) < 0.5, fr.REFIT, 0)
    return f


def invalidate(fields, records, which):
    """Takes AOF_FIELD_VALID off every fit of the windows `which` (record indices)."""
    F = [0] + [int(f) for f in records["frame"]]
    for m in which:
        fields["flags"][F[m]:F[m + 1]] &= ~np.uint32(fr.VALID)


# ---- designed recordings: block records for every pair -------------------------------------------------------------------------
INVALID_DESIGNS = ("skipped", "few")      # (`reach` fits under a predictor that moves its blocks off the reach)


def designed_pairs(p, n_pairs, seed=0, invalid_spans=()):
    """(blocks [n_pairs, nb], subdirs [n_pairs, nb], flows [n_pairs]) drawn from a pool of 96 designed pairs of
    field_ref.DESIGNS, every predictor among them; the pairs of invalid_spans [(lo, hi)] hold designs that do not fit."""
    pool_b, pool_s, pool_f = fr.batch(p, 96, seed=seed)
    names = list(fr.DESIGNS)
    bad = np.array([i for i in range(96) if names[i % len(names)] in INVALID_DESIGNS])
    rng = np.random.default_rng([17, seed, n_pairs])
    pick = rng.integers(0, 96, n_pairs)
    for lo, hi in invalid_spans:
        pick[lo:hi] = bad[rng.integers(0, len(bad), hi - lo)]
    flows = pool_f[pick].copy()
    flows["count"] = np.arange(n_pairs) & 0xFFFF        # (never read by the fit)
    return pool_b[pick], pool_s[pick], flows


# ---- the recordings of the end-to-end cases (tests/test_gpu_sequence_field.py; their conditions: tests/test_sequence_field_ref.py) --
E2E = {
    "px4-64-rate15": dict(cls="px4", crop=(64, 64), cam=(160, 120), n=36, rate=15, seed=3, generic=False),
    "px4-64-rate0": dict(cls="px4", crop=(64, 64), cam=(160, 120), n=24, rate=0, seed=5, generic=False),
    "opencv-128-two-levels": dict(cls="opencv", crop=(128, 128), cam=(320, 240), n=24, rate=15, seed=4, generic=False),
    "px4-64-generic-search": dict(cls="px4", crop=(64, 64), cam=(160, 120), n=30, rate=15, seed=8, generic=True),
}


def e2e_params(aof, case):
    cw, ch = case["crop"]
    return aof.px4flow_params(cw, ch) if case["cls"] == "px4" else aof.px4flow_params(cw, ch, pyramid_levels=2, mean_subtract=1)


def e2e_recording(synth, case):
    """(camera frames [n, cam_h, cam_w], times int64 [n]): a camera that climbs (a steady zoom about the frame centre, which is
    the crop's, with a small pan) for the first two thirds, then yaws (chains of zooming and rotating pairs); ~75 fps with
    jitter."""
    w, h = case["cam"]
    n, seed = case["n"], case["seed"]
    climb = 2 * n // 3
    frames = [synth.make_camera_sequence(w, h, climb, seed=50 + seed, max_step=1, zoom_q16=300)[0]]
    pairs = [synth.make_warp_pair(w, h, reach=2, pair_index=10 * seed + k, noise=2) for k in range((n - climb + 1) // 2)]
    frames.append(np.stack([f for q in pairs for f in (q[0], q[1])])[:n - climb])
    rng = np.random.default_rng(200 + seed)
    times = np.cumsum(np.concatenate([[0], rng.integers(12000, 15000, n - 1)])).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(frames)), times
