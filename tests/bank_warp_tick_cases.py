"""What a case of warp_plan_ref.TICK_CASES pushes and what the references say it leaves, worked out on the host alone:
the shape, the parameters, the layout of the sensor planes, the mixed meshes, the run, and per push -- T ticks, then for the
cases that ask for it one burst of K = 3 -- every stream's record, wire bytes, warped crop and exposure histogram from the
numpy model (tests/bank_warp_ref.py) and an oracle chain of its own fed the model's crops.  prepare() also asserts, on the
oracle's records alone, the conditions that keep a case from passing vacuously; tests/test_warp_plan_ref.py runs it for every
case on the CPU, tests/test_gpu_bank_warp_tick_plan.py holds the device to it."""
import numpy as np

import bank_camera_ref as cref
import bank_ref as ref
import bank_warp_ref as wref
import crop_source_ref as csr
import warp_plan_ref as wplan
from bank_ref import FX, FY
from bank_rig import OFFSET
from bank_warp_rig import INTERVAL, RATE, Shape, format_rows, host_buffer, host_model, mixed_meshes_of, planes_run, shape_order, shape_rows

K = 3
COUNTS = np.array([[1, 2, 3, 2, 3], [3, 3, 2, 0, 1]], np.uint8)   # (tests/test_gpu_bank_warp_tick.py: burst 0, burst 1)
REFUSED = 3
SEED = 51   # chosen on the CPU: prepare()'s conditions hold for every case
IDLE, BAD, FRAME = "idle", "bad-sensor", "frame"


def runs_of(case):
    """The (subpixel, pixel format, burst) runs of a case: each of its subpixel values on grey planes (the burst rides on the
    first), then its other formats."""
    out = [(sub, csr.GREY8, case["burst"] and i == 0) for i, sub in enumerate(case["subpixel"])]
    return out + [(case["subpixel"][0], getattr(csr, name), False) for name in case["formats"]]


def every_run():
    return [(c, *r) for c in wplan.TICK_CASES for r in runs_of(c)]


def run_id(c, sub, fmt, burst):
    return c["id"] + ("" if sub else "-integer") + ("" if fmt == csr.GREY8 else "-" + next(n for n in c["formats"] if getattr(csr, n) == fmt).lower())


def shape_of(case):
    return Shape(case["S"], case["w"], case["h"], case["w"] + 32, case["h"] + 16, case["T"])


class Prepared:
    pass


def prepare(aof, orc, synth, case, sub, fmt, burst):
    """Everything of one run but the device."""
    q = Prepared()
    q.case, q.shape, q.fmt, q.burst = case, shape_of(case), fmt, burst
    n, w, h, T = q.shape.S, q.shape.W, q.shape.H, q.shape.T
    q.params = aof.px4flow_params(w, h, pyramid_levels=case["levels"], mean_subtract=case["mean_subtract"], subpixel=sub)
    assert aof.check_params(q.params) == 0
    q.cam = aof.bank_camera_params(w + 8, h + 2, w, h, 0, INTERVAL, cref.DEROTATE, FX, FY)   # (scalars no stream has)
    q.bp = aof.bank_params(n, FX, FY, RATE, OFFSET, 1, 100, 0)
    q.path = wplan.tick_path(case)
    q.rows = None if fmt == csr.GREY8 else format_rows(fmt, q.shape)
    recs, _, q.nbytes = csr.layout(q.rows or shape_rows(q.shape), shape_order(q.shape), w, h)
    q.meshes = mixed_meshes_of(recs, q.shape)
    q.every_other = n - 1 if n == 5 else 2
    q.burst_at = -(-T // K)                                          # the burst behind the ticks: the run's ticks burst_at * K ...
    q.run = planes_run(synth, SEED, q.every_other, q.shape, ticks=(q.burst_at + 1) * K if burst else T)
    q.given = np.zeros((q.burst_at + 1, n), np.uint8)
    q.given[q.burst_at] = COUNTS[1] if n == 5 else COUNTS[1][[0, 1, 4, 3]]   # (four streams: the every-other stream is stream 2)
    # the pushes in order: (run tick, active [S]); a burst's round r is live for a stream's first count rounds
    q.steps = [(k, q.run.active[k].astype(bool)) for k in range(T)]
    if burst:
        q.steps += [(q.burst_at * K + r, r < q.given[q.burst_at]) for r in range(K)]
    times = np.stack([q.run.times[k] for k, _ in q.steps])
    active = np.stack([a for _, a in q.steps]).astype(np.uint8)
    q.due, _ = cref.gate(times, active, INTERVAL)
    chains = [ref.oracle_chain(aof, orc, q.params, RATE, OFFSET, 0) for _ in range(n)]
    q.want = []                                                      # per step, per stream: (kind, record, wire, crop, histogram or None)
    q.plain_differs = np.zeros(n, bool)
    for i, (k, act) in enumerate(q.steps):
        buf = host_buffer(recs, q.nbytes, q.run, k, fmt)
        row = []
        for s in range(n):
            if not act[s]:
                row.append((IDLE, None, b"", None, None))
            elif s == REFUSED:
                row.append((BAD, None, b"", None, None))
            else:
                crop = host_model(buf, recs[s], fmt, q.meshes[s], w, h, q.nbytes)
                q.plain_differs[s] |= not np.array_equal(crop, csr.crop(buf, recs[s], fmt, 1, w, h))
                rec, wire = chains[s].push(crop, q.run.times[k, s], q.run.gyro[k, s])
                row.append((FRAME, rec, wire, crop, wref.histogram(crop) if q.due[i, s] else None))
        q.want.append(row)
    # ---- what keeps the case from passing vacuously, on the references alone
    warped = [s for s in range(n) if s != REFUSED and int(q.meshes[s].reshape(-1)[0]["x"]) != wref.NONE]
    assert len(warped) == n - 2 and not q.plain_differs[0], "one unwarped stream, one refused, the rest warped"
    for s in warped:
        assert q.plain_differs[s], (case["id"], s, "the warped crop is the plain crop")
        assert any(row[s][0] == FRAME and int(row[s][1]["quality"]) > 0 for row in q.want), (case["id"], s, "no record with quality > 0")
    live = [(i, s) for i, row in enumerate(q.want) for s in range(n) if row[s][0] == FRAME]
    assert any(q.due[i, s] for i, s in live) and any(not q.due[i, s] for i, s in live), (case["id"], "due and not-due frames")
    assert any(row[q.every_other][0] == IDLE for row in q.want) and all(row[REFUSED][0] != FRAME for row in q.want)
    return q
