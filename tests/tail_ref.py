"""The tail matrix (tests/test_tail_ref.py, tests/test_gpu_tail_matrix.py): focal lengths, output rates and motions that
take the published angle -- aof_atan2f(px, focal), include/aof_math.h -- through every branch of its code, and the rate
limiter through windows of 75 frames and more.  Here: the branch structure restated (angle_class), frames that move by
whole pixels (steady_sequence), the cases with their inputs for the sequence pipeline and for the stream bank, and the
census of an oracle chain: which branch every published angle takes, with the pixel sums recomputed from orc.flow_pair
and held to the chain's own angles.  Every condition is on the ORACLE's records.  Nothing here touches the GPU."""
from collections import Counter

import numpy as np

import bank_ref as ref
from bank_rig import OFFSET, params_of
from mavlink_model import py_frame
from sequence_ref import crop_of, replay

TAN_PI_8 = 0.41421356237309504880            # aof_math.h's constant: the same double
CLASSES = ("direct", "reduced", "equal", "swapped_reduced", "swapped_direct")
K_BURST = 5


def angle_class(px, focal):
    """(class, sign of px) of aof_atan2f(px, focal) for focal > 0, in the function's own arithmetic: both floats widened
    to double, t = lo / hi in double, t against tan(pi/8), lo == hi, |px| against focal.  sign: -1, 0, +1."""
    y, x = float(np.float32(px)), float(np.float32(focal))
    assert x > 0.0 and y == y
    ay = abs(y)
    lo, hi = (x, ay) if x < ay else (ay, x)
    sign = (y > 0.0) - (y < 0.0)
    if lo == hi:
        return "equal", sign
    folded = lo / hi > TAN_PI_8
    if ay > x:
        return ("swapped_reduced" if folded else "swapped_direct"), sign
    return ("reduced" if folded else "direct"), sign


def steady_sequence(w, h, n, velocity, seed):
    """n crops [n, h, w] u8 of ONE texture (uniform noise under a 3 x 3 box, integer arithmetic), the window moving by
    velocity = (vx, vy) whole pixels per frame: every pair is an exact translation."""
    vx, vy = int(velocity[0]), int(velocity[1])
    W, H = w + abs(vx) * (n - 1), h + abs(vy) * (n - 1)
    noise = np.random.default_rng(seed).integers(0, 256, (H + 2, W + 2)).astype(np.uint32)
    tex = (sum(noise[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) // 9).astype(np.uint8)
    x0, y0 = (0 if vx >= 0 else W - w), (0 if vy >= 0 else H - h)
    return np.stack([tex[y0 + k * vy:y0 + k * vy + h, x0 + k * vx:x0 + k * vx + w] for k in range(n)])


# ---- the cases -------------------------------------------------------------------------------------------------------
# motion: None = synth.make_sequence(..., max_step=3), else the velocity of steady_sequence.  n: frames of the sequence
# pipeline's recording; T: ticks of the bank's run (S streams, each active in four ticks of five: bank_ref.make_run).
# reaches: the classes the case is there for ("zero": a published angle with px == 0 behind a first frame).
FX, FY = ref.FX, ref.FY

CASES = [
    dict(id="short-focal", fx=12.0, fy=3.0, rate=15, motion=None, cfg="px4-64", n=90, T=50, S=5, seed=3, facade=True, camera=True,
         reaches=("reduced", "equal", "swapped_reduced", "swapped_direct")),
    dict(id="focal-equals-flow", fx=2.0, fy=2.0, rate=0, motion=(2, -2), cfg="px4-64", n=48, T=50, S=5, seed=4,
         reaches=("equal",)),
    dict(id="sub-pixel-focal", fx=2.0, fy=0.5, rate=0, motion=None, cfg="px4-64", n=48, T=50, S=5, seed=5,
         reaches=("swapped_direct", "zero")),
    dict(id="slow-rate", fx=FX, fy=FY, rate=1, motion=(4, -3), cfg="px4-64", n=330, T=330, S=5, seed=6, facade=True, camera=True,
         reaches=("swapped_reduced",)),
    dict(id="slow-rate-two-level", fx=FX, fy=FY, rate=2, motion=(4, -3), cfg="opencv-128", n=150, T=150, S=4, seed=7,
         reaches=("reduced",)),
    dict(id="long-focal", fx=4000.0, fy=0.25, rate=15, motion=None, cfg="px4-64", n=90, T=50, S=5, seed=8,
         reaches=("direct", "swapped_direct")),
]
BY_ID = {c["id"]: c for c in CASES}
LONG_WINDOW = 75            # summed frames behind a slow-rate publication


def sensor_of(cfg):
    return (160, 120) if cfg == "px4-64" else (320, 240)


def sequence_inputs(synth, aof, case):
    """The recording of the sequence pipeline: sensor frames [n, cam_h, cam_w], times [n] (9..18 ms apart), gyro [n, 4]
    (test_gpu_sequence.make_inputs' recipe)."""
    cam_w, cam_h = sensor_of(case["cfg"])
    n, seed = case["n"], case["seed"]
    rng = np.random.default_rng(100 + seed)
    times = np.cumsum(np.concatenate([[0], rng.integers(9000, 18000, n - 1)])).astype(np.int64)
    if case["motion"] is None:
        frames, _ = synth.make_sequence(cam_w, cam_h, n, 4, seed=seed, max_step=3)
    else:
        frames = steady_sequence(cam_w, cam_h, n, case["motion"], seed)
    rng = np.random.default_rng(seed)
    gyro = np.zeros((n, 4), np.float32)
    gyro[:, :3] = rng.normal(0, 0.004, (n, 3)).astype(np.float32)
    gyro[:, 3] = np.clip(np.diff(np.concatenate([[0], times])).astype(np.float64) * 1e-6, 0, 1).astype(np.float32)
    return frames, times, gyro


def stream_source(case, w, h):
    """bank_ref.make_run's per-stream sequence source of a case (None: its own make_sequence)."""
    if case["motion"] is None:
        return None
    return lambda s, T: steady_sequence(w, h, T, case["motion"], 1000 * case["seed"] + s)


def bank_run(synth, aof, case):
    p = params_of(aof, case["cfg"])
    return ref.make_run(synth, p.width, p.height, case["S"], case["T"], case["seed"], source=stream_source(case, p.width, p.height))


def burst_run(run, K=K_BURST):
    """The same streams in bursts of K rounds: every stream's frames, times and gyro samples in their order, dealt out
    count[j, s] = 0..K at a time (seeded; stream 0 has all K rounds of burst 0) to the first rounds of burst j -- a burst's
    active rounds are its first count[s] -- until every stream has run dry.  Returns (Run of B*K ticks, counts [B, S],
    given [B, S]: one full count replaced by a value above K, which counts as K)."""
    S = run.S
    rng = np.random.default_rng(run.T * 31 + S)
    mine = [np.flatnonzero(run.active[:, s]) for s in range(S)]
    at, rows = [0] * S, []
    while any(at[s] < len(mine[s]) for s in range(S)):
        c = rng.integers(0, K + 1, S)
        if not rows:
            c[0] = K
        rows.append([min(int(c[s]), len(mine[s]) - at[s]) for s in range(S)])
        at = [at[s] + rows[-1][s] for s in range(S)]
    counts = np.array(rows, np.uint8)
    B = len(rows)
    shape = lambda a: (B * K,) + a.shape[1:]
    frames = rng.integers(0, 256, shape(run.frames), dtype=np.uint8)        # idle rounds hold noise
    times = rng.integers(0, 1 << 40, shape(run.times)).astype(np.int64)
    gyro = rng.normal(0, 1.0, shape(run.gyro)).astype(np.float32)
    active = np.zeros(shape(run.active), np.uint8)
    at = [0] * S
    for j in range(B):
        for s in range(S):
            c = int(counts[j, s])
            ticks, dst = mine[s][at[s]:at[s] + c], slice(j * K, j * K + c)
            frames[dst, s], times[dst, s], gyro[dst, s], active[dst, s] = run.frames[ticks, s], run.times[ticks, s], run.gyro[ticks, s], 1
            at[s] += c
    given = counts.copy()
    given[tuple(np.argwhere(counts == K)[-1])] = 200
    return ref.Run(frames, times, gyro, active), counts, given


# ---- the census ------------------------------------------------------------------------------------------------------
def census(orc, po, frames, published, fx, fy, rate):
    """One stream.  frames [n, h, w]: what the chain was fed, in order; published: [(k, angle_x, angle_y)] of the chain's
    publications behind frame 0 (k: index into frames).  Recomputes the limiter's sums from orc.flow_pair in frame order
    in float32 (rate <= 0: the pair's own flow), asserts that orc.angle(sum, focal) IS the chain's angle, and returns
    (Counter {(axis, class, sign): n}, [(k, sum_x, sum_y, summed frames)])."""
    counts, sums = Counter(), []
    pub = {int(k): (ax, ay) for k, ax, ay in published}
    sx = sy = np.float32(0)
    summed = 0
    for k in range(1, len(frames)):
        f = orc.flow_pair(po, frames[k - 1], frames[k])["flow"]
        if rate <= 0:
            sx, sy, summed = np.float32(f["flow_x"]), np.float32(f["flow_y"]), 1
        elif f["quality"] > 0:
            sx, sy, summed = np.float32(sx + f["flow_x"]), np.float32(sy + f["flow_y"]), summed + 1
        if k not in pub:
            continue
        for axis, s, focal, ang in (("x", sx, fx, pub[k][0]), ("y", sy, fy, pub[k][1])):
            assert np.float32(orc.angle(float(s), focal)).tobytes() == np.float32(ang).tobytes(), (k, axis, s, focal, ang)
            counts[(axis,) + angle_class(s, focal)] += 1
        sums.append((k, sx, sy, summed))
        sx = sy = np.float32(0)
        summed = 0
    assert len(sums) == len(pub), "every publication lies inside the frames"
    return counts, sums


def census_of_records(orc, po, run, want, fx, fy, rate):
    """census() of every stream of a bank run and its oracle records [T, S]: (Counter, sums of all streams)."""
    counts, sums = Counter(), []
    for s in range(run.S):
        act = run.active[:, s] == 1
        recs = want[act, s]
        pub = [(i, r["flow_x"], r["flow_y"]) for i, r in enumerate(recs) if i >= 1 and r["quality"] >= 0]
        c, m = census(orc, po, run.frames[act, s], pub, fx, fy, rate)
        counts.update(c)
        sums += m
    return counts, sums


def by_class(counts):
    """{(class, sign): n} over both axes."""
    out = Counter()
    for (_, cls, sign), n in counts.items():
        out[(cls, sign)] += n
    return out


def check_reaches(case, counts, sums):
    """The conditions on ONE case's oracle records: every class its row names at least once; slow-rate: at least two
    publications whose window holds >= 75 summed frames and whose |sum x| exceeds the focal length."""
    seen = by_class(counts)
    for cls in case["reaches"]:
        if cls == "zero":
            assert seen[("direct", 0)] >= 1, (case["id"], "no published angle with px == 0", dict(seen))
        else:
            assert sum(seen[(cls, sign)] for sign in (-1, 0, 1)) >= 1, (case["id"], "does not reach", cls, dict(seen))
    if case["id"] == "slow-rate":
        long = [m for m in sums if m[3] >= LONG_WINDOW and abs(float(m[1])) > float(np.float32(case["fx"]))]
        assert len(long) >= 2, (case["id"], "publications behind long windows", [(m[0], float(m[1]), m[3]) for m in sums])


_cache = {}


def oracle_of_sequence(aof, orc, synth, case):
    """The sequence pipeline's recording of a case and what the oracle chain leaves of it, made once: dict(frames, times,
    gyro, cropped, recs, wire, counts, sums) -- recs and wire as sequence_ref.replay returns them."""
    key = ("sequence", case["id"])
    if key not in _cache:
        p = params_of(aof, case["cfg"])
        frames, times, gyro = sequence_inputs(synth, aof, case)
        cropped = crop_of(frames, p.width, p.height)
        po = orc.params_from(p)
        o = orc.Px4(po, case["fx"], case["fy"], case["rate"])
        recs, wire = replay(o.calc_flow, cropped, times, gyro, OFFSET, 250, py_frame)
        counts, sums = census(orc, po, cropped, [(r[0], r[3], r[4]) for r in recs if r[0] >= 1], case["fx"], case["fy"], case["rate"])
        _cache[key] = dict(frames=frames, times=times, gyro=gyro, cropped=cropped, recs=recs, wire=wire, counts=counts, sums=sums)
    return _cache[key]


def oracle_of_bank(aof, orc, synth, case):
    """The bank run of a case and its oracle records, made once: dict(run, want, wire, counts, sums)."""
    key = ("bank", case["id"])
    if key not in _cache:
        p = params_of(aof, case["cfg"])
        run = bank_run(synth, aof, case)
        chains = [ref.oracle_chain(aof, orc, p, case["rate"], OFFSET, 0, fx=case["fx"], fy=case["fy"]) for _ in range(run.S)]
        want, wire = ref.expected(run, chains)
        counts, sums = census_of_records(orc, orc.params_from(p), run, want, case["fx"], case["fy"], case["rate"])
        _cache[key] = dict(run=run, want=want, wire=wire, counts=counts, sums=sums)
    return _cache[key]
