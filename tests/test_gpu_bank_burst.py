"""The stream bank in bursts (aof_bank_push_burst_device / aof_bank_push_camera_burst_device, include/aof.h): K frame
rounds per stream in one call must leave, byte for byte, what K calls of the single-tick entry point leave on a twin
bank -- call k with round k's buffers and d_active[s] = (k < count[s]) -- and what the CPU oracle's chain per stream
leaves (tests/bank_ref.py, tests/bank_camera_ref.py driven round by round with the same activity rule), so that the
feature is not held to the library's own tick alone.  Every case first asserts, on the oracle chain and before the
device is compared, that its input meets the situations it is there for (census()).  Every comparison is on raw
bytes; every output buffer is pre-filled with 0xEE (wire frames with 0).  The rig: tests/bank_rig.py; the cases:
tests/bank_cases.py."""
import ctypes as C

import numpy as np
import pytest

import bank_camera_ref as cref
import bank_ref as ref
from bank_cases import Case
from bank_ref import FX, FY
from bank_rig import EINVAL, EIO, ENOSPC, OFFSET, BankRig, params_of, untouched
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

BASIC = ("first-frame-then-more", "count0", "publication-before-the-last-round", "held")
GATE = ("gate-opens-in-a-later-round-and-stays-shut",)

CASES = [
    dict(id="px4-64-K5", cfg="px4-64", K=5, seed=1, needs=BASIC + ("zero-quality-frame-skipped",)),
    dict(id="px4-64-K1", cfg="px4-64", K=1, B=24, seed=2, needs=("count0", "held")),
    dict(id="px4-64-K16-wrap", cfg="px4-64", K=16, B=3, seed=3, wrap=True, needs=BASIC + ("u32-wrap-inside-a-burst",)),
    dict(id="px4-64-K7-seq253", cfg="px4-64", K=7, B=8, seed=4, first_seq=253, needs=BASIC + ("sequence-255-to-0",)),
    dict(id="px4-64-K5-rate0", cfg="px4-64", K=5, seed=5, rate=0, needs=("rate0", "first-frame-then-more", "count0")),
    dict(id="px4-64-K3-no-subpixel-stride", cfg="px4-64", K=3, B=10, seed=6, overrides=dict(subpixel=0), frame_stride=64 * 64 + 48,
         pad=96, needs=BASIC),
    dict(id="px4-64-K5-mean-subtract", cfg="px4-64", K=5, seed=7, overrides=dict(mean_subtract=1), needs=BASIC),
    dict(id="opencv-128-K5", cfg="opencv-128", K=5, seed=8, needs=BASIC),
    dict(id="opencv-128-K16-no-gyro", cfg="opencv-128", K=16, B=3, S=12, seed=9, use_gyro=False, needs=BASIC),
    dict(id="opencv-128-K3-plain-levels", cfg="opencv-128", K=3, B=10, S=12, seed=10, overrides=dict(subpixel=0, mean_subtract=0),
         needs=BASIC),
    dict(id="px4-64-K5-composed", cfg="px4-64", K=5, seed=11, path=2, needs=BASIC),
    dict(id="dense-192x160-K4", cfg="dense-192x160", K=4, S=12, seed=12, needs=BASIC),
    dict(id="camera-px4-64-K5", cfg="px4-64", camera=True, K=5, seed=21, needs=BASIC + GATE + ("zero-quality-frame-skipped",)),
    dict(id="camera-px4-64-K1", cfg="px4-64", camera=True, K=1, B=24, seed=22, needs=("count0", "held")),
    dict(id="camera-px4-64-K16-wrap", cfg="px4-64", camera=True, K=16, B=3, seed=23, wrap=True,
         needs=BASIC + GATE + ("u32-wrap-inside-a-burst",)),
    dict(id="camera-odd-origin-K7", cfg="px4-64", camera=True, sensor=(322, 242), skew=2, K=7, B=6, seed=24, pad=37,
         camera_stride=322 * 242 + 5, needs=BASIC + GATE + ("crop-origin-on-an-odd-byte",)),
    dict(id="camera-no-exposure-K5", cfg="px4-64", camera=True, K=5, seed=25, exposure=False, needs=BASIC + ("no-exposure-records",)),
    dict(id="camera-no-subpixel-no-derotate-K3", cfg="px4-64", camera=True, K=3, B=10, seed=26, overrides=dict(subpixel=0),
         derotate=False, interval=50_000, needs=BASIC + GATE),
    dict(id="camera-opencv-128-K5", cfg="opencv-128", camera=True, K=5, S=12, seed=27, needs=BASIC + GATE),
    dict(id="camera-opencv-128-K16-rate0", cfg="opencv-128", camera=True, K=16, B=2, S=8, seed=28, rate=0, interval=50_000,
         needs=("rate0", "first-frame-then-more") + GATE),
    dict(id="camera-opencv-128-K3-plain-levels", cfg="opencv-128", camera=True, K=3, B=8, S=8, seed=29,
         overrides=dict(subpixel=0, mean_subtract=0), needs=BASIC),
    dict(id="camera-px4-64-K5-composed", cfg="px4-64", camera=True, K=5, seed=30, path=2, needs=BASIC + GATE),
    dict(id="camera-tile16-K4", cfg="tile16-160x128", camera=True, K=4, S=12, seed=31, interval=50_000, needs=BASIC + GATE),
]

EVERY_SITUATION = set(BASIC + GATE + ("zero-quality-frame-skipped", "u32-wrap-inside-a-burst", "sequence-255-to-0", "rate0",
                                      "no-exposure-records", "crop-origin-on-an-odd-byte"))


def test_the_cases_ask_for_every_situation_the_issue_lists():
    assert set().union(*(c["needs"] for c in CASES)) == EVERY_SITUATION
    ks = {c["K"] for c in CASES}
    assert 1 in ks and 16 in ks and any(k % 2 == 1 and k > 1 for k in ks)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_a_burst_equals_k_single_ticks_on_a_twin_bank_and_the_oracle_chain(aof, orc, synth, gpu_device, case):
    """After every burst of a run of several: every output against K single ticks on a twin bank and against the oracle
    chain per stream, and the bank's frames and state regions against the twin's."""
    c = Case(aof, orc, synth, **{k: v for k, v in case.items() if k != "id"})      # (asserts the census)
    eng, eng_t = c.engine(), c.engine()
    dev, twin = c.burst_device(eng, gpu_device), c.tick_device(eng_t, gpu_device)
    for j in range(c.B):
        got = dev.push(j, c.given, c.sensors(j))
        c.check_against_oracle(j, got, orc)
        c.check_against_ticks(j, got, twin)
        assert dev.bank.frames_bytes().tobytes() == twin.bank.frames_bytes().tobytes(), ("frames region", j)
        assert dev.bank.state_bytes().tobytes() == twin.bank.state_bytes().tobytes(), ("state region", j)
        if c.camera:
            assert dev.gate_bytes().tolist() == c.after[(j + 1) * c.K - 1].tolist(), ("gate", j)
    eng.close(), eng_t.close()


def test_a_null_count_means_every_round(aof, orc, synth, gpu_device):
    """d_count == NULL: all K rounds of every stream, against K ticks with d_active == NULL on a twin bank."""
    p = params_of(aof, "px4-64")
    S, K, B = 16, 5, 3
    run = ref.make_run(synth, 64, 64, S, K * B, 41, black=False)
    run.active[:] = 1
    for s in range(S):                                   # (make_run's idle entries hold noise: give every tick a frame)
        run.frames[:, s] = synth.make_sequence(64, 64, K * B, 4, seed=4100 + s, max_step=3)[0]
        run.times[:, s] = 11000 * (np.arange(K * B) + 1) + 7 * s
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    eng, eng_t = aof.FlowEngine(p, 0), aof.FlowEngine(p, 0)
    dev, twin = BankRig(aof, eng, run, bp, gpu_device, K=K), BankRig(aof, eng_t, run, bp, gpu_device)
    full = np.full((B, S), K, np.uint8)
    for j in range(B):
        dev.load(j, full)
        dev.enqueue(all_rounds=True)
        for k, (recs, sent, _, _) in enumerate(dev.read()):
            twin.load(j * K + k)
            twin.enqueue(all_rounds=True)
            tick = twin.read()
            assert recs.tobytes() == tick.recs.tobytes() and sent == tick.wire, (j, k)
        assert dev.bank_bytes() == twin.bank_bytes(), j
    eng.close(), eng_t.close()


@pytest.mark.parametrize("camera,cfg,K,seed", [(False, "px4-64", 5, 51), (False, "opencv-128", 16, 52), (True, "px4-64", 7, 53),
                                               (True, "opencv-128", 5, 54)])
def test_both_paths_leave_identical_bytes_after_every_burst(aof, orc, synth, gpu_device, camera, cfg, K, seed):
    """aof_set_bank_path 1 and 2 over the same run: every output and the bank's frames and state regions identical
    after every burst; path 0 equals them."""
    c = Case(aof, orc, synth, cfg, K, S=16, B=4, seed=seed, camera=camera, needs=BASIC)
    engs = [c.engine(path) for path in (1, 2, 0)]
    devs = [c.burst_device(e, gpu_device) for e in engs]
    for j in range(c.B):
        sensors = c.sensors(j)
        outs = []
        for d in devs:
            d.load(j, c.given, sensors)
            d.enqueue()
            outs.append((d.raw(), d.bank_bytes()))
        assert outs[0][0] == outs[1][0], ("outputs, path 1 against path 2", j)
        assert outs[0][1] == outs[1][1], ("bank bytes, path 1 against path 2", j)
        assert outs[2] == outs[0], ("path 0", j)
    for e in engs:
        e.close()


@pytest.mark.parametrize("camera", [False, True])
def test_a_masked_reset_between_bursts(aof, orc, synth, gpu_device, camera):
    """A masked reset between two bursts: the reset streams are new to the next burst -- a first frame, sequence number
    first_seq, the gate open --, the others go on as if nothing had happened.  Against the oracle chain with fresh
    objects for the reset streams, on both paths."""
    import torch
    S, K, B, at = 24, 5, 6, 3
    mask = (np.arange(S) % 3 == 1).astype(np.uint8)
    c = Case(aof, orc, synth, "px4-64", K, S=S, B=B, seed=61, camera=camera, first_seq=9, resets={at: mask}, needs=BASIC)
    plain = Case(aof, orc, synth, "px4-64", K, S=S, B=B, seed=61, camera=camera, first_seq=9)
    assert c.want.tobytes() != plain.want.tobytes(), "the reset changes what the chain expects"
    for path in (1, 2):
        eng = c.engine(path)
        dev = c.burst_device(eng, gpu_device)
        for j in range(B):
            if j == at:
                before = dev.bank.state_bytes()
                eng.bank_reset(dev.bank, torch.from_numpy(mask).to(gpu_device))
                after = dev.bank.state_bytes()
                assert not after[mask == 1].any() and after[mask == 0].tobytes() == before[mask == 0].tobytes()
            got = dev.push(j, c.given, c.sensors(j))
            c.check_against_oracle(j, got, orc)
            if camera:
                assert dev.gate_bytes().tolist() == c.after[(j + 1) * K - 1].tolist(), (path, j)
        first_after = [(int(np.flatnonzero(c.run.active[at * K:, s])[0]) + at * K, s) for s in np.flatnonzero(mask)]
        assert all(c.want[t, s]["frame"] == 1 for t, s in first_after)
        eng.close()


@pytest.mark.parametrize("camera,path", [(False, 1), (False, 2), (True, 1), (True, 2)])
def test_a_captured_burst_replays_on_new_inputs(aof, orc, synth, gpu_device, camera, path):
    """One burst captured with torch.cuda.graph (a linear graph: one stream) and replayed for every burst of a run with
    new frames, times and counts copied into the same input tensors equals the eager run."""
    import torch
    c = Case(aof, orc, synth, "opencv-128", 5, S=12, B=5, seed=71, camera=camera, needs=BASIC)
    eng = c.engine(path)
    eager = c.burst_device(eng, gpu_device)
    outs = []
    for j in range(c.B):
        eager.load(j, c.given, c.sensors(j))
        eager.enqueue()
        outs.append(eager.raw())
    dev = c.burst_device(eng, gpu_device)
    dev.push(0, c.given, c.sensors(0))           # (every kernel of the burst has run once before the capture)
    eng.bank_reset(dev.bank)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dev.enqueue()
    for j in range(c.B):
        dev.load(j, c.given, c.sensors(j))
        g.replay()
        assert dev.raw() == outs[j], j
    assert dev.bank_bytes() == eager.bank_bytes()
    eng.close()


def test_burst_entry_points_argument_handling(aof, synth, gpu_device):
    """What the burst entry points refuse on top of the single-tick ones, with which code, and that a refused call
    leaves the bank and the outputs untouched."""
    import torch
    p = params_of(aof, "px4-64")
    S, K, cw, ch = 8, 4, 320, 240
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    cam = aof.bank_camera_params(cw, ch, 64, 64, 0, 200_000, cref.DEROTATE, FX, FY)
    L, staging = aof.bank_camera_layout(p, bp, cam)
    assert staging == aof.bank_layout(p, bp).total_bytes
    buf = torch.zeros(L.total_bytes + 256, dtype=torch.uint8, device=gpu_device)
    sensor = torch.randint(0, 256, (K, S, ch, cw), dtype=torch.uint8, device=gpu_device)
    frames = sensor[:, :, 88:152, 128:192].contiguous()
    times = (torch.arange(K * S, dtype=torch.int64, device=gpu_device).view(K, S) // S) * 12000 + 70000
    outs = dict(recs=torch.zeros((K, S, 48), dtype=torch.uint8, device=gpu_device),
                expo=torch.zeros(K * S * 48 + 4, dtype=torch.uint8, device=gpu_device),
                derot=torch.zeros(K * S * 8 + 4, dtype=torch.uint8, device=gpu_device),
                wire=torch.zeros((K, S, 56), dtype=torch.uint8, device=gpu_device),
                lens=torch.zeros((K, S), dtype=torch.uint8, device=gpu_device))
    stream = torch.cuda.current_stream().cuda_stream
    plain, camera, reset = aof.lib.aof_bank_push_burst_device, aof.lib.aof_bank_push_camera_burst_device, aof.lib.aof_bank_reset_device
    burst = aof.bank_burst_params(K)

    def pargs(**kw):
        b, u = kw.get("bp", bp), kw.get("burst", burst)
        return [kw.get("ctx", eng._ctx), C.byref(b) if b is not None else None, C.byref(u) if u is not None else None,
                kw.get("frames", frames.data_ptr()), kw.get("times", times.data_ptr()), None, None, kw.get("bank", buf.data_ptr()),
                kw.get("bytes", L.total_bytes), kw.get("recs", outs["recs"].data_ptr()), kw.get("wire", outs["wire"].data_ptr()),
                kw.get("lens", outs["lens"].data_ptr()), stream]

    def cargs(**kw):
        b, u, c = kw.get("bp", bp), kw.get("burst", burst), kw.get("cam", cam)
        return [kw.get("ctx", eng._ctx), C.byref(b) if b is not None else None, C.byref(c) if c is not None else None,
                C.byref(u) if u is not None else None, kw.get("sensor", sensor.data_ptr()), kw.get("times", times.data_ptr()), None, None,
                kw.get("bank", buf.data_ptr()), kw.get("bytes", L.total_bytes), kw.get("recs", outs["recs"].data_ptr()),
                kw.get("expo", outs["expo"].data_ptr()), kw.get("derot", outs["derot"].data_ptr()),
                kw.get("wire", outs["wire"].data_ptr()), kw.get("lens", outs["lens"].data_ptr()), stream]

    assert reset(eng._ctx, C.byref(bp), None, buf.data_ptr(), L.total_bytes, stream) == 0
    assert camera(*cargs()) == 0
    torch.cuda.synchronize()
    r = aof.ticks_view(outs["recs"][K - 1])
    assert (r["frame"] == K).all()
    for t in outs.values():
        t.fill_(0xEE)
    snapshot = buf.clone()
    bad = lambda **kw: aof.bank_params(**{**dict(n_streams=S, focal_x=FX, focal_y=FY, output_rate=15, offset_timestamp_usec=OFFSET), **kw})
    bcam = lambda *a, **kw: aof.bank_camera_params(*a, **{**dict(derotate=cref.DEROTATE, focal_x=FX, focal_y=FY), **kw})
    B = aof.bank_burst_params
    common = [
        (dict(ctx=None), EINVAL), (dict(bp=None), EINVAL), (dict(burst=None), EINVAL), (dict(bank=None), EINVAL),
        (dict(times=None), EINVAL), (dict(recs=None), EINVAL), (dict(lens=None), EINVAL),
        (dict(burst=B(0)), EINVAL), (dict(burst=B(17)), EINVAL), (dict(burst=B(-1)), EINVAL),
        (dict(bp=bad(n_streams=0)), EINVAL), (dict(bp=bad(frame_stride=4096 + 8)), EINVAL), (dict(bp=bad(focal_x=0.0)), EINVAL),
        (dict(bank=buf.data_ptr() + 16), EINVAL),
    ]
    plain_only = [
        (dict(frames=None), EINVAL),
        (dict(burst=B(K, S * 4096 - 16)), EINVAL),        # below one round
        (dict(burst=B(K, S * 4096 + 8)), EINVAL),         # not a multiple of 16
        (dict(burst=B(K, -S * 4096)), EINVAL),
        (dict(bytes=staging - 1), ENOSPC),                # (staging == aof_bank_layout().total_bytes)
        (dict(bp=bad(n_streams=S + 1), bytes=staging), ENOSPC),
    ]
    camera_only = [
        (dict(sensor=None), EINVAL), (dict(cam=None), EINVAL), (dict(derot=None), EINVAL),
        (dict(expo=outs["expo"].data_ptr() + 2), EINVAL), (dict(derot=outs["derot"].data_ptr() + 2), EINVAL),
        (dict(cam=bcam(cw, ch, 64, 48)), EINVAL), (dict(cam=bcam(64, 48, 64, 64)), EINVAL),
        (dict(cam=bcam(cw, ch, 64, 64, camera_stride=cw * ch - 1)), EINVAL),
        (dict(burst=B(K, S * cw * ch - 1)), EINVAL),      # below one round of sensor frames
        (dict(bytes=L.total_bytes - 1), ENOSPC), (dict(bp=bad(n_streams=S + 1)), ENOSPC),
        (dict(bytes=staging), ENOSPC),                    # a bank sized by aof_bank_layout
    ]
    for kw, code in common + plain_only:
        assert plain(*pargs(**kw)) == code, ("plain", kw)
    for kw, code in common + camera_only:
        assert camera(*cargs(**kw)) == code, ("camera", kw)
    torch.cuda.synchronize()
    assert torch.equal(buf, snapshot), "a refused call must leave the bank untouched"
    assert all(untouched(t.cpu().numpy()) for t in outs.values()), "a refused call must leave the outputs untouched"
    assert b"bank" in aof.lib.aof_last_error(eng._ctx)
    # the context is still usable: a padded round_stride for the camera form needs no alignment, and a bank sized by the
    # camera layout serves the plain burst; NULL d_count / d_gyro / d_mavlink / d_exposure are fine
    times += 80000
    assert plain(*pargs(wire=None, lens=None)) == 0
    torch.cuda.synchronize()
    assert (aof.ticks_view(outs["recs"][K - 1])["frame"] == 2 * K).all()
    off = aof.bank_camera_params(cw, ch, 64, 64, 0, 200_000, None, FX, FY)
    times += 80000
    assert camera(*cargs(cam=off, expo=None, derot=None, wire=None, lens=None)) == 0
    torch.cuda.synchronize()
    assert (aof.ticks_view(outs["recs"][0])["frame"] == 2 * K + 1).all()
    assert untouched(outs["expo"].cpu().numpy()) and untouched(outs["derot"].cpu().numpy())
    eng.close()


def test_a_faulted_context_launches_no_burst(aof, synth, gpu_device):
    """The context's sticky device-side condition (a finaliser deadline, as tests/test_gpu_parity.py raises it): the
    burst entry points return -EIO like the single-tick ones, before their first launch -- the bank keeps its bytes."""
    import torch
    p = aof.default_params(640, 480)
    hp, hc, _ = synth.make_batch(640, 480, 8, 4, 4300)
    idx = np.arange(256) % 8
    eng = aof.FlowEngine(p, 0)
    S, K = 2, 3
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    cam = aof.bank_camera_params(640, 480, 640, 480, 0, 200_000, None, FX, FY)
    bank = eng.bank_create(bp, gpu_device, camera=cam)
    eng.set_search_mode(aof.SEARCH_EXHAUSTIVE)
    eng.set_reduce_fusion(True)
    eng.debug_vote_deadline_ticks(0)
    eng.flow_batch(torch.from_numpy(hp[idx]).to(gpu_device), torch.from_numpy(hc[idx]).to(gpu_device))
    torch.cuda.synchronize()
    bank.buffer.fill_(0xC3)
    frames = torch.full((K, S, 480, 640), 0x5A, dtype=torch.uint8, device=gpu_device)
    times = torch.arange(K * S, dtype=torch.int64, device=gpu_device).view(K, S) * 40000
    codes = []
    for call in (lambda: eng.bank_push(bank, frames[0], times[0]), lambda: eng.bank_push_camera(bank, frames[0], times[0]),
                 lambda: eng.bank_push_burst(bank, K, frames, times), lambda: eng.bank_push_camera_burst(bank, K, frames, times)):
        with pytest.raises(aof.AofError) as e:
            call()
        codes.append(e.value.code)
        assert "deadline" in str(e.value)
    assert codes == [EIO] * 4
    torch.cuda.synchronize()
    assert bool((bank.buffer == 0xC3).all()), "the faulted context must not have launched anything into the bank"
    eng.close()
