"""The stream bank on raw sensor frames (aof_bank_push_camera_device, include/aof.h): one call per tick takes S sensor
frames and leaves what mainloop.cpp:295-373 produces per camera -- against the CPU oracle's chain per stream (crop and
masked histogram: orc.ingest, MSV: orc.exposure_msv, calcFlow chain: tests/bank_ref.py, gyro compensation: orc.derotate,
the exposure gate restated in integers), against the two calls it replaces (aof_ingest_batch_device + aof_bank_push_device),
against the sequence pipeline, on both of its paths, from a captured graph, and through its argument checks.  Every
comparison is on raw bytes; every output buffer is pre-filled with 0xEE.  Inputs: tests/bank_camera_ref.py; the rig:
tests/bank_rig.py."""
import ctypes as C

import numpy as np
import pytest

import bank_camera_ref as cref
import bank_ref as ref
from bank_cases import run_camera_case
from bank_ref import FX, FY
from bank_rig import EINVAL, ENOSPC, GATED, LIMITED, OFFSET, SENSOR, BankRig, params_of, same_exposure, same_records, untouched
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

CASES = [
    dict(id="px4-64-from-320x240", cfg="px4-64", S=24, T=48, seed=1, census=LIMITED, gated=GATED),
    dict(id="opencv-128-from-640x480", cfg="opencv-128", S=12, T=48, seed=2, census=LIMITED, gated=GATED),
    dict(id="odd-origin-322x242", cfg="px4-64", sensor=(322, 242), S=24, T=48, seed=3, census=LIMITED, gated=GATED, skew=1),
    dict(id="strides", cfg="px4-64", S=24, T=48, seed=4, census=LIMITED, gated=GATED, camera_stride=320 * 240 + 37,
         frame_stride=64 * 64 + 48, skew=3),
    dict(id="crop-is-the-sensor-frame", cfg="px4-64", sensor=(64, 64), S=24, T=48, seed=5, census=LIMITED, gated=GATED),
    dict(id="S1", cfg="px4-64", S=1, T=48, seed=6, census=LIMITED, gated=GATED),
    dict(id="S300-path1", cfg="px4-64", S=300, T=8, seed=7, path=1, interval=50_000),
    dict(id="S300-path2", cfg="px4-64", S=300, T=8, seed=7, path=2, interval=50_000),
    dict(id="interval0", cfg="px4-64", S=24, T=48, seed=8, census=LIMITED, interval=0),
    dict(id="interval50000", cfg="opencv-128", S=12, T=48, seed=9, census=LIMITED, interval=50_000),
    dict(id="no-exposure", cfg="px4-64", S=24, T=48, seed=10, census=LIMITED, exposure=False),
    dict(id="no-derotate", cfg="px4-64", S=24, T=48, seed=11, census=LIMITED, gated=GATED, derotate=False),
    dict(id="no-gyro", cfg="opencv-128", S=12, T=48, seed=12, census=LIMITED, gated=GATED, use_gyro=False),
    dict(id="wrap", cfg="px4-64", S=24, T=48, seed=13, census=LIMITED, gated=GATED, wrap=True),
    dict(id="composed-path2-px4-64", cfg="px4-64", S=24, T=48, seed=14, census=LIMITED, gated=GATED, path=2),
    dict(id="dense-192x160-composed", cfg="dense-192x160", S=12, T=48, seed=15, census=LIMITED, gated=GATED),
    dict(id="tile16-160x128-composed", cfg="tile16-160x128", S=12, T=48, seed=16, census=LIMITED, gated=GATED, path=1),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_camera_bank_equals_the_oracle_chain_per_stream_and_tick(aof, orc, synth, gpu_device, case):
    kw = {k: v for k, v in case.items() if k != "id"}
    want, due = run_camera_case(aof, orc, synth, gpu_device, **kw)
    if case["id"].startswith("S300"):
        # 8 ticks: over all streams some frame was gated and some beyond a first frame was due
        assert ((want["quality"] != ref.TICK_IDLE) & (due == 0)).any() and (due[want["frame"] > 1] == 1).any()
    if case["id"] == "interval0":
        assert (due == (want["quality"] != ref.TICK_IDLE)).all()


@pytest.mark.parametrize("cfg,seed,S", [("px4-64", 21, 24), ("opencv-128", 22, 12)])
def test_camera_push_equals_ingest_batch_followed_by_the_plain_push(aof, synth, gpu_device, cfg, seed, S):
    """The calls it replaces, on a second bank over the same run: records, wire frames, the frames region and the state
    bytes equal after every tick -- except next_exposure_us, which the plain push passes through (0) and which is
    compared against the restated gate."""
    import torch
    p = params_of(aof, cfg)
    T, sensor = 48, SENSOR[cfg]
    run = cref.add_saturated_patches(ref.make_run(synth, p.width, p.height, S, T, seed))
    cam_run = cref.CameraRun(run, sensor[0], sensor[1], seed)
    due, after = cref.gate(run.times, run.active, cref.EXPOSURE_INTERVAL_US)
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 3)
    cam = aof.bank_camera_params(sensor[0], sensor[1], p.width, p.height, 0, cref.EXPOSURE_INTERVAL_US, cref.DEROTATE, FX, FY)
    eng_a, eng_b = aof.FlowEngine(p, 0), aof.FlowEngine(p, 0)
    dev = BankRig(aof, eng_a, run, bp, gpu_device, camera=(cam, cam_run))
    plain = eng_b.bank_create(bp, gpu_device)
    frames = torch.zeros((S, p.height, p.width), dtype=torch.uint8, device=gpu_device)
    recs = torch.zeros((S, 48), dtype=torch.uint8, device=gpu_device)
    wire = torch.zeros((S, 56), dtype=torch.uint8, device=gpu_device)
    lens = torch.zeros(S, dtype=torch.uint8, device=gpu_device)
    hist = torch.zeros((S, 10), dtype=torch.int32, device=gpu_device)
    held = 0
    for k in range(T):
        got = dev.push(k)
        recs.fill_(0xEE), wire.zero_(), lens.fill_(0xEE)
        aof.ingest_batch(dev.frames.view(S, sensor[1], sensor[0]), p.width, p.height, cropped=frames, hist=hist)
        eng_b.bank_push(plain, frames, dev.times, dev.select, dev.gyro, mavlink=True, records=recs, out_frames=wire, out_lengths=lens)
        torch.cuda.synchronize()
        assert got.recs.tobytes() == aof.ticks_view(recs).tobytes(), k
        w, n = wire.cpu().numpy(), lens.cpu().numpy()
        assert got.wire == [bytes(w[s, :n[s]]) for s in range(S)], k
        assert dev.bank.frames_bytes().tobytes() == plain.frames_bytes().tobytes(), k
        sa, sb = dev.bank.state_bytes(), plain.state_bytes()
        assert sa[:, :56].tobytes() == sb[:, :56].tobytes(), k
        assert not sb[:, 56:].any() and dev.gate_bytes().tolist() == after[k].tolist(), k
        # the due frames' histograms are the ingest kernel's
        h = hist.cpu().numpy().view(np.uint32)
        for s in np.flatnonzero(due[k]):
            assert got.exposure[s]["hist"].tolist() == h[s].tolist(), (k, s)
        assert (got.exposure["due"] == due[k]).all(), k
        held += int((got.recs["quality"] == aof.TICK_HELD).sum())
    assert held > 10 * S
    eng_a.close(), eng_b.close()


@pytest.mark.parametrize("cfg,seed,S", [("px4-64", 31, 40), ("opencv-128", 32, 16)])
def test_both_camera_paths_leave_identical_bytes_after_every_tick(aof, synth, gpu_device, cfg, seed, S):
    """aof_set_bank_path(1) and (2) over the same run: every output and the bank's frames and state regions (padding
    included) byte-identical after every tick.  The flow engine's workspace behind them is not compared: the composed
    path computes and ignores the flows of idle and first-frame streams (include/aof.h), the one-launch kernel never
    starts them, so block records of such streams legitimately differ there; the tick's pixel records of all other
    streams are compared through d_records."""
    p = params_of(aof, cfg)
    T, sensor = 48, SENSOR[cfg]
    run = cref.add_saturated_patches(ref.make_run(synth, p.width, p.height, S, T, seed))
    cam_run = cref.CameraRun(run, sensor[0], sensor[1], seed)
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 3)
    cam = aof.bank_camera_params(sensor[0], sensor[1], p.width, p.height, 0, cref.EXPOSURE_INTERVAL_US, cref.DEROTATE, FX, FY)
    engs, devs = [], []
    for path in (1, 2):
        eng = aof.FlowEngine(p, 0)
        eng.set_bank_path(path)
        engs.append(eng)
        devs.append(BankRig(aof, eng, run, bp, gpu_device, camera=(cam, cam_run)))
    held = published = n_due = n_gated = 0
    for k in range(T):
        frames_img = cam_run.sensor(k)
        a, b = devs[0].push(k, sensors=frames_img), devs[1].push(k, sensors=frames_img)
        assert a.recs.tobytes() == b.recs.tobytes(), k
        assert a.wire == b.wire, k
        assert a.exposure.tobytes() == b.exposure.tobytes(), k
        assert a.derotated.tobytes() == b.derotated.tobytes(), k
        L = devs[0].bank.layout
        ba, bb = devs[0].bank.buffer[:L.scratch].cpu().numpy(), devs[1].bank.buffer[:L.scratch].cpu().numpy()
        assert ba.tobytes() == bb.tobytes(), k
        held += int((a.recs["quality"] == aof.TICK_HELD).sum())
        published += int(((a.recs["quality"] >= 0) & (a.recs["frame"] > 1)).sum())
        n_due += int(a.exposure["due"].sum())
        n_gated += int(((a.recs["quality"] != aof.TICK_IDLE) & (a.exposure["due"] == 0)).sum())
    assert held > 10 * S and published > 3 * S and n_due >= 2 * S and n_gated > 10 * S
    for e in engs:
        e.close()


def test_one_stream_through_the_bank_equals_the_sequence_pipeline(aof, synth, gpu_device):
    """40 sensor frames fed one per tick through a bank of one stream (statistics with every frame, de-rotation on) and
    the same recording through aof_sequence_device: published records field for field, message frames, every frame's
    histogram and every pair's de-rotated floats."""
    import torch
    n, cam_w, cam_h, w, h = 40, 160, 120, 64, 64
    p = aof.px4flow_params(w, h)
    rng = np.random.default_rng(41)
    times = np.cumsum(np.concatenate([[0], rng.integers(9000, 18000, n - 1)])).astype(np.int64)
    frames, _ = synth.make_sequence(cam_w, cam_h, n, 4, seed=41, max_step=3)
    gyro = np.zeros((n, 4), np.float32)
    gyro[:, :3] = rng.normal(0, 0.004, (n, 3)).astype(np.float32)
    gyro[:, 3] = np.float32(0.013)
    eng = aof.FlowEngine(p, 0)
    sp = aof.sequence_params(cam_w, cam_h, w, h, FX, FY, 15, OFFSET, 1, 100, 0, derotate=cref.DEROTATE)
    ws, L = eng.sequence(sp, torch.from_numpy(frames).to(gpu_device), torch.from_numpy(times).to(gpu_device),
                         torch.from_numpy(gyro).to(gpu_device))
    torch.cuda.synchronize()
    out = eng.sequence_outputs(sp, ws, L, n)
    assert len(out["records"]) >= 4 and (out["derotated"] != np.stack([out["flows"]["flow_x"], out["flows"]["flow_y"]], -1)).any()

    run = ref.Run(np.zeros((n, 1, h, w), np.uint8), times.reshape(n, 1), gyro.reshape(n, 1, 4), np.ones((n, 1), np.uint8))
    cam_run = cref.CameraRun(run, cam_w, cam_h, 41)
    bp = aof.bank_params(1, FX, FY, 15, OFFSET, 1, 100, 0)
    cam = aof.bank_camera_params(cam_w, cam_h, w, h, 0, 0, cref.DEROTATE, FX, FY)
    for path in (1, 2):
        eng.set_bank_path(path)
        dev = BankRig(aof, eng, run, bp, gpu_device, camera=(cam, cam_run))
        m = 0
        for k in range(n):
            got = dev.push(k, sensors=frames[k:k + 1])
            r, e = got.recs[0], got.exposure[0]
            assert e["due"] == 1 and e["hist"].tolist() == out["exposure"][k].tolist(), (path, k)
            if k == 0:
                assert not got.derotated.any()
            else:
                assert got.derotated[0].tobytes() == out["derotated"][k - 1].tobytes(), (path, k)
                assert r["pixel"].tobytes() == out["flows"][k - 1].tobytes(), (path, k)
            if r["quality"] >= 0:
                q = out["records"][m]
                assert q["frame"] == r["frame"] - 1 == k, (path, k)
                for name in ("quality", "dt_us", "flow_x", "flow_y", "gyro_x", "gyro_y", "gyro_z"):
                    assert q[name].tobytes() == r[name].tobytes(), (path, k, name)
                assert got.wire[0] == out["mavlink"][m] and len(got.wire[0]) > 0, (path, k)
                m += 1
        assert m == len(out["records"])
    eng.close()


@pytest.mark.parametrize("path", [1, 2])
def test_a_captured_camera_tick_replays_on_new_inputs(aof, synth, gpu_device, path):
    """One camera tick captured with torch.cuda.graph (a linear graph) and replayed for 20 ticks with new sensor frames,
    times and masks copied into the same input tensors equals the eager run."""
    import torch
    p = params_of(aof, "opencv-128")
    S, T, sensor = 16, 20, SENSOR["opencv-128"]
    run = cref.add_saturated_patches(ref.make_run(synth, 128, 128, S, T, 51))
    cam_run = cref.CameraRun(run, sensor[0], sensor[1], 51)
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    cam = aof.bank_camera_params(sensor[0], sensor[1], 128, 128, 0, 50_000, cref.DEROTATE, FX, FY)
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    eager = BankRig(aof, eng, run, bp, gpu_device, camera=(cam, cam_run))
    outs = [eager.push(k) for k in range(T)]
    dev = BankRig(aof, eng, run, bp, gpu_device, camera=(cam, cam_run))
    dev.push(0)                                  # (every kernel of the tick has run once before the capture)
    eng.bank_reset(dev.bank)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dev.enqueue()
    for k in range(T):
        dev.load(k)
        g.replay()
        got = dev.read()
        assert got.recs.tobytes() == outs[k].recs.tobytes(), k
        assert got.wire == outs[k].wire, k
        assert got.exposure.tobytes() == outs[k].exposure.tobytes(), k
        assert got.derotated.tobytes() == outs[k].derotated.tobytes(), k
    assert dev.bank.frames_bytes().tobytes() == eager.bank.frames_bytes().tobytes()
    assert dev.bank.state_bytes().tobytes() == eager.bank.state_bytes().tobytes()
    d = np.stack([o.exposure["due"] for o in outs])
    q = np.stack([o.recs["quality"] for o in outs])
    assert (d[4:] == 1).any() and ((d == 0) & (q != aof.TICK_IDLE)).any() and (q == aof.TICK_HELD).any() and (q[4:] >= 0).any()
    eng.close()


def test_camera_entry_point_argument_handling(aof, synth, gpu_device):
    """What aof_bank_push_camera_device refuses, with which code, and that a refused call leaves bank and outputs
    untouched."""
    import torch
    p = params_of(aof, "px4-64")
    S, cw, ch = 8, 320, 240
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    cam = aof.bank_camera_params(cw, ch, 64, 64, 0, 200_000, cref.DEROTATE, FX, FY)
    L, staging = aof.bank_camera_layout(p, bp, cam)
    assert L.total_bytes > aof.bank_layout(p, bp).total_bytes == staging
    buf = torch.zeros(L.total_bytes + 256, dtype=torch.uint8, device=gpu_device)
    sensor = torch.from_numpy(synth.make_sequence(cw, ch, S, 4, seed=61, max_step=3)[0]).to(gpu_device)
    times = torch.arange(S, dtype=torch.int64, device=gpu_device) * 1000 + 70000
    outs = dict(recs=torch.zeros((S, 48), dtype=torch.uint8, device=gpu_device),
                expo=torch.zeros(S * 48 + 4, dtype=torch.uint8, device=gpu_device),     # (room for a misaligned pointer)
                derot=torch.zeros(S * 8 + 4, dtype=torch.uint8, device=gpu_device),
                wire=torch.zeros((S, 56), dtype=torch.uint8, device=gpu_device),
                lens=torch.zeros(S, dtype=torch.uint8, device=gpu_device))
    stream = torch.cuda.current_stream().cuda_stream
    push, reset = aof.lib.aof_bank_push_camera_device, aof.lib.aof_bank_reset_device

    def args(**kw):
        b, c = kw.get("bp", bp), kw.get("cam", cam)
        return [kw.get("ctx", eng._ctx), C.byref(b) if b is not None else None, C.byref(c) if c is not None else None,
                kw.get("sensor", sensor.data_ptr()), kw.get("times", times.data_ptr()), None, None,
                kw.get("bank", buf.data_ptr()), kw.get("bytes", L.total_bytes), kw.get("recs", outs["recs"].data_ptr()),
                kw.get("expo", outs["expo"].data_ptr()), kw.get("derot", outs["derot"].data_ptr()),
                kw.get("wire", outs["wire"].data_ptr()), kw.get("lens", outs["lens"].data_ptr()), stream]

    assert reset(eng._ctx, C.byref(bp), None, buf.data_ptr(), L.total_bytes, stream) == 0
    assert push(*args()) == 0                                             # every stream's first frame
    torch.cuda.synchronize()
    e = aof.exposure_view(outs["expo"][:S * 48].view(S, 48))
    assert (e["due"] == 1).all() and (e["hist"].sum(1) == 4096).all()
    for t in outs.values():
        t.fill_(0xEE)
    snapshot = buf.clone()
    bad = lambda **kw: aof.bank_params(**{**dict(n_streams=S, focal_x=FX, focal_y=FY, output_rate=15, offset_timestamp_usec=OFFSET), **kw})
    bcam = lambda *a, **kw: aof.bank_camera_params(*a, **{**dict(derotate=cref.DEROTATE, focal_x=FX, focal_y=FY), **kw})
    refused = [
        (dict(ctx=None), EINVAL), (dict(bp=None), EINVAL), (dict(cam=None), EINVAL), (dict(bank=None), EINVAL),
        (dict(sensor=None), EINVAL), (dict(times=None), EINVAL), (dict(recs=None), EINVAL),
        (dict(lens=None), EINVAL),                                                              # d_mavlink without its lengths
        (dict(derot=None), EINVAL),                                                             # derotate without d_derotated
        (dict(expo=outs["expo"].data_ptr() + 2), EINVAL), (dict(derot=outs["derot"].data_ptr() + 2), EINVAL),   # 4-byte alignment
        (dict(cam=bcam(cw, ch, 64, 48)), EINVAL), (dict(cam=bcam(cw, ch, 128, 128)), EINVAL),   # crop != the context's frame
        (dict(cam=bcam(64, 48, 64, 64)), EINVAL),                                               # crop larger than the sensor frame
        (dict(cam=bcam(cw, ch, 64, 64, camera_stride=cw * ch - 1)), EINVAL),                    # below one sensor frame
        (dict(bp=bad(n_streams=0)), EINVAL), (dict(bp=bad(frame_stride=4096 + 8)), EINVAL), (dict(bp=bad(focal_x=0.0)), EINVAL),
        (dict(bank=buf.data_ptr() + 16), EINVAL),                                               # 256-byte alignment
        (dict(bytes=L.total_bytes - 1), ENOSPC),
        (dict(bytes=staging), ENOSPC),                                                          # a bank sized by aof_bank_layout
        (dict(bp=bad(n_streams=S + 1)), ENOSPC),
    ]
    for kw, code in refused:
        assert push(*args(**kw)) == code, kw
    torch.cuda.synchronize()
    assert torch.equal(buf, snapshot), "a refused call must leave the bank untouched"
    assert all(untouched(t.cpu().numpy()) for t in outs.values()), "a refused call must leave the outputs untouched"
    assert b"bank" in aof.lib.aof_last_error(eng._ctx)
    # the context is still usable; NULL d_exposure / d_derotated (derotate off) / d_mavlink are fine, and a bank sized by
    # the camera layout serves the plain push as well
    off = aof.bank_camera_params(cw, ch, 64, 64, 0, 200_000, None, FX, FY)
    times += 80000
    assert push(*args(cam=off, expo=None, derot=None, wire=None, lens=None)) == 0
    torch.cuda.synchronize()
    r = aof.ticks_view(outs["recs"])
    assert (r["frame"] == 2).all() and (r["quality"] >= 0).all() and (r["dt_us"] == times.cpu().numpy()).all()
    assert untouched(outs["expo"].cpu().numpy()) and untouched(outs["derot"].cpu().numpy())
    frames = torch.zeros((S, 64, 64), dtype=torch.uint8, device=gpu_device)
    times += 80000
    assert aof.lib.aof_bank_push_device(eng._ctx, C.byref(bp), frames.data_ptr(), times.data_ptr(), None, None, buf.data_ptr(),
                                        L.total_bytes, outs["recs"].data_ptr(), None, None, stream) == 0
    torch.cuda.synchronize()
    assert (aof.ticks_view(outs["recs"])["frame"] == 3).all()
    eng.close()


def test_a_masked_reset_mid_run_opens_the_gate_of_the_reset_streams(aof, orc, synth, gpu_device):
    """After a masked reset the reset streams' gate is 0 again -- their next frame is due, and a first frame --, the
    others keep theirs."""
    import torch
    p = params_of(aof, "px4-64")
    S, T, at = 24, 48, 20
    run = cref.add_saturated_patches(ref.make_run(synth, 64, 64, S, T, 71))
    cam_run = cref.CameraRun(run, 320, 240, 71)
    mask = (np.arange(S) % 3 == 1).astype(np.uint8)
    new = lambda s=0: ref.oracle_chain(aof, orc, p, 15, OFFSET, 9)
    want, wire = ref.expected(run, [new() for _ in range(S)], resets={at: mask}, new_chain=new)
    due, after = cref.gate(run.times, run.active, cref.EXPOSURE_INTERVAL_US, resets={at: mask})
    plain_due, _ = cref.gate(run.times, run.active, cref.EXPOSURE_INTERVAL_US)
    assert (due != plain_due).any(), "the reset changes what is due"
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 9)
    cam = aof.bank_camera_params(320, 240, 64, 64, 0, cref.EXPOSURE_INTERVAL_US, cref.DEROTATE, FX, FY)
    for path in (1, 2):
        eng = aof.FlowEngine(p, 0)
        eng.set_bank_path(path)
        dev = BankRig(aof, eng, run, bp, gpu_device, camera=(cam, cam_run))
        for k in range(T):
            if k == at:
                before = dev.gate_bytes()
                assert before[mask == 1].all()
                eng.bank_reset(dev.bank, torch.from_numpy(mask).to(gpu_device))
                now = dev.gate_bytes()
                assert not now[mask == 1].any() and now[mask == 0].tolist() == before[mask == 0].tolist()
            frames_img = cam_run.sensor(k)
            got = dev.push(k, sensors=frames_img)
            same_records(got.recs, want[k], k, f"path {path}")
            assert got.wire == wire[k], (path, k)
            same_exposure(got.exposure, cref.expected_exposure(aof, orc, frames_img, run, k, due[k]), k, f"path {path}")
            assert dev.gate_bytes().tolist() == after[k].tolist(), (path, k)
        first_after = [int(np.flatnonzero(run.active[at:, s])[0]) + at for s in np.flatnonzero(mask)]
        assert all(want[k, s]["frame"] == 1 and due[k, s] == 1 for k, s in zip(first_after, np.flatnonzero(mask)))
        eng.close()
