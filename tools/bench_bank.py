#!/usr/bin/env python3
"""The stream bank's tick against the library's two existing ways in, one GPU, one process, legs alternated:
  T0 / T1 / T2  aof_bank_push_device, all streams active, with MAVLink frames: as the library chooses the path (0), the
                one-launch kernel (1), the composed path (2) -- the sweep kBankFusedMaxStreams (aof_bank.cpp) comes from;
  B             what the library offers today for state-keeping streams: S contexts, one aof_stream_push_host each per
                tick, in a loop on one thread (S <= 64 only);
  C             aof_flow_batch_device on the same S pairs resident in memory: flow without state, the floor of any tick
                that computes S flows.
With --camera, the tick on raw sensor frames (320x240 -> PX4 64x64, 640x480 -> 128x128 on two levels):
  K0 / K1 / K2  aof_bank_push_camera_device (statistics at 200 000 us, gyro, MAVLink frames, de-rotation on) as the library
                chooses the path, on the one-launch kernel, on the composed path (K1 / K2 from 1 024 streams on: the
                sweep kBankCameraFusedMaxStreams comes from);
  Y             what a caller had before: aof_ingest_batch_device into a tick buffer, then aof_bank_push_device;
  T0            the plain tick on pre-cropped frames.
With --burst K[,K...], K frame rounds per call against K calls of the single tick on the same frames, plain and camera
form (--forms), each on path 0 / 1 / 2:
  B0 / B1 / B2  one aof_bank_push_burst_device (aof_bank_push_camera_burst_device) of K rounds, all streams in all rounds;
  T0 / T1 / T2  K calls of aof_bank_push_device (aof_bank_push_camera_device) on round k's buffers: the same library
                and the entry point that existed before bursts -- the yardstick.
With --outbox, what it costs and gains to collect the published messages of a push into one dense list
(aof_bank_collect_device), at 15 Hz with 9-18 ms between a stream's frames and at output_rate 0 (everything publishes):
  T             the tick alone, pipelined (as T0);
  D             tick + collect into a device outbox, pipelined: D - T prices the extra launch in a stream that runs on;
  H             what a host had before: tick + three asynchronous device-to-host copies (records, lengths, frames) into
                pinned memory + stream synchronise + np.flatnonzero(quality >= 0) -- the yardstick of O;
  O             tick + collect into a HostOutbox + polling the tag.
H and O are timed per tick from the enqueue to the host holding the list; one line with bursts of K = 5 rounds.
With --exposure-control, the auto-exposure controller behind the camera push (320x240 -> PX4 64x64; K = 1: the camera
tick, K = 5: the camera burst; statistics at 200 000 us, frames 13 333 us apart):
  T             the camera push alone, pipelined;
  C             camera push + aof_bank_exposure_control_device, pipelined: C - T prices the extra launch;
  H             what a host did before: camera push + one asynchronous device-to-host copy of the exposure records into
                pinned memory + stream synchronise + aof_exposure_control_host on host states: every step ends with the
                host holding the commands.
With --mavlink-rx, the MAVLink receive in front of the IMU call (64x64 ticks; 4 HIGHRES_IMU frames per stream and tick,
alone -- mix "imu" -- and inside about 1 KB of other frames -- mix "mixed"):
  H             aof_bank_mavlink_rx_host over the S slots of a pinned receive block + one host-to-device copy of the
                samples and counts + records-only push + aof_bank_imu_device: the way without the receive call, and the
                yardstick of D;
  D             one host-to-device copy of the receive block (bytes and lengths) + aof_bank_mavlink_rx_device + the same
                push and IMU call.
With --per-stream, the plain tick with an array of per-stream records bound (aof_set_bank_streams: every stream its own
focal lengths, output rate, offset and MAVLink identity) against the tick on the scalars of aof_bank_params:
  U1 / U2       aof_bank_push_device, nothing bound, on the one-launch kernel (1) and the composed path (2) -- also what a
                build without the call runs (AOF_LIB: the yardstick of U on this build);
  P1 / P2       the same tick with S distinct records bound.
With --per-sensor, the camera tick with an array of per-stream sensor records bound (aof_set_bank_sensors: S records equal
to aof_bank_sensor_from_camera, so both legs move the same bytes and the difference is the record's load and check)
against the camera tick on the scalars of aof_bank_camera, 64x64 from 320x240 and 128x128 from 640x480:
  K1 / K2       aof_bank_push_camera_device, nothing bound, on the one-launch kernel (1) and the composed path (2) -- also
                what a build without the call runs (AOF_LIB: the yardstick of K on this build);
  S1 / S2       the same tick with the S records bound.
With --pixel-formats, the camera tick with packed 16-bit sensor pixels (aof_set_bank_pixel_formats), on both bank paths
(leg names end in the path, 1 or 2):
    G   sensors bound, no formats: grey frames (with AOF_LIB, on a build without the call: the yardstick of P0 on this build);
    P0  formats bound, all AOF_PIXEL_GREY8: the same frames, the same bytes;
    Y   all AOF_PIXEL_LUMA16_LO (YUYV): cam_w x cam_h pixels of two bytes, the crop fetched out of the packed frames;
    M   formats mixed per stream (s % 3): every stream in a slot of 2 cam_w cam_h bytes;
    D   what a caller does without the call: a device de-interleave of the whole packed buffer (one strided copy kernel,
        2 + 1 bytes moved per sensor pixel) into a grey buffer, then leg G on that.
With --binning, the camera tick with binned sensor pixels (aof_set_bank_binning), on both bank paths (leg names end in the
path, 1 or 2).  A binned stream's sensor is bin * (crop + 16) pixels a side with the footprint at its centre, every crop
pixel of the synthetic frame repeated bin x bin times, so every leg searches the same frames:
    G   sensors and formats (all grey) bound, no bins (with AOF_LIB, on a build without the call: the yardstick of B0);
    B0  bins bound, all ones: the same frames, the same bytes;
    B2 / B4   every stream binned 2x / 4x, grey sensors;
    Y4  AOF_PIXEL_LUMA16_LO sensors binned 4x;
    D2 / D4   what a caller does without the call: aof_ingest_sensors_binned_device of the B2 / B4 sensors into a dense
        grey buffer, then the camera tick on that buffer (sensors and formats bound, as G).
With --raw-formats, the camera tick with raw mono pixels (AOF_PIXEL_Y10 .. AOF_PIXEL_Y12P), on both bank paths (leg names
end in the path, 1 or 2).  Every stream's frame lies in a slot of 2 cam_w cam_h bytes, its rows row_bytes of its format apart:
    G   sensors bound, no formats: grey frames (with AOF_LIB, on a build without the formats: the yardstick of G on this build);
    R   all AOF_PIXEL_Y10: 16-bit little-endian words, the grey value in bits 2..9;
    P   all AOF_PIXEL_Y10P: four pixels in five bytes;
    M   formats mixed per stream (s % 8 over GREY8, LUMA16_LO, LUMA16_HI, Y10, Y12, Y14, Y10P, Y12P);
    D   what a caller does without the formats: a device unpack of the whole Y10 buffer (a shift of the 16-bit words and a
        narrowing copy, two launches, 2 + 2 + 2 + 1 bytes moved per sensor pixel) into a grey buffer, then leg G on that.
With --warp, the camera tick with warp meshes (aof_set_bank_warps) on 640 x 480 grey frames -- the synthetic frame at the
centre crop and repeated around it, so that a mesh reaching outside the plain crop reads moving texture:
    P   the composed camera tick (path 2), nothing bound (with AOF_LIB, on a build without the call: the yardstick of P);
    I   the same with S identity meshes bound (path 2: the composed path of a bank with meshes bound);
    L   with the mesh of a barrel lens (k1 -0.28, k2 0.07, focal length 0.9 of the crop size);
    F   the one-launch camera tick (path 1), nothing bound: what a warped bank gives up (also run under AOF_LIB);
    U   what a caller does without the binding: aof_ingest_warped_device into a grey buffer, then the camera tick on it;
    W   the barrel lens on path 1: the one-launch tick with the warp inside it (k_bank_tick_warp.hip);
    WI  identity meshes on path 1;
    WB1 / WB2   a burst of K = 5 rounds with the lens on path 1 (five launches of that kernel) and on path 2 (fifteen
        launches), us per burst; the sensor frames of the burst legs carry noise around the crop.
    W, WI, WB1 and WB2 assert through aof_bank_last_path that they timed the path they name.  The yardstick of W is leg L
    of the build before the kernel, loaded through AOF_LIB in the same session (--legs P,L,F).
With --field, the stream bank's motion field behind the plain tick (aof_bank_field_device; the records and prototypes are
tests/bank_field_rig.py's), on both bank paths (leg names end in the path, 1 or 2), S = 64 .. 4 096:
    T   the tick alone, pipelined (with AOF_LIB, on a build without the call: the yardstick of T on this build);
    F   tick + aof_bank_field_device, pipelined: F - T prices the fit and the window's step in a stream that runs on;
    H   what a host does without the call: tick + asynchronous device-to-host copies of the block records, the
        sub-directions and the tick records into pinned memory + stream synchronise + aof_bank_field_host: every step ends
        with the host holding the records.
K1 / K2 are the legs --camera runs under those names (leg_camera); --per-sensor --legs K1,K2 runs them alone, which is how
two builds of the library are compared in turn in one session.
Every leg settles for about 0.2 s of untimed ticks, then times at least --ticks ticks and at least --seconds seconds
with the host clock around ticks that end in a synchronise.  The whole sweep runs --repeats times: the difference
between the repeats is the run-to-run spread a difference between legs has to beat.
    python tools/bench_bank.py [--streams 1,16,...] [--configs px4-64,opencv-128] > profiles/bank_tick_sweep.txt
    python tools/bench_bank.py --camera > profiles/bank_camera_tick_sweep.txt
    python tools/bench_bank.py --burst 2,5,16 > profiles/bank_burst_sweep.txt
    python tools/bench_bank.py --outbox > profiles/bank_outbox_sweep.txt
    python tools/bench_bank.py --exposure-control > profiles/bank_exposure_control_sweep.txt
    python tools/bench_bank.py --imu > profiles/bank_imu_sweep.txt
    python tools/bench_bank.py --mavlink-rx > profiles/bank_mavlink_rx_sweep.txt
    python tools/bench_bank.py --per-stream --streams 64,1024 > profiles/bank_per_stream_ab.txt
    python tools/bench_bank.py --per-sensor --streams 64,1024 > profiles/bank_per_sensor_ab.txt
    python tools/bench_bank.py --binning --repeats 3 > profiles/bank_binning_ab.txt
    python tools/bench_bank.py --raw-formats --repeats 3 > profiles/bank_raw_formats_ab.txt
    python tools/bench_bank.py --warp --repeats 3 > profiles/bank_warp_ab.txt
    python tools/bench_bank.py --warp --repeats 3 --streams 64,256,1024,2048,4096 > profiles/bank_warp_one_launch_ab.txt
    python tools/bench_bank.py --field --repeats 3 > profiles/bank_field_ab.txt"""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

aof = ge.load_package()
synth = importlib.import_module(ge.PKG_NAME + ".synth")
FX, FY = 216.6677, 216.2457
RING = 8          # ticks whose frames and time stamps are resident: the timed loop cycles through them
POOL = 16         # distinct synthetic streams; stream s shows pool[s % POOL]


def params_of(name):
    if name == "px4-64":
        return aof.px4flow_params(64, 64)
    if name == "opencv-128":
        return aof.px4flow_params(128, 128, pyramid_levels=2, mean_subtract=1)
    raise SystemExit(f"unknown configuration {name}")


def tick_bytes(p):
    """Compulsory bytes per stream and tick: read the stored and the new frame, write the new one, the record and the
    MAVLink frame; and of a stateless pair (algorithmic_bytes)."""
    return 3 * p.width * p.height + 48 + 56, aof.algorithmic_bytes(p)


def timed(step, sync, min_ticks, min_seconds, settle_seconds):
    """step(i) enqueues tick i.  Returns (seconds per tick, ticks timed)."""
    i, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < settle_seconds:
        for _ in range(16):
            step(i)
            i += 1
        sync()
    done, elapsed, chunk = 0, 0.0, 256
    while done < min_ticks or elapsed < min_seconds:
        t0 = time.perf_counter()
        for _ in range(chunk):
            step(i)
            i += 1
        sync()
        elapsed += time.perf_counter() - t0
        done += chunk
    return elapsed / done, done


class Inputs:
    """RING ticks of S streams on the device: frames [RING][S, h, w], times [RING][S]."""

    def __init__(self, p, S, dev):
        w, h = p.width, p.height
        pool = np.stack([synth.make_sequence(w, h, RING + 1, 4, seed=500 + k, max_step=3)[0] for k in range(POOL)])   # [POOL, RING + 1, h, w]
        idx = np.arange(S) % POOL
        self.host = pool                                            # (the B leg pushes from host memory)
        self.frames = [torch.from_numpy(pool[:, k]).to(dev)[torch.from_numpy(idx).to(dev)].contiguous() for k in range(RING + 1)]
        # ~75 frames/s against a 15 Hz output rate: a publication every five frames (and one at the ring's wrap)
        self.times = [torch.full((S,), 13333 * (k + 1), dtype=torch.int64, device=dev) for k in range(RING + 1)]
        self.gyro = torch.full((S, 4), 0.001, dtype=torch.float32, device=dev)


def distinct_streams(S):
    """BANK_STREAM_DTYPE [S]: no two neighbours alike in focal lengths, identity and offset.  The rate is the unbound
    leg's 15 Hz in every record: streams with other rates publish in other ticks, and a tick in which any stream publishes
    pays for a frame being packed -- that would time another workload, not the array."""
    s = np.arange(S)
    recs = np.zeros(S, aof.BANK_STREAM_DTYPE)
    recs["focal_x"], recs["focal_y"] = 150.0 + (s % 97) * 1.25, 160.0 + (s % 89) * 1.5
    recs["output_rate"] = 15
    recs["system_id"], recs["component_id"], recs["first_seq"] = s % 255 + 1, 100 + s % 3, s % 256
    recs["offset_timestamp_usec"] = 5_000_000 + s
    return recs


def leg_tick(p, S, path, inp, dev, a, per_stream=False):
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000, 1, 100, 0)
    bank = eng.bank_create(bp, dev)
    if per_stream:
        eng.set_bank_streams(torch.from_numpy(distinct_streams(S).view(np.uint8).reshape(S, 32)).to(dev))
    recs = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    wire = torch.empty((S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty(S, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn, ctx, bpp = aof.lib.aof_bank_push_device, eng._ctx, C.byref(bp)
    calls = [(inp.frames[k].data_ptr(), inp.times[k].data_ptr()) for k in range(RING)]
    rest = (None, inp.gyro.data_ptr(), bank.buffer.data_ptr(), bank.buffer.numel(), recs.data_ptr(), wire.data_ptr(), lens.data_ptr(), stream)

    def step(i):
        f, t = calls[i % RING]
        rc = fn(ctx, bpp, f, t, *rest)
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
    out = timed(step, torch.cuda.synchronize, a.ticks, a.seconds, a.settle)
    r = aof.ticks_view(recs)
    assert (r["quality"] >= aof.TICK_HELD).all() and (r["frame"] > a.ticks).all(), "the timed ticks were real ticks"
    eng.close()
    return out


SENSOR = {"px4-64": (320, 240), "opencv-128": (640, 480)}
DEROTATE = (4.5, 0.05)


def sensor_frames(p, S, inp, dev, cam_w, cam_h):
    """RING ticks of S sensor frames on the device: inp.frames[k] at the crop origin of noise."""
    x0, y0 = cam_w // 2 - p.width // 2, cam_h // 2 - p.height // 2
    out = []
    for k in range(RING):
        cam = torch.randint(0, 256, (S, cam_h, cam_w), dtype=torch.uint8, device=dev)
        cam[:, y0:y0 + p.height, x0:x0 + p.width] = inp.frames[k]
        out.append(cam)
    return out


def leg_camera(p, S, path, inp, cams, dev, a, cam_w, cam_h, per_sensor=False):
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000, 1, 100, 0)
    cam = aof.bank_camera_params(cam_w, cam_h, p.width, p.height, 0, 200_000, DEROTATE, FX, FY)
    bank = eng.bank_create(bp, dev, camera=cam)
    if per_sensor:
        table = aof.bank_sensor_from_camera(p, cam, n=S)
        eng.set_bank_sensors(torch.from_numpy(table.view(np.uint8).reshape(S, 32)).to(dev), S, S * cam_w * cam_h)
    recs = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    expo = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    derot = torch.empty((S, 2), dtype=torch.float32, device=dev)
    wire = torch.empty((S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty(S, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn, ctx, bpp, cp = aof.lib.aof_bank_push_camera_device, eng._ctx, C.byref(bp), C.byref(cam)
    # the clock runs on at 13 333 us per tick across the ring's wraps, so the gate opens every 15 ticks, as on a camera
    times = torch.zeros(S, dtype=torch.int64, device=dev)
    rest = (times.data_ptr(), None, inp.gyro.data_ptr(), bank.buffer.data_ptr(), bank.buffer.numel(), recs.data_ptr(), expo.data_ptr(),
            derot.data_ptr(), wire.data_ptr(), lens.data_ptr(), stream)
    ptrs = [c.data_ptr() for c in cams]

    def step(i):
        times.add_(13333)
        rc = fn(ctx, bpp, cp, ptrs[i % RING], *rest)
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
    out = timed(step, torch.cuda.synchronize, a.ticks, a.seconds, a.settle)
    r = aof.ticks_view(recs)
    assert (r["quality"] >= aof.TICK_HELD).all() and (r["frame"] > a.ticks).all(), "the timed ticks were real ticks"
    eng.close()
    return out


def leg_pixels(p, S, path, inp, dev, a, cam_w, cam_h, leg):
    """One of G / P0 / Y / M / D of --pixel-formats on `path`: the camera tick with sensor records bound.  Stream s's frame
    lies in a slot of its own (cam_w cam_h bytes for G and P0, twice that for the packed legs), its rows cam_w * bpp bytes
    apart; inp.frames[k] sits at the centre crop, in the grey byte of each pixel; everything else is noise."""
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000, 1, 100, 0)
    cam = aof.bank_camera_params(cam_w, cam_h, p.width, p.height, 0, 200_000, DEROTATE, FX, FY)
    bank = eng.bank_create(bp, dev, camera=cam)
    fmts = {"G": None, "P0": np.zeros(S, np.uint8), "Y": np.ones(S, np.uint8), "M": (np.arange(S) % 3).astype(np.uint8),
            "D": np.ones(S, np.uint8)}[leg]
    packed = leg in ("Y", "M", "D")
    slot = cam_w * cam_h * (2 if packed else 1)
    x0, y0 = cam_w // 2 - p.width // 2, cam_h // 2 - p.height // 2
    src_fmts = fmts if packed else np.zeros(S, np.uint8)
    bpps = np.where(src_fmts == 0, 1, 2)
    cams = []
    for k in range(RING):
        buf = torch.randint(0, 256, (S, slot), dtype=torch.uint8, device=dev)
        for f in sorted(set(src_fmts.tolist())):
            idx = torch.from_numpy(np.nonzero(src_fmts == f)[0]).to(dev)
            bpp, phase = (1, 0) if f == 0 else (2, f - 1)
            view = buf[:, :cam_w * cam_h * bpp].view(S, cam_h, cam_w, bpp)
            sub = view[idx]
            sub[:, y0:y0 + p.height, x0:x0 + p.width, phase] = inp.frames[k][idx]
            view[idx] = sub
        cams.append(buf)
    grey = torch.empty((S, cam_w * cam_h), dtype=torch.uint8, device=dev) if leg == "D" else None
    table = aof.bank_sensor_from_camera(p, cam, n=S)
    if leg != "D":
        table["offset"] = np.arange(S, dtype=np.uint64) * np.uint64(slot)
        table["pitch"] = cam_w * bpps
    d_table = torch.from_numpy(table.view(np.uint8).reshape(S, 32)).to(dev)
    eng.set_bank_sensors(d_table, S, S * (cam_w * cam_h if leg == "D" else slot))
    if fmts is not None and leg != "D":
        d_fmts = torch.from_numpy(fmts).to(dev)
        eng.set_bank_pixel_formats(d_fmts, S)
    recs = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    expo = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    derot = torch.empty((S, 2), dtype=torch.float32, device=dev)
    wire = torch.empty((S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty(S, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn, ctx, bpp_, cp = aof.lib.aof_bank_push_camera_device, eng._ctx, C.byref(bp), C.byref(cam)
    times = torch.zeros(S, dtype=torch.int64, device=dev)
    rest = (times.data_ptr(), None, inp.gyro.data_ptr(), bank.buffer.data_ptr(), bank.buffer.numel(), recs.data_ptr(), expo.data_ptr(),
            derot.data_ptr(), wire.data_ptr(), lens.data_ptr(), stream)
    ptrs = [c.data_ptr() for c in cams]
    lumas = [c.view(S, cam_w * cam_h, 2)[:, :, 0] for c in cams] if leg == "D" else None

    def step(i):
        times.add_(13333)
        if leg == "D":
            grey.copy_(lumas[i % RING])
            rc = fn(ctx, bpp_, cp, grey.data_ptr(), *rest)
        else:
            rc = fn(ctx, bpp_, cp, ptrs[i % RING], *rest)
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
    out = timed(step, torch.cuda.synchronize, a.ticks, a.seconds, a.settle)
    r = aof.ticks_view(recs)
    assert (r["quality"] >= aof.TICK_HELD).all() and (r["frame"] > a.ticks).all(), "the timed ticks were real ticks"
    eng.close()
    return out


def pixel_formats_sweep(a, dev):
    print("# legs (the digit: bank path 1 / 2): G sensors bound, grey frames; P0 formats bound, all GREY8; Y all LUMA16_LO; M formats s % 3; "
          "D device de-interleave of the packed buffer, then G (exposure records, de-rotation, MAVLink frames on, all streams active)")
    print("# us = microseconds per tick (host clock, ticks ending in a synchronise)")
    bound = hasattr(aof.lib, "aof_set_bank_pixel_formats")      # (AOF_LIB may name a build without the call: G legs only)
    kinds = ["G", "P0", "Y", "M", "D"] if bound else ["G"]
    legs = [(k + str(path), k, path) for path in (1, 2) for k in kinds]
    if a.legs is not None:
        legs = [leg for leg in legs if leg[0] in a.legs.split(",")]
    sizes = [int(s) for s in a.streams.split(",")]
    results = {}
    for rep in range(a.repeats):
        for cfg in a.configs.split(","):
            p = params_of(cfg)
            cam_w, cam_h = SENSOR[cfg]
            for S in sizes:
                inp = Inputs(p, S, dev)
                for name, kind, path in legs:
                    sec, n = leg_pixels(p, S, path, inp, dev, a, cam_w, cam_h, kind)
                    results.setdefault((cfg, S, name), []).append(sec)
                    print(f"rep {rep} {cfg:11s} S={S:6d} {name:3s} {sec * 1e6:10.2f} us  ({n} ticks)", flush=True)
                    torch.cuda.empty_cache()
                del inp
    print("# ---- summary (median of the repeats; p10..p90 of the repeats in us) ----")
    for cfg in a.configs.split(","):
        for S in sizes:
            m = {n: float(np.median(results[(cfg, S, n)])) for n, _, _ in legs}
            line = f"{cfg:11s} S={S:6d}  " + "  ".join(
                f"{n} {m[n] * 1e6:9.2f} us ({np.percentile(results[(cfg, S, n)], 10) * 1e6:.2f}..{np.percentile(results[(cfg, S, n)], 90) * 1e6:.2f})"
                for n in m)
            for path in (1, 2):
                if all(k + str(path) in m for k in ("G", "P0", "Y", "M", "D")):
                    g, q, y, mm, d = (m[k + str(path)] for k in ("G", "P0", "Y", "M", "D"))
                    line += f"  P0{path}/G{path} {q / g:5.3f}  Y{path}/D{path} {y / d:5.3f}  M{path}/D{path} {mm / d:5.3f}"
            print(line)


RAW_GROUPS = {0: (1, 1, None), 1: (1, 2, 0), 2: (1, 2, 8), 4: (1, 2, 2), 5: (1, 2, 4), 6: (1, 2, 6), 7: (4, 5, None), 8: (2, 3, None)}
RAW_MIX = (0, 1, 2, 4, 5, 6, 7, 8)


def leg_raw(p, S, path, inp, dev, a, cam_w, cam_h, leg):
    """One of G / R / P / M / D of --raw-formats on `path`: the camera tick with sensor records bound.  inp.frames[k] sits at
    the centre crop as the grey values of each stream's format (include/aof.h, "raw mono pixels"); every other bit is noise."""
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000, 1, 100, 0)
    cam = aof.bank_camera_params(cam_w, cam_h, p.width, p.height, 0, 200_000, DEROTATE, FX, FY)
    bank = eng.bank_create(bp, dev, camera=cam)
    fmts = {"G": np.zeros(S, np.uint8), "R": np.full(S, 4, np.uint8), "P": np.full(S, 7, np.uint8),
            "M": np.array(RAW_MIX, np.uint8)[np.arange(S) % len(RAW_MIX)], "D": np.full(S, 4, np.uint8)}[leg]
    slot = cam_w * cam_h * (1 if leg == "G" else 2)
    x0, y0 = cam_w // 2 - p.width // 2, cam_h // 2 - p.height // 2
    assert cam_w % 4 == 0 and x0 % 4 == 0
    rows = np.array([cam_w // RAW_GROUPS[int(f)][0] * RAW_GROUPS[int(f)][1] for f in fmts])
    cams = []
    for k in range(RING):
        buf = torch.randint(0, 256, (S, slot), dtype=torch.uint8, device=dev)
        for f in sorted(set(fmts.tolist())):
            idx = torch.from_numpy(np.nonzero(fmts == f)[0]).to(dev)
            G, Bg, shift = RAW_GROUPS[f]
            frames = inp.frames[k][idx]
            if shift is None:       # a group's leading bytes are its pixels' grey values
                view = buf[:, :cam_h * (cam_w // G) * Bg].view(S, cam_h, cam_w // G, Bg)
                sub = view[idx]
                sub[:, y0:y0 + p.height, x0 // G:(x0 + p.width) // G, :G] = frames.view(len(idx), p.height, p.width // G, G)
                view[idx] = sub
            else:                   # bits shift .. shift + 7 of a little-endian word
                view = buf[:, :cam_h * cam_w * 2].view(S, cam_h, cam_w, 2)
                sub = view[idx]
                old = sub[:, y0:y0 + p.height, x0:x0 + p.width].to(torch.int32)
                word = (old[..., 0] | old[..., 1] << 8) & ~(0xFF << shift) | frames.to(torch.int32) << shift
                sub[:, y0:y0 + p.height, x0:x0 + p.width, 0] = (word & 0xFF).to(torch.uint8)
                sub[:, y0:y0 + p.height, x0:x0 + p.width, 1] = (word >> 8 & 0xFF).to(torch.uint8)
                view[idx] = sub
        cams.append(buf)
    grey = torch.empty((S, cam_w * cam_h), dtype=torch.uint8, device=dev) if leg == "D" else None
    words = torch.empty((S, cam_w * cam_h), dtype=torch.int16, device=dev) if leg == "D" else None
    table = aof.bank_sensor_from_camera(p, cam, n=S)
    if leg != "D":
        table["offset"] = np.arange(S, dtype=np.uint64) * np.uint64(slot)
        table["pitch"] = rows
    d_table = torch.from_numpy(table.view(np.uint8).reshape(S, 32)).to(dev)
    eng.set_bank_sensors(d_table, S, S * (cam_w * cam_h if leg == "D" else slot))
    if leg not in ("G", "D"):
        d_fmts = torch.from_numpy(fmts).to(dev)
        eng.set_bank_pixel_formats(d_fmts, S)
    recs = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    expo = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    derot = torch.empty((S, 2), dtype=torch.float32, device=dev)
    wire = torch.empty((S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty(S, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn, ctx, bpp_, cp = aof.lib.aof_bank_push_camera_device, eng._ctx, C.byref(bp), C.byref(cam)
    times = torch.zeros(S, dtype=torch.int64, device=dev)
    rest = (times.data_ptr(), None, inp.gyro.data_ptr(), bank.buffer.data_ptr(), bank.buffer.numel(), recs.data_ptr(), expo.data_ptr(),
            derot.data_ptr(), wire.data_ptr(), lens.data_ptr(), stream)
    ptrs = [c.data_ptr() for c in cams]
    raw16 = [c.view(torch.int16) for c in cams] if leg == "D" else None

    def step(i):
        times.add_(13333)
        if leg == "D":
            torch.bitwise_right_shift(raw16[i % RING], 2, out=words)
            grey.copy_(words)          # (narrowing: the low byte of each shifted word)
            rc = fn(ctx, bpp_, cp, grey.data_ptr(), *rest)
        else:
            rc = fn(ctx, bpp_, cp, ptrs[i % RING], *rest)
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
    out = timed(step, torch.cuda.synchronize, a.ticks, a.seconds, a.settle)
    r = aof.ticks_view(recs)
    assert (r["quality"] >= aof.TICK_HELD).all() and (r["frame"] > a.ticks).all(), "the timed ticks were real ticks"
    eng.close()
    return out


def raw_formats_sweep(a, dev):
    print("# legs (the digit: bank path 1 / 2): G sensors bound, grey frames; R all Y10; P all Y10P; M formats s % 8 over the eight; "
          "D device unpack of the Y10 buffer, then G (exposure records, de-rotation, MAVLink frames on, all streams active)")
    print("# us = microseconds per tick (host clock, ticks ending in a synchronise)")
    bound = hasattr(aof.lib, "aof_bank_pixel_row_bytes")      # (AOF_LIB may name a build without the formats: G legs only)
    kinds = ["G", "R", "P", "M", "D"] if bound else ["G"]
    legs = [(k + str(path), k, path) for path in (1, 2) for k in kinds]
    if a.legs is not None:
        legs = [leg for leg in legs if leg[0] in a.legs.split(",")]
    sizes = [int(s) for s in a.streams.split(",")]
    results = {}
    for rep in range(a.repeats):
        for cfg in a.configs.split(","):
            p = params_of(cfg)
            cam_w, cam_h = SENSOR[cfg]
            for S in sizes:
                inp = Inputs(p, S, dev)
                for name, kind, path in legs:
                    sec, n = leg_raw(p, S, path, inp, dev, a, cam_w, cam_h, kind)
                    results.setdefault((cfg, S, name), []).append(sec)
                    print(f"rep {rep} {cfg:11s} S={S:6d} {name:3s} {sec * 1e6:10.2f} us  ({n} ticks)", flush=True)
                    torch.cuda.empty_cache()
                del inp
    print("# ---- summary (median of the repeats; p10..p90 of the repeats in us) ----")
    for cfg in a.configs.split(","):
        for S in sizes:
            m = {n: float(np.median(results[(cfg, S, n)])) for n, _, _ in legs}
            line = f"{cfg:11s} S={S:6d}  " + "  ".join(
                f"{n} {m[n] * 1e6:9.2f} us ({np.percentile(results[(cfg, S, n)], 10) * 1e6:.2f}..{np.percentile(results[(cfg, S, n)], 90) * 1e6:.2f})"
                for n in m)
            for path in (1, 2):
                if all(k + str(path) in m for k in ("R", "P", "M", "D")):
                    r, q, mm, d = (m[k + str(path)] for k in ("R", "P", "M", "D"))
                    line += f"  R{path}/D{path} {r / d:5.3f}  P{path}/D{path} {q / d:5.3f}  M{path}/D{path} {mm / d:5.3f}"
            print(line)


BIN_RING = 4      # resident ticks of the --binning legs (a 4x binned 128 x 128 stream reads 576 x 576 sensor pixels)


def leg_binning(p, S, path, inp, dev, a, leg):
    """One of G / B0 / B2 / B4 / Y4 / D2 / D4 of --binning on `path` (see the module's text)."""
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    w, h = p.width, p.height
    b = {"G": 1, "B0": 1, "B2": 2, "B4": 4, "Y4": 4, "D2": 2, "D4": 4}[leg]
    bpp = 2 if leg == "Y4" else 1
    two_calls = leg in ("D2", "D4")
    cam_w, cam_h = b * (w + 16), b * (h + 16)
    slot = cam_w * cam_h * bpp
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000, 1, 100, 0)
    cam = aof.bank_camera_params(w + 16, h + 16, w, h, 0, 200_000, DEROTATE, FX, FY)
    bank = eng.bank_create(bp, dev, camera=cam)
    x0, y0 = cam_w // 2 - b * w // 2, cam_h // 2 - b * h // 2
    cams = []
    for k in range(BIN_RING):
        buf = torch.randint(0, 256, (S, cam_h, cam_w, bpp), dtype=torch.uint8, device=dev)
        buf[:, y0:y0 + b * h, x0:x0 + b * w, 0] = inp.frames[k].repeat_interleave(b, 1).repeat_interleave(b, 2)
        cams.append(buf)
    table = np.zeros(S, aof.BANK_SENSOR_DTYPE)
    table["offset"] = np.arange(S, dtype=np.uint64) * np.uint64(slot)
    table["pitch"], table["width"], table["height"], table["x0"], table["y0"] = cam_w * bpp, cam_w, cam_h, x0, y0
    d_table = torch.from_numpy(table.view(np.uint8).reshape(S, 32)).to(dev)
    d_fmts = torch.full((S,), bpp - 1, dtype=torch.uint8, device=dev)
    d_bins = torch.full((S,), b, dtype=torch.uint8, device=dev)
    grey = None
    if two_calls:      # the tick runs on the dense crops: records of w x h frames, the crop the frame
        grey = torch.empty((S, h, w), dtype=torch.uint8, device=dev)
        dense = np.zeros(S, aof.BANK_SENSOR_DTYPE)
        dense["offset"] = np.arange(S, dtype=np.uint64) * np.uint64(w * h)
        dense["pitch"], dense["width"], dense["height"] = w, w, h
        d_dense = torch.from_numpy(dense.view(np.uint8).reshape(S, 32)).to(dev)
        eng.set_bank_sensors(d_dense, S, S * w * h)
        d_grey = torch.zeros(S, dtype=torch.uint8, device=dev)
        eng.set_bank_pixel_formats(d_grey, S)
    else:
        eng.set_bank_sensors(d_table, S, S * slot)
        eng.set_bank_pixel_formats(d_fmts, S)
        if leg != "G":
            eng.set_bank_binning(d_bins, S)
    recs = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    expo = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    derot = torch.empty((S, 2), dtype=torch.float32, device=dev)
    wire = torch.empty((S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty(S, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn, ctx, bpp_, cp = aof.lib.aof_bank_push_camera_device, eng._ctx, C.byref(bp), C.byref(cam)
    times = torch.zeros(S, dtype=torch.int64, device=dev)
    rest = (times.data_ptr(), None, inp.gyro.data_ptr(), bank.buffer.data_ptr(), bank.buffer.numel(), recs.data_ptr(), expo.data_ptr(),
            derot.data_ptr(), wire.data_ptr(), lens.data_ptr(), stream)
    ptrs = [c.data_ptr() for c in cams]
    ingest = aof.lib.aof_ingest_sensors_binned_device if two_calls else None

    def step(i):
        times.add_(13333)
        if two_calls:
            rc = ingest(w, h, ptrs[i % BIN_RING], S * slot, d_table.data_ptr(), d_fmts.data_ptr(), d_bins.data_ptr(), S, grey.data_ptr(),
                        w * h, None, None, stream)
            rc = rc or fn(ctx, bpp_, cp, grey.data_ptr(), *rest)
        else:
            rc = fn(ctx, bpp_, cp, ptrs[i % BIN_RING], *rest)
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
    out = timed(step, torch.cuda.synchronize, a.ticks, a.seconds, a.settle)
    r = aof.ticks_view(recs)
    assert (r["quality"] >= aof.TICK_HELD).all() and (r["frame"] > a.ticks).all(), "the timed ticks were real ticks"
    eng.close()
    return out


def binning_sweep(a, dev):
    print("# legs (the digit: bank path 1 / 2): G sensors and formats bound, no bins; B0 bins bound, all ones; B2 / B4 every stream binned; "
          "Y4 LUMA16_LO binned 4x; D2 / D4 aof_ingest_sensors_binned_device into a grey buffer, then G on it "
          "(exposure records, de-rotation, MAVLink frames on, all streams active)")
    print("# us = microseconds per tick (host clock, ticks ending in a synchronise)")
    bound = hasattr(aof.lib, "aof_set_bank_binning")      # (AOF_LIB may name a build without the call: G legs only)
    kinds = ["G", "B0", "B2", "B4", "Y4", "D2", "D4"] if bound else ["G"]
    legs = [(k + str(path), k, path) for path in (1, 2) for k in kinds]
    if a.legs is not None:
        legs = [leg for leg in legs if leg[0] in a.legs.split(",")]
    sizes = [int(s) for s in a.streams.split(",")]
    results = {}
    for rep in range(a.repeats):
        for cfg in a.configs.split(","):
            p = params_of(cfg)
            for S in sizes:
                inp = Inputs(p, S, dev)
                for name, kind, path in legs:
                    sec, n = leg_binning(p, S, path, inp, dev, a, kind)
                    results.setdefault((cfg, S, name), []).append(sec)
                    print(f"rep {rep} {cfg:11s} S={S:6d} {name:3s} {sec * 1e6:10.2f} us  ({n} ticks)", flush=True)
                    torch.cuda.empty_cache()
                del inp
    print("# ---- summary (median of the repeats; p10..p90 of the repeats in us) ----")
    for cfg in a.configs.split(","):
        for S in sizes:
            m = {n: float(np.median(results[(cfg, S, n)])) for n, _, _ in legs}
            line = f"{cfg:11s} S={S:6d}  " + "  ".join(
                f"{n} {m[n] * 1e6:9.2f} us ({np.percentile(results[(cfg, S, n)], 10) * 1e6:.2f}..{np.percentile(results[(cfg, S, n)], 90) * 1e6:.2f})"
                for n in m)
            for path in (1, 2):
                if all(k + str(path) in m for k in kinds) and bound:
                    g, b0, b2, b4, y4, d2, d4 = (m[k + str(path)] for k in ("G", "B0", "B2", "B4", "Y4", "D2", "D4"))
                    line += (f"  B0{path}/G{path} {b0 / g:5.3f}  B2{path}/G{path} {b2 / g:5.3f}  B4{path}/G{path} {b4 / g:5.3f}  Y4{path}/G{path} {y4 / g:5.3f}"
                             f"  B2{path}/D2{path} {b2 / d2:5.3f}  B4{path}/D4{path} {b4 / d4:5.3f}")
            print(line)


WARP_RING = 4          # ticks of 640 x 480 sensor frames resident per size (2 048 streams: 2.5 GB)
WARP_SENSOR = (640, 480)


def tiled_sensor_frames(p, S, inp, dev, cam_w, cam_h, ring):
    """`ring` ticks of S sensor frames on the device: inp.frames[k] at the crop origin and repeated around it, so that a
    mesh that reaches outside the plain crop still reads moving texture (noise there would time another search)."""
    w, h = p.width, p.height
    x0, y0 = cam_w // 2 - w // 2, cam_h // 2 - h // 2
    ys = (torch.arange(cam_h, device=dev) - y0) % h
    xs = (torch.arange(cam_w, device=dev) - x0) % w
    return [inp.frames[k][:, ys][:, :, xs].contiguous() for k in range(ring)]


def leg_warp(p, S, inp, cams, dev, a, leg):
    """One of P / I / L / F / U / W / WI of --warp (see warp_sweep's text): the camera tick on 640 x 480 grey frames."""
    eng = aof.FlowEngine(p, 0)
    w, h = p.width, p.height
    cam_w, cam_h = WARP_SENSOR
    path = {"P": 2, "I": 2, "L": 2, "F": 1, "U": 0, "W": 1, "WI": 1}[leg]
    eng.set_bank_path(path)
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000, 1, 100, 0)
    two_calls = leg == "U"
    cam = aof.bank_camera_params(w if two_calls else cam_w, h if two_calls else cam_h, w, h, 0, 200_000, DEROTATE, FX, FY)
    bank = eng.bank_create(bp, dev, camera=cam)
    x0, y0 = cam_w // 2 - w // 2, cam_h // 2 - h // 2
    d_points = d_table = grey = None
    if leg in ("I", "L", "U", "W", "WI"):
        # the lens of a short downward camera: 13 % barrel at the crop's corner, seen by a pinhole camera of the same focal length
        f = 0.9 * max(w, h)
        mesh = aof.warp_mesh_identity(p, x0, y0) if leg in ("I", "WI") else aof.warp_mesh_from_lens(p, f, f, cam_w / 2.0, cam_h / 2.0, k1=-0.28, k2=0.07)
        d_points = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(mesh, (S,) + mesh.shape)).view(np.uint8).reshape(S, -1)).to(dev)
    if two_calls:
        table = aof.bank_sensor_from_camera(p, aof.bank_camera_params(cam_w, cam_h, w, h, 0, 200_000, DEROTATE, FX, FY), n=S)
        d_table = torch.from_numpy(table.view(np.uint8).reshape(S, 32)).to(dev)
        grey = torch.empty((S, h, w), dtype=torch.uint8, device=dev)
    elif d_points is not None:
        eng.set_bank_warps(d_points, S)
    recs = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    expo = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    derot = torch.empty((S, 2), dtype=torch.float32, device=dev)
    wire = torch.empty((S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty(S, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn, ctx, bpp, cp = aof.lib.aof_bank_push_camera_device, eng._ctx, C.byref(bp), C.byref(cam)
    times = torch.zeros(S, dtype=torch.int64, device=dev)
    rest = (times.data_ptr(), None, inp.gyro.data_ptr(), bank.buffer.data_ptr(), bank.buffer.numel(), recs.data_ptr(), expo.data_ptr(),
            derot.data_ptr(), wire.data_ptr(), lens.data_ptr(), stream)
    ptrs = [c.data_ptr() for c in cams]
    unwarp = aof.lib.aof_ingest_warped_device if two_calls else None

    def step(i):
        times.add_(13333)
        if two_calls:
            rc = unwarp(w, h, ptrs[i % WARP_RING], S * cam_w * cam_h, d_table.data_ptr(), None, d_points.data_ptr(), S, grey.data_ptr(), w * h,
                        None, None, stream)
            rc = rc or fn(ctx, bpp, cp, grey.data_ptr(), *rest)
        else:
            rc = fn(ctx, bpp, cp, ptrs[i % WARP_RING], *rest)
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
    out = timed(step, torch.cuda.synchronize, a.ticks, a.seconds, a.settle)
    r = aof.ticks_view(recs)
    assert (r["quality"] >= aof.TICK_HELD).all() and (r["frame"] > a.ticks).all(), "the timed ticks were real ticks"
    if path and hasattr(aof.lib, "aof_bank_last_path"):
        assert eng.last_bank_path() == path, (leg, "timed path", eng.last_bank_path(), "meant", path)
    eng.close()
    return out


WARP_BURST_K = 5


def leg_warp_burst(p, S, dev, a, path):
    """WB1 / WB2 of --warp: one camera burst of K = 5 rounds per step with the barrel lens bound, on `path`."""
    w, h = p.width, p.height
    cam_w, cam_h = WARP_SENSOR
    f = 0.9 * max(w, h)
    mesh = aof.warp_mesh_from_lens(p, f, f, cam_w / 2.0, cam_h / 2.0, k1=-0.28, k2=0.07)
    points = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(mesh, (S,) + mesh.shape)).view(np.uint8).reshape(S, -1)).to(dev)
    inp = BurstInputs(p, S, WARP_BURST_K, dev, sensor=WARP_SENSOR)
    return leg_burst(p, S, WARP_BURST_K, path, inp, dev, a, WARP_SENSOR, False, points=points)


def warp_sweep(a, dev):
    print("# legs, all on 640 x 480 grey sensor frames: P the composed camera tick (path 2), nothing bound; I the same with identity meshes bound; "
          "L with the mesh of a barrel lens (k1 -0.28, k2 0.07); F the one-launch camera tick (path 1), nothing bound: what a warped bank gives up; "
          "U aof_ingest_warped_device into a grey buffer, then the camera tick on it (path 0): a separate unwarp launch "
          "(exposure records, de-rotation, MAVLink frames on, all streams active)")
    print("# us = microseconds per tick (host clock, ticks ending in a synchronise)")
    bound = hasattr(aof.lib, "aof_set_bank_warps")      # (AOF_LIB may name a build without the call: P and F only)
    legs = ["P", "I", "L", "F", "U"] if bound else ["P", "F"]
    if hasattr(aof.lib, "aof_bank_last_path"):          # (the build with the warp inside the one-launch tick)
        print("# W the barrel lens on path 1 (the one-launch tick with the warp inside it); WI identity meshes on path 1; WB1 / WB2 a burst of "
              f"K = {WARP_BURST_K} rounds with the lens on path 1 / path 2, us per burst (noise around the crop); each asserts aof_bank_last_path")
        legs += ["W", "WI", "WB1", "WB2"]
    if a.legs is not None:
        legs = [leg for leg in legs if leg in a.legs.split(",")]
    sizes = [int(s) for s in a.streams.split(",")]
    results = {}
    for rep in range(a.repeats):
        for cfg in a.configs.split(","):
            p = params_of(cfg)
            for S in sizes:
                inp = Inputs(p, S, dev)
                cams = tiled_sensor_frames(p, S, inp, dev, *WARP_SENSOR, WARP_RING)
                for name in legs:
                    sec, n = leg_warp_burst(p, S, dev, a, int(name[2])) if name.startswith("WB") else leg_warp(p, S, inp, cams, dev, a, name)
                    results.setdefault((cfg, S, name), []).append(sec)
                    print(f"rep {rep} {cfg:11s} S={S:6d} {name:2s} {sec * 1e6:10.2f} us  ({n} ticks)", flush=True)
                del inp, cams
                torch.cuda.empty_cache()
    print("# ---- summary (median of the repeats; p10..p90 of the repeats in us) ----")
    for cfg in a.configs.split(","):
        for S in sizes:
            m = {n: float(np.median(results[(cfg, S, n)])) for n in legs}
            line = f"{cfg:11s} S={S:6d}  " + "  ".join(
                f"{n} {m[n] * 1e6:9.2f} us ({np.percentile(results[(cfg, S, n)], 10) * 1e6:.2f}..{np.percentile(results[(cfg, S, n)], 90) * 1e6:.2f})"
                for n in m)
            if all(n in m for n in ("P", "I", "L", "F", "U")):
                line += f"  I/P {m['I'] / m['P']:5.3f}  L/P {m['L'] / m['P']:5.3f}  L/F {m['L'] / m['F']:5.3f}  L/U {m['L'] / m['U']:5.3f}"
            if all(n in m for n in ("L", "F", "W")):
                line += f"  W/F {m['W'] / m['F']:5.3f}  W/L {m['W'] / m['L']:5.3f}"
            if all(n in m for n in ("WB1", "WB2")):
                line += f"  WB1/WB2 {m['WB1'] / m['WB2']:5.3f}"
            print(line)


def leg_two_calls(p, S, inp, cams, dev, a, cam_w, cam_h):
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000, 1, 100, 0)
    bank = eng.bank_create(bp, dev)
    frames = torch.empty((S, p.height, p.width), dtype=torch.uint8, device=dev)
    hist = torch.empty((S, 10), dtype=torch.int32, device=dev)
    recs = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    wire = torch.empty((S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty(S, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ingest, push, ctx, bpp = aof.lib.aof_ingest_batch_device, aof.lib.aof_bank_push_device, eng._ctx, C.byref(bp)
    ip = aof.IngestParams(cam_w, cam_h, p.width, p.height)
    ipp = C.byref(ip)
    times = torch.zeros(S, dtype=torch.int64, device=dev)
    ptrs = [c.data_ptr() for c in cams]
    ing = (cam_w * cam_h, S, frames.data_ptr(), p.width * p.height, hist.data_ptr(), stream)
    rest = (frames.data_ptr(), times.data_ptr(), None, inp.gyro.data_ptr(), bank.buffer.data_ptr(), bank.buffer.numel(), recs.data_ptr(),
            wire.data_ptr(), lens.data_ptr(), stream)

    def step(i):
        times.add_(13333)
        rc = ingest(ipp, ptrs[i % RING], *ing) or push(ctx, bpp, *rest)
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
    out = timed(step, torch.cuda.synchronize, a.ticks, a.seconds, a.settle)
    eng.close()
    return out


def leg_plain(p, S, inp, dev, a):
    """leg_tick with the camera legs' running clock (one more small kernel per tick, like theirs)."""
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000, 1, 100, 0)
    bank = eng.bank_create(bp, dev)
    recs = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    wire = torch.empty((S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty(S, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn, ctx, bpp = aof.lib.aof_bank_push_device, eng._ctx, C.byref(bp)
    times = torch.zeros(S, dtype=torch.int64, device=dev)
    ptrs = [f.data_ptr() for f in inp.frames[:RING]]
    rest = (times.data_ptr(), None, inp.gyro.data_ptr(), bank.buffer.data_ptr(), bank.buffer.numel(), recs.data_ptr(), wire.data_ptr(),
            lens.data_ptr(), stream)

    def step(i):
        times.add_(13333)
        rc = fn(ctx, bpp, ptrs[i % RING], *rest)
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
    out = timed(step, torch.cuda.synchronize, a.ticks, a.seconds, a.settle)
    eng.close()
    return out


def camera_sweep(a, dev):
    print("# legs: K0/K1/K2 camera tick on path 0/1/2 (statistics at 200 000 us, gyro, MAVLink frames, de-rotation), "
          "Y = aof_ingest_batch_device + aof_bank_push_device, T0 = plain tick on pre-cropped frames; every leg advances its clock "
          "on the device per tick (one small kernel more than a caller with real time stamps)")
    print("# us = microseconds per tick (host clock, ticks ending in a synchronise)")
    sizes = [int(s) for s in a.streams.split(",")]
    results = {}
    for rep in range(a.repeats):
        for cfg in a.configs.split(","):
            p = params_of(cfg)
            cw, ch = SENSOR[cfg]
            for S in sizes:
                inp = Inputs(p, S, dev)
                cams = sensor_frames(p, S, inp, dev, cw, ch)
                legs = [("K0", lambda: leg_camera(p, S, 0, inp, cams, dev, a, cw, ch)), ("Y", lambda: leg_two_calls(p, S, inp, cams, dev, a, cw, ch)),
                        ("T0", lambda: leg_plain(p, S, inp, dev, a))]
                if S >= 1024:
                    legs += [("K1", lambda: leg_camera(p, S, 1, inp, cams, dev, a, cw, ch)), ("K2", lambda: leg_camera(p, S, 2, inp, cams, dev, a, cw, ch))]
                for name, fn in legs:
                    sec, n = fn()
                    results.setdefault((cfg, S, name), []).append(sec)
                    print(f"rep {rep} {cfg:11s} {cw}x{ch} S={S:6d} {name:2s} {sec * 1e6:10.2f} us  {1 / sec:12.0f} ticks/s  ({n} ticks)", flush=True)
                del inp, cams
                torch.cuda.empty_cache()
    print("# ---- summary (mean of the repeats; spread = |difference of the repeats| / mean) ----")
    for cfg in a.configs.split(","):
        p = params_of(cfg)
        print(f"# {cfg}: frame bytes per stream and tick: camera tick on the one-launch path {3 * p.width * p.height}, two calls {5 * p.width * p.height}")
        for S in sizes:
            m = {n: float(np.mean(results[(cfg, S, n)])) for n in ("K0", "Y", "T0", "K1", "K2") if (cfg, S, n) in results}
            sp = {n: (abs(results[(cfg, S, n)][0] - results[(cfg, S, n)][-1]) / m[n]) for n in m}
            gain = (m["Y"] - m["K0"]) / m["Y"]
            line = (f"{cfg:11s} S={S:6d}  K0 {m['K0'] * 1e6:9.2f} us (+-{sp['K0'] * 100:4.1f} %)  Y {m['Y'] * 1e6:9.2f} (+-{sp['Y'] * 100:4.1f} %)  "
                    f"T0 {m['T0'] * 1e6:9.2f} (+-{sp['T0'] * 100:4.1f} %)  K0 below Y by {gain * 100:5.1f} % "
                    f"({'more' if gain > sp['K0'] + sp['Y'] else 'NOT more'} than the legs' spread)  K0/T0 {m['K0'] / m['T0']:5.3f}")
            if "K1" in m:
                line += (f"  K1 {m['K1'] * 1e6:9.2f} (+-{sp['K1'] * 100:4.1f} %)  K2 {m['K2'] * 1e6:9.2f} (+-{sp['K2'] * 100:4.1f} %)  "
                         f"faster path {'K1' if m['K1'] <= m['K2'] else 'K2'}")
            print(line)


def timed_bursts(step, sync, K, min_rounds, min_seconds, settle_seconds):
    """step() enqueues K frame rounds (one burst, or K ticks).  Returns (seconds per K rounds, rounds timed)."""
    chunk = max(4, 128 // K)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < settle_seconds:
        for _ in range(chunk):
            step()
        sync()
    done, elapsed = 0, 0.0
    while done * K < min_rounds or elapsed < min_seconds:
        t0 = time.perf_counter()
        for _ in range(chunk):
            step()
        sync()
        elapsed += time.perf_counter() - t0
        done += chunk
    return elapsed / done, done * K


class BurstInputs:
    """K rounds of S streams on the device, round-major: frames [K, S, h, w] (camera: sensor frames [K, S, ch, cw] with
    the frames at the crop origin of noise), times [K, S] (13 333 us per round), gyro [K, S, 4]."""

    def __init__(self, p, S, K, dev, sensor=None):
        w, h = p.width, p.height
        pool = np.stack([synth.make_sequence(w, h, K, 4, seed=500 + k, max_step=3)[0] for k in range(POOL)])   # [POOL, K, h, w]
        idx = torch.from_numpy(np.arange(S) % POOL).to(dev)
        frames = torch.from_numpy(pool).to(dev)[idx].transpose(0, 1).contiguous()                               # [K, S, h, w]
        if sensor is None:
            self.frames = frames
        else:
            cw, ch = sensor
            x0, y0 = cw // 2 - w // 2, ch // 2 - h // 2
            self.frames = torch.randint(0, 256, (K, 1, ch, cw), dtype=torch.uint8, device=dev).repeat(1, S, 1, 1)
            self.frames[:, :, y0:y0 + h, x0:x0 + w] = frames
        self.round_bytes = self.frames[0].numel()
        self.times0 = (torch.arange(K, dtype=torch.int64, device=dev).view(K, 1) + 1).repeat(1, S) * 13333
        self.gyro = torch.full((K, S, 4), 0.001, dtype=torch.float32, device=dev)


def leg_burst(p, S, K, path, inp, dev, a, sensor, single_ticks, points=None):
    """One burst of K rounds per step, or (single_ticks) K calls of the single tick on the same buffers, round by round.
    points: S warp meshes to bind (--warp's burst legs, which assert the path they timed)."""
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    if points is not None:
        eng.set_bank_warps(points, S)
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000, 1, 100, 0)
    cam = aof.bank_camera_params(sensor[0], sensor[1], p.width, p.height, 0, 200_000, DEROTATE, FX, FY) if sensor else None
    bank = eng.bank_create(bp, dev, camera=cam)
    recs = torch.empty((K, S, 48), dtype=torch.uint8, device=dev)
    expo = torch.empty((K, S, 48), dtype=torch.uint8, device=dev)
    derot = torch.empty((K, S, 2), dtype=torch.float32, device=dev)
    wire = torch.empty((K, S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty((K, S), dtype=torch.uint8, device=dev)
    times = inp.times0.clone()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctx, bpp, cp = eng._ctx, C.byref(bp), C.byref(cam) if cam else None
    burst = aof.bank_burst_params(K)
    bank_args = (bank.buffer.data_ptr(), bank.buffer.numel())

    def rounds(k):   # the pointers of round k (k = 0: of the whole burst)
        f, t, g = inp.frames.data_ptr() + k * inp.round_bytes, times.data_ptr() + k * S * 8, inp.gyro.data_ptr() + k * S * 16
        r, w, n = recs.data_ptr() + k * S * 48, wire.data_ptr() + k * S * 56, lens.data_ptr() + k * S
        if cam:
            return (f, t, None, g) + bank_args + (r, expo.data_ptr() + k * S * 48, derot.data_ptr() + k * S * 8, w, n, stream)
        return (f, t, None, g) + bank_args + (r, w, n, stream)
    if single_ticks:
        fn = aof.lib.aof_bank_push_camera_device if cam else aof.lib.aof_bank_push_device
        head = (ctx, bpp, cp) if cam else (ctx, bpp)
        calls = [head + rounds(k) for k in range(K)]
    else:
        fn = aof.lib.aof_bank_push_camera_burst_device if cam else aof.lib.aof_bank_push_burst_device
        head = (ctx, bpp, cp, C.byref(burst)) if cam else (ctx, bpp, C.byref(burst))
        calls = [head + rounds(0)]
    step_us = 13333 * K

    def step():
        times.add_(step_us)      # the clock runs on across the bursts (one small kernel per K rounds, in every leg)
        for c in calls:
            rc = fn(*c)
            if rc:
                raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
    out = timed_bursts(step, torch.cuda.synchronize, K, a.ticks, a.seconds, a.settle)
    r = aof.ticks_view(recs[K - 1])
    assert (r["quality"] >= aof.TICK_HELD).all() and (r["frame"] > a.ticks).all(), "the timed rounds were real rounds"
    if points is not None:
        assert eng.last_bank_path() == path, ("timed path", eng.last_bank_path(), "meant", path)
    eng.close()
    return out


def burst_sweep(a, dev):
    print("# legs: B0/B1/B2 one burst of K rounds on path 0/1/2, T0/T1/T2 K calls of the single tick on the same buffers on path 0/1/2 "
          "(all streams in all rounds, gyro, MAVLink frames; camera form: statistics at 200 000 us, de-rotation); every leg advances "
          "its clock on the device once per K rounds")
    print("# us = microseconds per K rounds (host clock, chunks of steps ending in a synchronise)")
    sizes = [int(s) for s in a.streams.split(",")]
    forms, ks = a.forms.split(","), [int(k) for k in a.burst.split(",")]
    legs = [("B0", 0, False), ("T0", 0, True), ("B1", 1, False), ("T1", 1, True), ("B2", 2, False), ("T2", 2, True)]
    results, skipped = {}, set()
    # (--legs B1,...: a subset, for comparing two builds of the library loaded through AOF_LIB; no summary then)
    want = [n for n, _, _ in legs] if a.legs == "T0,T1,T2,C,B" else a.legs.split(",")
    for rep in range(a.repeats):
        for cfg in a.configs.split(","):
            p = params_of(cfg)
            for form in forms:
                sensor = SENSOR[cfg] if form == "camera" else None
                for K in ks:
                    for S in sizes:
                        item = sensor[0] * sensor[1] if sensor else p.width * p.height
                        if K * S * item > a.input_bytes_max:
                            skipped.add((cfg, form, K, S))
                            print(f"rep {rep} {cfg:11s} {form:6s} K={K:2d} S={S:6d} skipped: {K * S * item / 2**30:.1f} GiB of input", flush=True)
                            continue
                        inp = BurstInputs(p, S, K, dev, sensor)
                        for name, path, single in legs:
                            if name not in want:
                                continue
                            sec, n = leg_burst(p, S, K, path, inp, dev, a, sensor, single)
                            results.setdefault((cfg, form, K, S, name), []).append(sec)
                            print(f"rep {rep} {cfg:11s} {form:6s} K={K:2d} S={S:6d} {name:2s} {sec * 1e6:10.2f} us  {sec / K * 1e6:9.2f} us/round  "
                                  f"({n} rounds)", flush=True)
                        del inp
                        torch.cuda.empty_cache()
    if len(want) != len(legs):
        return
    print("# ---- summary (mean of the repeats; spread = |difference of the repeats| / mean) ----")
    for cfg in a.configs.split(","):
        p = params_of(cfg)
        for form in forms:
            for K in ks:
                print(f"# {cfg} {form} K={K}: frame bytes per stream, burst on the one-launch path {(K + 2) * p.width * p.height}, K ticks {3 * K * p.width * p.height}")
                for S in sizes:
                    if (cfg, form, K, S) in skipped:
                        continue
                    m = {n: float(np.mean(results[(cfg, form, K, S, n)])) for n, _, _ in legs}
                    sp = {n: abs(results[(cfg, form, K, S, n)][0] - results[(cfg, form, K, S, n)][-1]) / m[n] for n in m}
                    gain = (m["T0"] - m["B0"]) / m["T0"]
                    print(f"{cfg:11s} {form:6s} K={K:2d} S={S:6d}  " + "  ".join(f"{n} {m[n] * 1e6:9.2f} (+-{sp[n] * 100:4.1f} %)" for n in m) +
                          f"  B0 below T0 by {gain * 100:5.1f} % ({'more' if gain > sp['B0'] + sp['T0'] else 'NOT more'} than the legs' spread)  "
                          f"T0/B0 {m['T0'] / m['B0']:5.2f}  T1/B1 {m['T1'] / m['B1']:5.2f}  faster burst path {'B1' if m['B1'] <= m['B2'] else 'B2'}  "
                          f"B0/best {m['B0'] / min(m['B1'], m['B2']):5.3f}")


class OutboxInputs:
    """K rounds of S streams per step on the device: RING steps of frames [K, S, h, w]; the streams' clocks run on by
    9 000..18 000 us per frame (the test recipe's spacing), drawn once per ring slot."""

    def __init__(self, p, S, K, dev):
        w, h = p.width, p.height
        pool = np.stack([synth.make_sequence(w, h, RING * K, 4, seed=500 + k, max_step=3)[0] for k in range(POOL)])   # [POOL, RING * K, h, w]
        idx = torch.from_numpy(np.arange(S) % POOL).to(dev)
        pool_d = torch.from_numpy(pool).to(dev)
        self.frames = [pool_d[:, k * K:(k + 1) * K][idx].transpose(0, 1).contiguous() for k in range(RING)]          # [K, S, h, w] each
        rng = np.random.default_rng(7)
        step = rng.integers(9000, 18000, (RING, K, S)).astype(np.int64)
        self.offsets = torch.from_numpy(np.cumsum(step, axis=1)).to(dev)       # [RING, K, S]: round k's time behind the step's start
        self.advance = self.offsets[:, K - 1].contiguous()                      # [RING, S]
        self.gyro = torch.full((K, S, 4), 0.001, dtype=torch.float32, device=dev)


def hip_runtime():
    """hipMemcpyAsync / hipStreamSynchronize of the HIP runtime torch has loaded (the H leg's copies without torch's
    per-call overhead)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    return hip


def leg_outbox(p, S, K, rate, leg, inp, dev, a):
    """One of T / D / H / O on K rounds per step (K = 1: the tick, else the burst call).  Returns (seconds per step,
    steps, messages per step)."""
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S, FX, FY, rate, 5_000_000, 1, 100, 0)
    bank = eng.bank_create(bp, dev)
    n = K * S
    recs = torch.empty((K, S, 48), dtype=torch.uint8, device=dev)
    wire = torch.empty((K, S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty((K, S), dtype=torch.uint8, device=dev)
    clock = torch.zeros(S, dtype=torch.int64, device=dev)
    times = torch.zeros((K, S), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctx, bpp = eng._ctx, C.byref(bp)
    burst = aof.bank_burst_params(K)
    tail = (times.data_ptr(), None, inp.gyro.data_ptr(), bank.buffer.data_ptr(), bank.buffer.numel(), recs.data_ptr(), wire.data_ptr(),
            lens.data_ptr(), stream)
    if K == 1:
        push, head = aof.lib.aof_bank_push_device, (ctx, bpp)
    else:
        push, head = aof.lib.aof_bank_push_burst_device, (ctx, bpp, C.byref(burst))
    ptrs = [f.data_ptr() for f in inp.frames]
    collect = aof.lib.aof_bank_collect_device
    counts = []

    def tick(i):
        torch.add(clock, inp.offsets[i % RING], out=times)      # the clocks run on across the ring's wraps (two small kernels
        clock.add_(inp.advance[i % RING])                       # per step, in every leg)
        rc = push(*head, ptrs[i % RING], *tail)
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())

    if leg == "T":
        out = timed(tick, torch.cuda.synchronize, a.ticks, a.seconds, a.settle)
    elif leg == "D":
        box = torch.empty(aof.outbox_layout(n, 0).total_bytes, dtype=torch.uint8, device=dev)
        cargs = (ctx, S, K, recs.data_ptr(), wire.data_ptr(), lens.data_ptr(), None, None, n, 0, box.data_ptr(), box.numel(), 1, None, stream)

        def step(i):
            tick(i)
            rc = collect(*cargs)
            if rc:
                raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
        out = timed(step, torch.cuda.synchronize, a.ticks, a.seconds, a.settle)
        counts.append(int(aof.outbox_view(box)[0]["n_messages"]))
    elif leg == "H":
        hip = hip_runtime()
        h_recs = torch.empty((n, 48), dtype=torch.uint8, pin_memory=True)
        h_wire = torch.empty((n, 56), dtype=torch.uint8, pin_memory=True)
        h_lens = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        quality = h_recs.numpy().view(aof.TICK_DTYPE).reshape(n)["quality"]
        copies = [(h.data_ptr(), d.data_ptr(), d.numel()) for h, d in ((h_recs, recs), (h_lens, lens), (h_wire, wire))]

        def step(i):
            tick(i)
            for dst, src, size in copies:
                if hip.hipMemcpyAsync(dst, src, size, 2, stream):           # hipMemcpyDeviceToHost
                    raise RuntimeError("hipMemcpyAsync failed")
            if hip.hipStreamSynchronize(stream):
                raise RuntimeError("hipStreamSynchronize failed")
            counts.append(len(np.flatnonzero(quality >= 0)))
        out = timed(step, lambda: None, a.ticks, a.seconds, a.settle)
    else:
        host = aof.HostOutbox(n)
        tagword = host.array[:8].view("<u8")
        n_messages = host.array[8:12].view("<u4")
        before, after = (ctx, S, K, recs.data_ptr(), wire.data_ptr(), lens.data_ptr(), None, None, n, 0, host.ptr, host.nbytes), (None, stream)

        def step(i):
            tick(i)
            tag = i + 1
            rc = collect(*before, tag, *after)
            if rc:
                raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
            deadline = time.perf_counter() + 5.0
            while tagword[0] != tag:
                if time.perf_counter() > deadline:
                    raise RuntimeError("the outbox tag did not arrive within 5 s")
            counts.append(int(n_messages[0]))
        out = timed(step, lambda: None, a.ticks, a.seconds, a.settle)
        torch.cuda.synchronize()
        host.close()
    torch.cuda.synchronize()
    r = aof.ticks_view(recs[K - 1])
    assert (r["quality"] >= aof.TICK_HELD).all() and (r["frame"] > a.ticks).all(), "the timed ticks were real ticks"
    eng.close()
    return out[0], out[1], float(np.mean(counts[-256:])) if counts else float("nan")


def outbox_sweep(a, dev):
    print("# legs: T tick alone (pipelined), D tick + collect into a device outbox (pipelined), H tick + 3 async D2H copies (records, "
          "lengths, frames) into pinned memory + stream synchronise + np.flatnonzero(quality >= 0), O tick + collect into a HostOutbox "
          "+ polling the tag; MAVLink frames on, all streams active, gyro; every leg advances its clocks on the device per step")
    print("# us = microseconds per step (a tick, or a burst of K rounds); T and D: host clock around chunks of steps ending in a "
          "synchronise; H and O: every step ends with the host holding the list; msgs = messages per step the leg's host saw")
    sizes = [int(s) for s in a.streams.split(",")]
    cases = [(cfg, 1, rate, S) for cfg in a.configs.split(",") for rate in (15, 0) for S in sizes]
    cases += [(cfg, 5, 15, S) for cfg, S in (("px4-64", 4096),) if cfg in a.configs.split(",")]        # the one burst line
    results, msgs = {}, {}
    for rep in range(a.repeats):
        for cfg, K, rate, S in cases:
            p = params_of(cfg)
            inp = OutboxInputs(p, S, K, dev)
            for leg in ("T", "D", "H", "O"):
                sec, n, m = leg_outbox(p, S, K, rate, leg, inp, dev, a)
                results.setdefault((cfg, K, rate, S, leg), []).append(sec)
                msgs[(cfg, K, rate, S, leg)] = m
                print(f"rep {rep} {cfg:11s} K={K:2d} rate={rate:2d} S={S:6d} {leg} {sec * 1e6:10.2f} us  ({n} steps, msgs {m:9.1f})", flush=True)
            del inp
            torch.cuda.empty_cache()
    print("# ---- summary (mean of the repeats; spread = |difference of the repeats| / mean) ----")
    for cfg, K, rate, S in cases:
        m = {leg: float(np.mean(results[(cfg, K, rate, S, leg)])) for leg in "TDHO"}
        sp = {leg: abs(results[(cfg, K, rate, S, leg)][0] - results[(cfg, K, rate, S, leg)][-1]) / m[leg] for leg in "TDHO"}
        gain = (m["H"] - m["O"]) / m["H"]
        print(f"{cfg:11s} K={K:2d} rate={rate:2d} S={S:6d}  " + "  ".join(f"{leg} {m[leg] * 1e6:9.2f} (+-{sp[leg] * 100:4.1f} %)" for leg in "TDHO") +
              f"  D-T {(m['D'] - m['T']) * 1e6:7.2f} us  msgs/step {msgs[(cfg, K, rate, S, 'O')]:9.1f} of {K * S}  "
              f"O below H by {gain * 100:5.1f} % ({'more' if gain > sp['O'] + sp['H'] else 'NOT more'} than the legs' spread)  H/O {m['H'] / m['O']:5.2f}")


def leg_exposure(p, S, K, leg, inp, dev, a, sensor):
    """One of T / C / H on K rounds of sensor frames per step.  Returns (seconds per step, rounds timed, controller
    steps per stream at the end)."""
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000, 1, 100, 0)
    cam = aof.bank_camera_params(sensor[0], sensor[1], p.width, p.height, 0, 200_000, None, FX, FY)
    bank = eng.bank_create(bp, dev, camera=cam)
    n = K * S
    recs = torch.empty((K, S, 48), dtype=torch.uint8, device=dev)
    expo = torch.empty((K, S, 48), dtype=torch.uint8, device=dev)
    wire = torch.empty((K, S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty((K, S), dtype=torch.uint8, device=dev)
    times = inp.times0.clone()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctx, burst, ec = eng._ctx, aof.bank_burst_params(K), aof.exposure_control_default()
    tail = (inp.frames.data_ptr(), times.data_ptr(), None, inp.gyro.data_ptr(), bank.buffer.data_ptr(), bank.buffer.numel(),
            recs.data_ptr(), expo.data_ptr(), None, wire.data_ptr(), lens.data_ptr(), stream)
    if K == 1:
        push, head = aof.lib.aof_bank_push_camera_device, (ctx, C.byref(bp), C.byref(cam))
    else:
        push, head = aof.lib.aof_bank_push_camera_burst_device, (ctx, C.byref(bp), C.byref(cam), C.byref(burst))

    def tick():
        times.add_(13333 * K)                                   # the clocks run on: the gate opens every 15 rounds
        rc = push(*head, *tail)
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())

    if leg == "T":
        out = timed_bursts(tick, torch.cuda.synchronize, K, a.ticks, a.seconds, a.settle)
        updates = float("nan")
    elif leg == "C":
        state = torch.zeros((S, 16), dtype=torch.uint8, device=dev)
        eng.bank_exposure_reset(state, exposure0=400, gain0=1)
        commands = torch.empty((K, S, 16), dtype=torch.uint8, device=dev)
        control = aof.lib.aof_bank_exposure_control_device
        cargs = (ctx, C.byref(ec), S, K, expo.data_ptr(), state.data_ptr(), commands.data_ptr(), stream)

        def step():
            tick()
            rc = control(*cargs)
            if rc:
                raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
        out = timed_bursts(step, torch.cuda.synchronize, K, a.ticks, a.seconds, a.settle)
        updates = float(aof.exposure_states_view(state)["updates"].mean())
    else:
        hip = hip_runtime()
        h_expo = torch.empty((n, 48), dtype=torch.uint8, pin_memory=True)
        states = np.zeros(S, aof.EXPOSURE_STATE_DTYPE)
        states["exposure"], states["gain"] = 400, 1
        commands = np.empty(n, aof.EXPOSURE_COMMAND_DTYPE)
        host = aof.lib.aof_exposure_control_host
        hargs = (C.byref(ec), S, K, h_expo.data_ptr(), states.ctypes.data, commands.ctypes.data)
        copy = (h_expo.data_ptr(), expo.data_ptr(), expo.numel(), 2, stream)       # hipMemcpyDeviceToHost

        def step():
            tick()
            if hip.hipMemcpyAsync(*copy):
                raise RuntimeError("hipMemcpyAsync failed")
            if hip.hipStreamSynchronize(stream):
                raise RuntimeError("hipStreamSynchronize failed")
            if host(*hargs):
                raise RuntimeError("aof_exposure_control_host failed")
        out = timed_bursts(step, lambda: None, K, a.ticks, a.seconds, a.settle)
        updates = float(states["updates"].mean())
    torch.cuda.synchronize()
    r = aof.ticks_view(recs[K - 1])
    assert (r["quality"] >= aof.TICK_HELD).all() and (r["frame"] > a.ticks).all(), "the timed rounds were real ticks"
    eng.close()
    return out[0], out[1], updates


def exposure_sweep(a, dev):
    print("# legs: T camera push alone (pipelined), C camera push + aof_bank_exposure_control_device (pipelined), H camera push + "
          "async D2H copy of the exposure records into pinned memory + stream synchronise + aof_exposure_control_host")
    print("# us = microseconds per step (a camera tick, or a camera burst of K rounds) of 320x240 -> 64x64 streams; T and C: host "
          "clock around chunks of steps ending in a synchronise; H: every step ends with the host holding the commands; "
          "upd = controller steps per stream when the leg ended")
    p, sensor = params_of("px4-64"), (320, 240)
    cases = [(K, S) for K in (1, 5) for S in (int(s) for s in a.streams.split(","))]
    results, upd = {}, {}
    for rep in range(a.repeats):
        for K, S in cases:
            inp = BurstInputs(p, S, K, dev, sensor=sensor)
            for leg in ("T", "C", "H"):
                sec, n, u = leg_exposure(p, S, K, leg, inp, dev, a, sensor)
                results.setdefault((K, S, leg), []).append(sec)
                upd[(K, S, leg)] = u
                print(f"rep {rep} px4-64 K={K:2d} S={S:6d} {leg} {sec * 1e6:10.2f} us  ({n} rounds, upd {u:7.1f})", flush=True)
            del inp
            torch.cuda.empty_cache()
    print("# ---- summary (mean of the repeats; spread = |difference of the repeats| / mean) ----")
    for K, S in cases:
        m = {leg: float(np.mean(results[(K, S, leg)])) for leg in "TCH"}
        sp = {leg: abs(results[(K, S, leg)][0] - results[(K, S, leg)][-1]) / m[leg] for leg in "TCH"}
        gain = (m["H"] - m["C"]) / m["H"]
        print(f"px4-64 K={K:2d} S={S:6d}  " + "  ".join(f"{leg} {m[leg] * 1e6:9.2f} (+-{sp[leg] * 100:4.1f} %)" for leg in "TCH") +
              f"  C-T {(m['C'] - m['T']) * 1e6:7.2f} us  C below H by {gain * 100:5.1f} % "
              f"({'more' if gain > sp['C'] + sp['H'] else 'NOT more'} than the legs' spread)  H/C {m['H'] / m['C']:5.2f}")


IMU_SAMPLES = 4      # HIGHRES_IMU samples per stream and frame round

# Leg G's host: what a caller of the push with d_gyro runs per step -- the reference's integrator
# (mainloop.cpp:383-405) over [K][M][S] samples, the round's sums written as aof_gyro [K][S] -- as one plain C loop,
# compiled when the sweep starts.  The sample times advance by step_us in the same pass.
HOST_LOOP_C = r"""
#include <math.h>
#include <stddef.h>
#include <stdint.h>
typedef struct { uint64_t t; float x, y, z; uint32_t r; } sample;
typedef struct { float x, y, z, dt_s; } gyro;
void integrate(sample *m, int K, int M, int S, uint64_t *prev, uint64_t step_us, gyro *out)
{
    for (int k = 0; k < K; k++)
        for (int s = 0; s < S; s++) {
            double gx = 0.0, gy = 0.0, gz = 0.0;
            for (int j = 0; j < M; j++) {
                sample *p = m + ((size_t)k * M + j) * S + s;
                p->t += step_us;
                const double dt = (double)(uint64_t)(p->t - prev[s]) / 1e6;
                if (prev[s] != 0 && dt < 0.05 && fabsf(p->x) < 20.0 && fabsf(p->y) < 20.0 && fabsf(p->z) < 20.0) {
                    gx += (double)p->x * dt; gy += (double)p->y * dt; gz += (double)p->z * dt;
                }
                prev[s] = p->t;
            }
            gyro *g = out + (size_t)k * S + s;
            g->x = (float)gx; g->y = (float)gy; g->z = (float)gz; g->dt_s = 0.013333f;
        }
}
"""
_host_loop = []


def host_loop():
    """The compiled HOST_LOOP_C (cc -O2, once per process)."""
    if not _host_loop:
        import subprocess
        import tempfile
        tmp = tempfile.mkdtemp(prefix="bench_bank_imu_")
        src, lib = os.path.join(tmp, "host_loop.c"), os.path.join(tmp, "host_loop.so")
        with open(src, "w") as f:
            f.write(HOST_LOOP_C)
        subprocess.run(["cc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", lib, "-lm"], check=True)
        fn = C.CDLL(lib).integrate
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
        fn.restype = None
        _host_loop.append(fn)
    return _host_loop[0]


def leg_imu(p, S, K, leg, inp, dev, a):
    """G: the host integrates the samples in a plain C loop that writes aof_gyro [K][S] (host_loop), copies them to the
    device and pushes with frames -- the way without the IMU call.  D: the samples are copied to the device, the push
    leaves records only, aof_bank_imu_device completes them.  Both advance the sample times in pinned memory per step (G
    inside its loop, D with one numpy add).  Returns (seconds per step, rounds timed)."""
    eng = aof.FlowEngine(p, 0)
    hip = hip_runtime()
    M = IMU_SAMPLES
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000 if leg == "G" else 0, 1, 100, 0)
    bank = eng.bank_create(bp, dev)
    recs = torch.empty((K, S, 48), dtype=torch.uint8, device=dev)
    wire = torch.empty((K, S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty((K, S), dtype=torch.uint8, device=dev)
    times = inp.times0.clone()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctx, burst = eng._ctx, aof.bank_burst_params(K)
    h_samples = torch.empty((K, M, S, 24), dtype=torch.uint8, pin_memory=True)
    samples = h_samples.numpy().view(aof.IMU_SAMPLE_DTYPE).reshape(K, M, S)
    step_us = 13333 * K
    # 300 Hz gyro samples that run on from step to step
    samples["time_usec"] = (1_000_000 + (np.arange(K)[:, None, None] * M + np.arange(M)[None, :, None]) * (13333 // M)).astype(np.uint64)
    samples["xgyro"], samples["ygyro"], samples["zgyro"], samples["reserved"] = 0.01, -0.02, 0.005, 0
    sample_times = samples["time_usec"]
    ip = aof.imu_params(S, K, M)
    # (the pinned blocks are rewritten while an earlier step's copy may still be in flight: a real host would
    # double-buffer; the bytes moved and the work done are the same)
    if leg == "G":
        gyro = torch.zeros((K, S, 4), dtype=torch.float32, device=dev)
        h_gyro = torch.zeros((K, S, 4), dtype=torch.float32, pin_memory=True)
        prev = np.zeros(S, np.uint64)
        integrate = host_loop()
        hargs = (h_samples.data_ptr(), K, M, S, prev.ctypes.data, step_us, h_gyro.data_ptr())
        copy = (gyro.data_ptr(), h_gyro.data_ptr(), gyro.numel() * 4, 1, stream)             # hipMemcpyHostToDevice
        tail = (inp.frames.data_ptr(), times.data_ptr(), None, gyro.data_ptr(), bank.buffer.data_ptr(), bank.buffer.numel(),
                recs.data_ptr(), wire.data_ptr(), lens.data_ptr(), stream)
    else:
        d_samples = torch.empty((K, M, S, 24), dtype=torch.uint8, device=dev)
        state = torch.zeros((S, 64), dtype=torch.uint8, device=dev)
        eng.bank_imu_reset(state, offset0=5_000_000)
        copy = (d_samples.data_ptr(), h_samples.data_ptr(), d_samples.numel(), 1, stream)
        imu = aof.lib.aof_bank_imu_device
        iargs = (ctx, C.byref(ip), d_samples.data_ptr(), None, times.data_ptr(), recs.data_ptr(), state.data_ptr(), recs.data_ptr(),
                 wire.data_ptr(), lens.data_ptr(), stream)
        tail = (inp.frames.data_ptr(), times.data_ptr(), None, None, bank.buffer.data_ptr(), bank.buffer.numel(),
                recs.data_ptr(), None, None, stream)
    if K == 1:
        push, head = aof.lib.aof_bank_push_device, (ctx, C.byref(bp))
    else:
        push, head = aof.lib.aof_bank_push_burst_device, (ctx, C.byref(bp), C.byref(burst))

    def step():
        times.add_(step_us)
        if leg == "G":
            integrate(*hargs)
        else:
            np.add(sample_times, step_us, out=sample_times)
        if hip.hipMemcpyAsync(*copy):
            raise RuntimeError("hipMemcpyAsync failed")
        rc = push(*head, *tail)
        if rc == 0 and leg == "D":
            rc = imu(*iargs)
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
    out_t = timed_bursts(step, torch.cuda.synchronize, K, a.ticks, a.seconds, a.settle)
    torch.cuda.synchronize()
    r = aof.ticks_view(recs[K - 1])
    assert (r["frame"] > a.ticks).all(), "the timed rounds were real ticks"
    if leg == "G":
        assert (h_gyro.numpy()[..., 0] > 0).all(), "the host loop integrated"
    else:
        assert (aof.imu_states_view(state)["samples_integrated"] > 0).all(), "the device integrated"
    eng.close()
    return out_t[0], out_t[1]


def imu_sweep(a, dev):
    print("# legs: G host loop over the samples (a plain C loop that writes aof_gyro [K][S]) + H2D copy of aof_gyro [K][S] + push with frames "
          "(the way without the IMU call), D H2D copy of the samples + records-only push + aof_bank_imu_device")
    print(f"# us = microseconds per step (a tick, or a burst of K rounds) of 64x64 streams, {IMU_SAMPLES} samples per stream and round; "
          "host clock around chunks of steps ending in a synchronise")
    p = params_of("px4-64")
    cases = [(K, S) for K in (1, 5) for S in (int(s) for s in a.streams.split(","))]
    results = {}
    for rep in range(a.repeats):
        for K, S in cases:
            inp = BurstInputs(p, S, K, dev)
            for leg in ("G", "D"):
                sec, n = leg_imu(p, S, K, leg, inp, dev, a)
                results.setdefault((K, S, leg), []).append(sec)
                print(f"rep {rep} px4-64 K={K:2d} S={S:6d} {leg} {sec * 1e6:10.2f} us  ({n} rounds)", flush=True)
            del inp
            torch.cuda.empty_cache()
    print("# ---- summary (mean of the repeats; spread = |difference of the repeats| / mean) ----")
    for K, S in cases:
        m = {leg: float(np.mean(results[(K, S, leg)])) for leg in "GD"}
        sp = {leg: abs(results[(K, S, leg)][0] - results[(K, S, leg)][-1]) / m[leg] for leg in "GD"}
        gain = (m["G"] - m["D"]) / m["G"]
        clear = abs(gain) > sp["G"] + sp["D"]
        print(f"px4-64 K={K:2d} S={S:6d}  " + "  ".join(f"{leg} {m[leg] * 1e6:9.2f} (+-{sp[leg] * 100:4.1f} %)" for leg in "GD") +
              f"  G/D {m['G'] / m['D']:5.2f}  {'D' if gain > 0 else 'G'} wins by {abs(gain) * 100:5.1f} % "
              f"({'more' if clear else 'NOT more'} than the legs' spread)")


RX_FRAMES = 4        # HIGHRES_IMU frames per stream and tick
RX_RING = 8          # ticks of received bytes resident in pinned memory: the timed loop cycles through them


def _crc_x25(data, crc=0xFFFF):
    for b in data:
        tmp = (b ^ crc) & 0xFF
        tmp = (tmp ^ (tmp << 4)) & 0xFF
        crc = ((crc >> 8) ^ (tmp << 8) ^ (tmp << 3) ^ (tmp >> 4)) & 0xFFFF
    return crc


def _mavlink2(msgid, payload, seq, extra):
    body = bytes([len(payload), 0, 0, seq & 255, 1, 1, msgid & 255, (msgid >> 8) & 255, msgid >> 16]) + payload
    crc = _crc_x25(body + bytes([extra]))
    return b"\xfd" + body + bytes([crc & 255, crc >> 8])


def rx_traffic(mix, S):
    """RX_RING ticks of what S autopilots send per tick: mix "imu": RX_FRAMES HIGHRES_IMU frames (MAVLink 2, 74 bytes
    each); mix "mixed": the same frames spread through about 1 KB of frames of other messages.  POOL distinct streams
    (stream s shows pool[s % POOL]: the frames' order is rotated, so neighbouring lanes are in different places).
    Returns (B, [RX_RING] arrays uint8 [S, B], [RX_RING] arrays uint16 [S])."""
    import struct
    rng = np.random.default_rng(77)
    blob = lambda n: rng.integers(0, 250, n, dtype=np.uint8).tobytes()
    ticks = []
    for k in range(RX_RING):
        pool = []
        for v in range(POOL):
            imu = [_mavlink2(105, struct.pack("<Q13fH", 1_000_000 + ((k * RX_FRAMES + j) * 13333) // RX_FRAMES, 0.1, 0.2, 9.8,
                                              0.01, -0.02, 0.005, 0.3, 0.1, 0.4, 1013.0, 0.0, 120.0, 25.0, 0x1FFF), k * RX_FRAMES + j, 93)
                   for j in range(RX_FRAMES)]
            other = []
            if mix == "mixed":
                other = ([_mavlink2(30, blob(28), i, 39) for i in range(10)] + [_mavlink2(33, blob(28), i, 104) for i in range(4)] +
                         [_mavlink2(24, blob(30), i, 24) for i in range(3)] + [_mavlink2(253, blob(51), 0, 83)])
            n_other = len(other) // RX_FRAMES
            parts = []
            for j in range(RX_FRAMES):
                parts += [imu[j]] + other[j * n_other:(j + 1) * n_other]
            parts += other[RX_FRAMES * n_other:]
            r = v % len(parts)
            pool.append(b"".join(parts[r:] + parts[:r]))
        ticks.append(pool)
    longest = max(len(b) for pool in ticks for b in pool)
    B = (longest + 15) // 16 * 16
    data, lens = [], []
    for pool in ticks:
        a = np.zeros((POOL, B), np.uint8)
        for v, b in enumerate(pool):
            a[v, :len(b)] = np.frombuffer(b, np.uint8)
        idx = np.arange(S) % POOL
        data.append(a[idx])
        lens.append(np.array([len(pool[v]) for v in idx], np.uint16))
    return B, data, lens


def leg_mavlink_rx(p, S, mix, leg, inp, dev, a):
    """One tick per step.  H: aof_bank_mavlink_rx_host over the S slots of the tick's pinned receive block, one copy of
    the samples (and their counts) to the device, the records-only push, the IMU call.  D: one copy of the receive
    block (bytes and lengths), aof_bank_mavlink_rx_device, the same push and IMU call.  The receive blocks are RX_RING
    pinned blocks the loop cycles through (the frames' times run backwards at the ring's wrap: one rejected sample per
    stream and wrap, on both legs).  Returns (seconds per step, ticks timed, B)."""
    eng = aof.FlowEngine(p, 0)
    hip = hip_runtime()
    M = IMU_SAMPLES
    B, data, lens = rx_traffic(mix, S)
    bp = aof.bank_params(S, FX, FY, 15, 0, 1, 100, 0)
    bank = eng.bank_create(bp, dev)
    recs = torch.empty((1, S, 48), dtype=torch.uint8, device=dev)
    wire = torch.empty((1, S, 56), dtype=torch.uint8, device=dev)
    lens_out = torch.empty((1, S), dtype=torch.uint8, device=dev)
    times = inp.times0.clone()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctx = eng._ctx
    block = S * B + 2 * S                                    # bytes [S][B], then u16 [S]
    ring = [torch.empty(block, dtype=torch.uint8, pin_memory=True) for _ in range(RX_RING)]
    for k in range(RX_RING):
        ring[k].numpy()[:S * B] = data[k].ravel()
        ring[k].numpy()[S * B:] = lens[k].view(np.uint8)
    sample_bytes = 24 * M * S
    d_samples = torch.zeros(sample_bytes + S, dtype=torch.uint8, device=dev)      # aof_imu_sample [M][S], then u8 [S]
    imu_state = torch.zeros((S, 64), dtype=torch.uint8, device=dev)
    eng.bank_imu_reset(imu_state, offset0=5_000_000)
    rp, ip = aof.mavlink_rx_params(S, 1, B, M), aof.imu_params(S, 1, M)
    imu = aof.lib.aof_bank_imu_device
    iargs = (ctx, C.byref(ip), d_samples.data_ptr(), d_samples.data_ptr() + sample_bytes, times.data_ptr(), recs.data_ptr(),
             imu_state.data_ptr(), recs.data_ptr(), wire.data_ptr(), lens_out.data_ptr(), stream)
    pargs = (ctx, C.byref(bp), inp.frames.data_ptr(), times.data_ptr(), None, None, bank.buffer.data_ptr(), bank.buffer.numel(),
             recs.data_ptr(), None, None, stream)
    push = aof.lib.aof_bank_push_device
    if leg == "H":
        h_samples = torch.zeros(sample_bytes + S, dtype=torch.uint8, pin_memory=True)
        states = np.zeros(S, aof.MAVLINK_RX_STATE_DTYPE)
        parse = aof.lib.aof_bank_mavlink_rx_host
        hargs = [(C.byref(rp), r.data_ptr(), r.data_ptr() + S * B, states.ctypes.data, h_samples.data_ptr(),
                  h_samples.data_ptr() + sample_bytes) for r in ring]
        copy = (d_samples.data_ptr(), h_samples.data_ptr(), sample_bytes + S, 1, stream)       # hipMemcpyHostToDevice
    else:
        d_block = torch.zeros(block, dtype=torch.uint8, device=dev)
        rx_state = torch.zeros((S, 128), dtype=torch.uint8, device=dev)
        eng.bank_mavlink_rx_reset(rx_state)
        rx = aof.lib.aof_bank_mavlink_rx_device
        rargs = (ctx, C.byref(rp), d_block.data_ptr(), d_block.data_ptr() + S * B, rx_state.data_ptr(), d_samples.data_ptr(),
                 d_samples.data_ptr() + sample_bytes, stream)
        copies = [(d_block.data_ptr(), r.data_ptr(), block, 1, stream) for r in ring]
    count = [0]

    def step():
        i = count[0] % RX_RING
        count[0] += 1
        times.add_(13333)
        if leg == "H":
            rc = parse(*hargs[i])
            if rc == 0 and hip.hipMemcpyAsync(*copy):
                raise RuntimeError("hipMemcpyAsync failed")
        else:
            if hip.hipMemcpyAsync(*copies[i]):
                raise RuntimeError("hipMemcpyAsync failed")
            rc = rx(*rargs)
        if rc == 0:
            rc = push(*pargs)
        if rc == 0:
            rc = imu(*iargs)
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
    out_t = timed_bursts(step, torch.cuda.synchronize, 1, a.ticks, a.seconds, a.settle)
    torch.cuda.synchronize()
    assert (aof.ticks_view(recs[0])["frame"] > a.ticks).all(), "the timed rounds were real ticks"
    st = states if leg == "H" else aof.mavlink_rx_states_view(rx_state)
    assert (st["imu_samples"] == RX_FRAMES * count[0]).all() and (st["bad_check"] == 0).all() and (st["overflowed"] == 0).all(), \
        "every HIGHRES_IMU frame was decoded"
    assert (aof.imu_states_view(imu_state)["samples_integrated"] > count[0]).all(), "the IMU call integrated them"
    eng.close()
    return out_t[0], out_t[1], B


def mavlink_rx_sweep(a, dev):
    print("# legs: H aof_bank_mavlink_rx_host over the S slots + H2D copy of the samples and counts + records-only push + "
          "aof_bank_imu_device, D H2D copy of the bytes and lengths + aof_bank_mavlink_rx_device + the same push and IMU call")
    print(f"# us = microseconds per tick of 64x64 streams; mixes: imu = {RX_FRAMES} HIGHRES_IMU frames per stream and tick, mixed = the "
          "same frames inside about 1 KB of other frames; host clock around chunks of ticks ending in a synchronise")
    p = params_of("px4-64")
    cases = [(mix, S) for mix in ("imu", "mixed") for S in (int(s) for s in a.streams.split(","))]
    results, slot = {}, {}
    for rep in range(a.repeats):
        for mix, S in cases:
            inp = BurstInputs(p, S, 1, dev)
            for leg in ("H", "D"):
                sec, n, B = leg_mavlink_rx(p, S, mix, leg, inp, dev, a)
                results.setdefault((mix, S, leg), []).append(sec)
                slot[mix] = B
                print(f"rep {rep} px4-64 {mix:5s} B={B:5d} S={S:6d} {leg} {sec * 1e6:10.2f} us  ({n} ticks)", flush=True)
            del inp
            torch.cuda.empty_cache()
    print("# ---- summary (mean of the repeats; spread = |difference of the repeats| / mean) ----")
    for mix, S in cases:
        m = {leg: float(np.mean(results[(mix, S, leg)])) for leg in "HD"}
        sp = {leg: abs(results[(mix, S, leg)][0] - results[(mix, S, leg)][-1]) / m[leg] for leg in "HD"}
        gain = (m["H"] - m["D"]) / m["H"]
        clear = abs(gain) > sp["H"] + sp["D"]
        print(f"px4-64 {mix:5s} B={slot[mix]:5d} S={S:6d}  " + "  ".join(f"{leg} {m[leg] * 1e6:9.2f} (+-{sp[leg] * 100:4.1f} %)" for leg in "HD") +
              f"  H/D {m['H'] / m['D']:5.2f}  {'D' if gain > 0 else 'H'} wins by {abs(gain) * 100:5.1f} % "
              f"({'more' if clear else 'NOT more'} than the legs' spread)")


def leg_contexts(p, S, inp, a):
    engs = [aof.FlowEngine(p, 0) for _ in range(S)]
    flow = np.zeros(1, aof.FLOW_DTYPE)
    frames = [[np.ascontiguousarray(inp.host[s % POOL, k]) for s in range(S)] for k in range(RING)]
    fn = aof.lib.aof_stream_push_host
    ctxs = [e._ctx for e in engs]
    ptrs = [[f.ctypes.data for f in tick] for tick in frames]
    out_ptr = flow.ctypes.data

    def step(i):
        row = ptrs[i % RING]
        for s in range(S):
            if fn(ctxs[s], row[s], out_ptr) < 0:
                raise aof.AofError(-5, aof.lib.aof_last_error(ctxs[s]).decode())
    out = timed(step, lambda: None, a.ticks, a.seconds, a.settle)   # (every call is synchronous)
    for e in engs:
        e.close()
    return out


def leg_batch(p, S, inp, dev, a):
    eng = aof.FlowEngine(p, 0)
    nb = eng.nblocks(0)
    blocks = torch.empty((S, nb), dtype=torch.int32, device=dev)
    flows = torch.empty((S, 16), dtype=torch.uint8, device=dev)
    subdirs = torch.empty((S, nb), dtype=torch.uint8, device=dev) if p.subpixel else None
    ws = torch.empty(aof.workspace_layout(p, S).total_bytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    calls = [eng.bind_batch(inp.frames[k], inp.frames[k + 1], blocks, flows, ws, subdirs=subdirs, stream=stream) for k in range(RING)]
    out = timed(lambda i: calls[i % RING](), torch.cuda.synchronize, a.ticks, a.seconds, a.settle)
    eng.close()
    return out


def class_marker(dev):
    """K2 of the exhaustive C2 search (1 024 VGA pairs) on this GPU: the figure profiles/README.md tells boxes apart by."""
    p = aof.default_params(640, 480)
    base = [synth.make_pair(640, 480, reach=4, pair_index=k) for k in range(8)]
    tp = torch.from_numpy(np.stack([b[0] for b in base])).to(dev).repeat(128, 1, 1).contiguous()
    tc = torch.from_numpy(np.stack([b[1] for b in base])).to(dev).repeat(128, 1, 1).contiguous()
    eng = aof.FlowEngine(p, 0)
    eng.set_search_mode(aof.SEARCH_EXHAUSTIVE)
    for _ in range(20):
        eng.flow_batch(tp, tc)
    torch.cuda.synchronize()
    eng.set_profiling(True, kernels=[aof.K_SEARCH])
    for _ in range(50):
        eng.flow_batch(tp, tc)
    torch.cuda.synchronize()
    ms = float(np.median(eng.profile_ms(aof.K_SEARCH)))
    eng.close()
    return ms


def per_stream_sweep(a, dev):
    print("# legs: U1/U2 plain tick on the scalars of aof_bank_params on path 1/2, P1/P2 the same tick with S distinct aof_bank_stream "
          "records bound (MAVLink frames on, all streams active, gyro)")
    print("# us = microseconds per tick (host clock, ticks ending in a synchronise)")
    bound = hasattr(aof.lib, "aof_set_bank_streams")      # (AOF_LIB may name a build without the call: U legs only)
    legs = [("U1", 1, False), ("U2", 2, False)] + ([("P1", 1, True), ("P2", 2, True)] if bound else [])
    sizes = [int(s) for s in a.streams.split(",")]
    results = {}
    for rep in range(a.repeats):
        for cfg in a.configs.split(","):
            p = params_of(cfg)
            for S in sizes:
                inp = Inputs(p, S, dev)
                for name, path, per_stream in legs:
                    sec, n = leg_tick(p, S, path, inp, dev, a, per_stream)
                    results.setdefault((cfg, S, name), []).append(sec)
                    print(f"rep {rep} {cfg:11s} S={S:6d} {name:2s} {sec * 1e6:10.2f} us  ({n} ticks)", flush=True)
                del inp
                torch.cuda.empty_cache()
    print("# ---- summary (mean of the repeats; spread = |difference of the repeats| / mean) ----")
    for cfg in a.configs.split(","):
        for S in sizes:
            m = {n: float(np.mean(results[(cfg, S, n)])) for n, _, _ in legs}
            sp = {n: abs(results[(cfg, S, n)][0] - results[(cfg, S, n)][-1]) / m[n] for n in m}
            line = f"{cfg:11s} S={S:6d}  " + "  ".join(f"{n} {m[n] * 1e6:9.2f} us (+-{sp[n] * 100:4.1f} %)" for n in m)
            if bound:
                line += f"  P1/U1 {m['P1'] / m['U1']:5.3f}  P2/U2 {m['P2'] / m['U2']:5.3f}"
            print(line)


def leg_field(p, S, path, inp, dev, a, kind):
    """One of T / F / H of --field on `path`: the plain tick, alone, with the field call behind it, or with the copies, the
    synchronise and the host function behind it."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bank_field_rig as rig
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    bp = aof.bank_params(S, FX, FY, 15, 5_000_000, 1, 100, 0)
    bank = eng.bank_create(bp, dev)
    recs = torch.empty((S, 48), dtype=torch.uint8, device=dev)
    wire = torch.empty((S, 56), dtype=torch.uint8, device=dev)
    lens = torch.empty(S, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn, ctx, bpp = aof.lib.aof_bank_push_device, eng._ctx, C.byref(bp)
    calls = [(inp.frames[k].data_ptr(), inp.times[k].data_ptr()) for k in range(RING)]
    rest = (None, inp.gyro.data_ptr(), bank.buffer.data_ptr(), bank.buffer.numel(), recs.data_ptr(), wire.data_ptr(), lens.data_ptr(), stream)
    sync = torch.cuda.synchronize
    after = None
    if kind != "T":
        lib = rig.bind(aof)
        fp = aof.field_params()
        fpp = C.byref(fp)
        nb = eng.nblocks(0)
        out = torch.empty((S, 48), dtype=torch.uint8, device=dev)
        fields = torch.empty((S, 64), dtype=torch.uint8, device=dev)
    if kind == "F":
        state = torch.zeros((S, 64), dtype=torch.uint8, device=dev)
        assert rig.reset(aof, eng, state) == 0
        tail = (bank.buffer.data_ptr(), bank.buffer.numel(), recs.data_ptr(), state.data_ptr(), fields.data_ptr(), out.data_ptr(), stream)

        def after():
            return lib.aof_bank_field_device(ctx, bpp, fpp, *tail)
    if kind == "H":
        at_b, at_s = rig.scratch_offsets(aof, p, bank.layout, S)
        d_blocks, d_sub = bank.buffer[at_b:at_b + 4 * S * nb], bank.buffer[at_s:at_s + S * nb]
        h_blocks = torch.empty(4 * S * nb, dtype=torch.uint8).pin_memory()
        h_sub = torch.empty(S * nb, dtype=torch.uint8).pin_memory()
        h_recs = torch.empty((S, 48), dtype=torch.uint8).pin_memory()
        h_state = np.zeros(S, rig.STATE_DTYPE)
        h_out, h_fields = np.zeros(S, rig.RECORD_DTYPE), np.zeros(S, aof.FIELD_DTYPE)
        pp = C.byref(p)
        host = (h_blocks.data_ptr(), h_sub.data_ptr() if p.subpixel else None, h_recs.data_ptr(), h_state.ctypes.data, h_fields.ctypes.data,
                h_out.ctypes.data)

        def after():
            h_blocks.copy_(d_blocks, non_blocking=True)
            if p.subpixel:
                h_sub.copy_(d_sub, non_blocking=True)
            h_recs.copy_(recs, non_blocking=True)
            sync()
            return lib.aof_bank_field_host(pp, bpp, None, fpp, *host)

    def step(i):
        f, t = calls[i % RING]
        rc = fn(ctx, bpp, f, t, *rest)
        if not rc and after is not None:
            rc = after()
        if rc:
            raise aof.AofError(rc, aof.lib.aof_last_error(ctx).decode())
    res = timed(step, sync, a.ticks, a.seconds, a.settle)
    r = aof.ticks_view(recs)
    assert (r["quality"] >= aof.TICK_HELD).all() and (r["frame"] > a.ticks).all(), "the timed ticks were real ticks"
    if kind == "F":
        o = out.cpu().numpy().reshape(-1).view(rig.RECORD_DTYPE)
        assert (o["frame"] == r["frame"]).all() and (np.frombuffer(state.cpu().numpy(), rig.STATE_DTYPE)["published"] > 0).all(), "the field call ran behind every tick"
    if path and hasattr(aof.lib, "aof_bank_last_path"):
        assert eng.last_bank_path() == path, (kind, "timed path", eng.last_bank_path(), "meant", path)
    eng.close()
    return res


def field_sweep(a, dev):
    print("# legs (the digit: bank path 1 / 2): T the plain tick alone; F tick + aof_bank_field_device, pipelined; H tick + copies of block "
          "records, sub-directions and tick records to pinned memory + synchronise + aof_bank_field_host (MAVLink frames on, all streams active, gyro)")
    print("# us = microseconds per tick (host clock; T and F: ticks ending in a synchronise every 256; H: every tick ends with the host holding the records)")
    bound = hasattr(aof.lib, "aof_bank_field_device")      # (AOF_LIB may name a build without the call: T legs only)
    kinds = ["T", "F", "H"] if bound else ["T"]
    legs = [(k + str(path), k, path) for path in (1, 2) for k in kinds]
    if a.legs is not None:
        legs = [leg for leg in legs if leg[0] in a.legs.split(",")]
    sizes = [int(s) for s in a.streams.split(",")]
    results = {}
    for rep in range(a.repeats):
        for cfg in a.configs.split(","):
            p = params_of(cfg)
            for S in sizes:
                inp = Inputs(p, S, dev)
                for name, kind, path in legs:
                    sec, n = leg_field(p, S, path, inp, dev, a, kind)
                    results.setdefault((cfg, S, name), []).append(sec)
                    print(f"rep {rep} {cfg:11s} S={S:6d} {name:3s} {sec * 1e6:10.2f} us  ({n} ticks)", flush=True)
                del inp
                torch.cuda.empty_cache()
    print("# ---- summary (median of the repeats; p10..p90 of the repeats in us) ----")
    for cfg in a.configs.split(","):
        for S in sizes:
            m = {n: float(np.median(results[(cfg, S, n)])) for n, _, _ in legs}
            line = f"{cfg:11s} S={S:6d}  " + "  ".join(
                f"{n} {m[n] * 1e6:9.2f} us ({np.percentile(results[(cfg, S, n)], 10) * 1e6:.2f}..{np.percentile(results[(cfg, S, n)], 90) * 1e6:.2f})"
                for n in m)
            for path in (1, 2):
                if all(k + str(path) in m for k in ("T", "F", "H")):
                    t, f, h = (m[k + str(path)] for k in ("T", "F", "H"))
                    line += f"  F{path}-T{path} {(f - t) * 1e6:6.2f} us  F{path}/T{path} {f / t:5.3f}  F{path}/H{path} {f / h:5.3f}"
            print(line)


def per_sensor_sweep(a, dev):
    print("# legs: K1/K2 camera tick on the scalars of aof_bank_camera on path 1/2, S1/S2 the same tick with S aof_bank_sensor "
          "records equal to aof_bank_sensor_from_camera bound (exposure records, de-rotation, MAVLink frames on, all streams active)")
    print("# us = microseconds per tick (host clock, ticks ending in a synchronise)")
    bound = hasattr(aof.lib, "aof_set_bank_sensors")      # (AOF_LIB may name a build without the call: K legs only)
    legs = [("K1", 1, False), ("K2", 2, False)] + ([("S1", 1, True), ("S2", 2, True)] if bound else [])
    if a.legs is not None:                                # (--legs K1,K2: the same legs from two builds, alternating)
        legs = [leg for leg in legs if leg[0] in a.legs.split(",")]
        bound = bound and len(legs) == 4
    sizes = [int(s) for s in a.streams.split(",")]
    results = {}
    for rep in range(a.repeats):
        for cfg in a.configs.split(","):
            p = params_of(cfg)
            cam_w, cam_h = SENSOR[cfg]
            for S in sizes:
                inp = Inputs(p, S, dev)
                cams = sensor_frames(p, S, inp, dev, cam_w, cam_h)
                for name, path, per_sensor in legs:
                    sec, n = leg_camera(p, S, path, inp, cams, dev, a, cam_w, cam_h, per_sensor)
                    results.setdefault((cfg, S, name), []).append(sec)
                    print(f"rep {rep} {cfg:11s} S={S:6d} {name:2s} {sec * 1e6:10.2f} us  ({n} ticks)", flush=True)
                del inp, cams
                torch.cuda.empty_cache()
    print("# ---- summary (median of the repeats; spread = (max - min) of the repeats / median) ----")
    for cfg in a.configs.split(","):
        for S in sizes:
            m = {n: float(np.median(results[(cfg, S, n)])) for n, _, _ in legs}
            sp = {n: (max(results[(cfg, S, n)]) - min(results[(cfg, S, n)])) / m[n] for n in m}
            line = f"{cfg:11s} S={S:6d}  " + "  ".join(f"{n} {m[n] * 1e6:9.2f} us (+-{sp[n] * 100:4.1f} %)" for n in m)
            if bound:
                line += f"  S1/K1 {m['S1'] / m['K1']:5.3f}  S2/K2 {m['S2'] / m['K2']:5.3f}"
            print(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", default="1,16,64,128,256,1024,4096,16384")
    ap.add_argument("--configs", default="px4-64,opencv-128")
    ap.add_argument("--ticks", type=int, default=2000, help="timed ticks per leg, at least")
    ap.add_argument("--seconds", type=float, default=0.5, help="timed seconds per leg, at least")
    ap.add_argument("--settle", type=float, default=0.2, help="untimed seconds in front of every leg")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--contexts-max", type=int, default=64, help="largest S of the B leg")
    ap.add_argument("--legs", default=None, help="legs to run (a kernel trace wants one at a time); default: T0,T1,T2,C,B, with "
                    "--per-sensor K1,K2,S1,S2")
    ap.add_argument("--no-marker", action="store_true")
    ap.add_argument("--camera", action="store_true", help="the sweep of the tick on raw sensor frames (legs K0, K1, K2, Y, T0)")
    ap.add_argument("--burst", default="", help="K[,K...]: the sweep of bursts of K rounds against K single ticks (legs B0-B2, T0-T2)")
    ap.add_argument("--outbox", action="store_true", help="the sweep of the outbox: legs T, D, H, O")
    ap.add_argument("--exposure-control", action="store_true", help="the sweep of the auto-exposure controller: legs T, C, H")
    ap.add_argument("--imu", action="store_true", help="the sweep of the IMU call: legs G, D")
    ap.add_argument("--mavlink-rx", action="store_true", help="the sweep of the MAVLink receive: legs H, D on two traffic mixes")
    ap.add_argument("--per-stream", action="store_true", help="the plain tick with per-stream records bound against the unbound tick: legs U1, U2, P1, P2")
    ap.add_argument("--per-sensor", action="store_true", help="the camera tick with per-stream sensor records bound against the unbound camera tick: legs K1, K2, S1, S2 "
                    "(K1 / K2 are --camera's legs of those names, the same leg_camera; --legs K1,K2 runs them alone, for two builds in turn)")
    ap.add_argument("--pixel-formats", action="store_true", help="the camera tick with packed 16-bit sensor pixels: legs G, P0, Y, M, D on both "
                    "bank paths (G1, ..., D2; --legs G1,G2 runs the yardstick alone, for a build without the call through AOF_LIB)")
    ap.add_argument("--binning", action="store_true", help="the camera tick with binned sensor pixels: legs G, B0, B2, B4, Y4, D2, D4 on both "
                    "bank paths (G1, ..., D42; --legs G1,G2 runs the yardstick alone, for a build without the call through AOF_LIB)")
    ap.add_argument("--raw-formats", action="store_true", help="the camera tick with raw mono pixels: legs G, R, P, M, D on both bank "
                    "paths (G1, ..., D2; --legs G1,G2 runs the yardstick alone, for a build without the formats through AOF_LIB)")
    ap.add_argument("--warp", action="store_true", help="the camera tick with warp meshes bound: legs P, I, L, F, U, W, WI, WB1, WB2 on 640 x 480 frames (--legs P,F "
                    "runs the legs that need no mesh alone, for a build without the call through AOF_LIB)")
    ap.add_argument("--field", action="store_true", help="the motion field behind the plain tick: legs T, F, H on both bank paths (--legs T1,T2 "
                    "runs the tick alone, for a build without the call through AOF_LIB)")
    ap.add_argument("--forms", default="plain,camera", help="--burst: entry points to sweep")
    ap.add_argument("--input-bytes-max", type=float, default=24 * 2**30, help="--burst: sizes whose K rounds of input exceed this are skipped")
    a = ap.parse_args()
    if a.legs is None and not a.per_sensor and not a.pixel_formats and not a.binning and not a.raw_formats and not a.warp and not a.field:
        a.legs = "T0,T1,T2,C,B"
    if a.burst and a.ticks == ap.get_default("ticks"):
        a.ticks = 1000           # (frame rounds)
    if a.camera and a.streams == ap.get_default("streams"):
        a.streams = "1,64,1024,1536,2048,4096"
    if (a.pixel_formats or a.binning or a.raw_formats) and a.streams == ap.get_default("streams"):
        a.streams = "64,256,1024,2048"
    if a.warp and a.streams == ap.get_default("streams"):
        a.streams = "64,256,1024,2048"
    if a.field and a.streams == ap.get_default("streams"):
        a.streams = "64,256,1024,4096"
    if a.exposure_control and a.streams == ap.get_default("streams"):
        a.streams = "64,1024,4096"
    if (a.imu or a.mavlink_rx) and a.streams == ap.get_default("streams"):
        a.streams = "64,256,1024,4096"
    if a.outbox and a.streams == ap.get_default("streams"):
        a.streams = "64,256,1024,4096,16384"
    if not torch.cuda.is_available():
        raise SystemExit("bench_bank.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    print(f"# tools/bench_bank.py {' '.join(sys.argv[1:])}")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    if not a.no_marker:
        print(f"# class marker: exhaustive C2 K2 (1 024 VGA pairs) {class_marker(dev):.4f} ms")
    if a.field:
        return field_sweep(a, dev)
    if a.per_stream:
        return per_stream_sweep(a, dev)
    if a.per_sensor:
        return per_sensor_sweep(a, dev)
    if a.pixel_formats:
        return pixel_formats_sweep(a, dev)
    if a.binning:
        return binning_sweep(a, dev)
    if a.raw_formats:
        return raw_formats_sweep(a, dev)
    if a.warp:
        return warp_sweep(a, dev)
    if a.mavlink_rx:
        return mavlink_rx_sweep(a, dev)
    if a.imu:
        return imu_sweep(a, dev)
    if a.exposure_control:
        return exposure_sweep(a, dev)
    if a.outbox:
        return outbox_sweep(a, dev)
    if a.burst:
        return burst_sweep(a, dev)
    if a.camera:
        return camera_sweep(a, dev)
    print("# legs: T0/T1/T2 bank tick on path 0/1/2 (MAVLink frames on, all streams active), B = S contexts x aof_stream_push_host, "
          "C = aof_flow_batch_device on S pairs")
    print("# us = microseconds per tick (host clock, ticks ending in a synchronise); Mframes/s = stream-frames per second")
    sizes = [int(s) for s in a.streams.split(",")]
    results = {}
    for rep in range(a.repeats):
        for cfg in a.configs.split(","):
            p = params_of(cfg)
            for S in sizes:
                inp = Inputs(p, S, dev)
                legs = [("T0", lambda: leg_tick(p, S, 0, inp, dev, a)), ("T1", lambda: leg_tick(p, S, 1, inp, dev, a)),
                        ("T2", lambda: leg_tick(p, S, 2, inp, dev, a)), ("C", lambda: leg_batch(p, S, inp, dev, a))]
                if S <= a.contexts_max:
                    legs.append(("B", lambda: leg_contexts(p, S, inp, a)))
                for name, fn in legs:
                    if name not in a.legs.split(","):
                        continue
                    sec, n = fn()
                    results.setdefault((cfg, S, name), []).append(sec)
                    print(f"rep {rep} {cfg:11s} S={S:6d} {name:2s} {sec * 1e6:10.2f} us  {1 / sec:12.0f} ticks/s  {S / sec / 1e6:9.3f} Mframes/s  ({n} ticks)", flush=True)
                del inp
                torch.cuda.empty_cache()
    if not all(n in a.legs.split(",") for n in ("T0", "T1", "T2", "C")):
        return
    print("# ---- summary (mean of the repeats; spread = |difference of the repeats| / mean) ----")
    for cfg in a.configs.split(","):
        tb, cb = tick_bytes(params_of(cfg))
        print(f"# {cfg}: bytes per stream and tick {tb}, per stateless pair {cb} (ratio {tb / cb:.2f})")
        for S in sizes:
            m = {n: float(np.mean(results[(cfg, S, n)])) for n in ("T0", "T1", "T2", "C", "B") if (cfg, S, n) in results}
            sp = {n: (abs(results[(cfg, S, n)][0] - results[(cfg, S, n)][-1]) / m[n]) for n in m}
            best = "T1" if m["T1"] <= m["T2"] else "T2"
            line = (f"{cfg:11s} S={S:6d}  T0 {m['T0'] * 1e6:9.2f} us (+-{sp['T0'] * 100:4.1f} %)  T1 {m['T1'] * 1e6:9.2f} (+-{sp['T1'] * 100:4.1f} %)  "
                    f"T2 {m['T2'] * 1e6:9.2f} (+-{sp['T2'] * 100:4.1f} %)  C {m['C'] * 1e6:9.2f} (+-{sp['C'] * 100:4.1f} %)  "
                    f"T0/C {m['T0'] / m['C']:5.2f}  faster path {best}  T0/best {m['T0'] / m[best]:5.3f}  "
                    f"T0 {1 / m['T0']:9.0f} ticks/s {S / m['T0'] / 1e6:8.3f} Mframes/s")
            if "B" in m:
                line += f"  B {m['B'] * 1e6:9.2f} us  B/T0 {m['B'] / m['T0']:6.1f}x"
            print(line)


if __name__ == "__main__":
    main()
