#!/usr/bin/env python3
"""What the sequence pipeline's MAVLink receive costs (aof_sequence_mavlink_rx_device, csrc/k_sequence_mavlink_rx.hip), one GPU,
one process: the connection log of a recording of 65 536 frames at 75 fps -- HIGHRES_IMU at 250 Hz over 874 s as MAVLink 2
frames (the frames of tests/mavlink_rx_ref.frame_v2, built here for all samples at once) with a frame of other traffic behind
every one, about 22 MB --, the device call, the host way, and the chain both ways:
  D      the device call alone, between device events: --inner calls per window, ms per call;
  H      the host way: aof_sequence_mavlink_rx_host on the log in host memory, the samples and sample_end copied up from pinned
         memory, a synchronise; a host clock;
  D+S+I  the chain: the receive, aof_sequence_device (records only) and aof_sequence_imu_device with n_samples = max_samples on
         one stream, a synchronise behind the last;
  H+S+I  the same chain fed from the host: H, then the two calls.
The median of --repeats windows (at least three) after a warm-up, in ms.  One box, one session: a figure, not a gate.  Writes
profiles/sequence_rx_cost.txt (--out)."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge   # noqa: E402
import mavlink_rx_ref as rx   # noqa: E402
import sequence_imu_rig as imu_rig   # noqa: E402
import sequence_rx_rig as rig   # noqa: E402

FX, FY = 216.6677, 216.2457


def x25_rows(rows):
    """mavlink_model.x25 over every row of a uint8 matrix at once."""
    crc = np.full(len(rows), 0xFFFF, np.uint32)
    for col in rows.T.astype(np.uint32):
        tmp = (col ^ crc) & 0xFF
        tmp = (tmp ^ (tmp << 4)) & 0xFF
        crc = ((crc >> 8) ^ (tmp << 8) ^ (tmp << 3) ^ (tmp >> 4)) & 0xFFFF
    return crc


def make_log(rng, T):
    """T HIGHRES_IMU frames (MAVLink 2, 62-byte payload) 4 ms apart with a frame of another message behind each ->
    (log uint8, the position behind each IMU frame's last byte, the sample times)."""
    times = 7_000_000 + 4000 * np.arange(T, dtype=np.uint64)
    payload = np.zeros((T, 62), np.uint8)
    payload[:, 0:8] = times.view(np.uint8).reshape(T, 8)
    payload[:, 8:52] = rng.normal(0, 0.8, (T, 11)).astype(np.float32).view(np.uint8).reshape(T, 44)
    payload[:, 60] = 0xFF                                        # fields_updated: the payload is not truncated
    head = np.zeros((T, 9), np.uint8)
    head[:, 0], head[:, 3], head[:, 4], head[:, 5], head[:, 6] = 62, np.arange(T) & 255, 1, 1, rx.HIGHRES_IMU
    crc = x25_rows(np.concatenate([head, payload, np.full((T, 1), rx.HIGHRES_IMU_EXTRA, np.uint8)], axis=1))
    frames = np.concatenate([np.full((T, 1), 0xFD, np.uint8), head, payload, (crc & 0xFF).astype(np.uint8)[:, None],
                             (crc >> 8).astype(np.uint8)[:, None]], axis=1)
    assert frames[5].tobytes() == rx.frame_v2(rx.HIGHRES_IMU, payload[5].tobytes(), seq=5, truncate=False), "the generator's frame"
    other = [rx.frame_v2(int(rng.choice([0, 30, 33, 74])), rng.integers(0, 256, int(rng.integers(4, 28)), dtype=np.uint8).tobytes(), seq=i)
             if i % 3 else rx.frame_v1(int(rng.choice([0, 1, 24])), rng.integers(0, 256, int(rng.integers(4, 28)), dtype=np.uint8).tobytes(), seq=i)
             for i in range(64)]
    width = frames.shape[1]
    sizes = width + np.array([len(other[i % 64]) for i in range(T)])
    starts = np.concatenate([[0], np.cumsum(sizes)])
    log = np.zeros(int(starts[-1]), np.uint8)
    at = starts[:-1]
    log[(at[:, None] + np.arange(width)[None, :]).reshape(-1)] = frames.reshape(-1)
    for j in range(64):
        o = np.frombuffer(other[j], np.uint8)
        rows = at[j::64] + width
        log[(rows[:, None] + np.arange(len(o))[None, :]).reshape(-1)] = np.tile(o, len(rows))
    return log, at + width, times


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inner", type=int, default=20, help="device calls per timed window of leg D")
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d"), help="a name for this measuring session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_rx_cost.txt"))
    args = ap.parse_args()
    assert args.repeats >= 3, "at least three repeats"
    aof = ge.load_package()   # (raises where the library has not been built)
    synth = importlib.import_module("aero_optical_flow_amd.synth")
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    device = torch.device("cuda:0")
    n, cw, ch, cam_w, cam_h = args.frames, 64, 64, 160, 120

    rng = np.random.default_rng(1)
    times = np.cumsum(np.concatenate([[0], rng.integers(12000, 15000, n - 1)])).astype(np.int64)      # ~75 fps
    T = int(times[-1] // 4000) + 8
    log, delivered, sample_times = make_log(rng, T)
    N, M = len(log), T + 16
    arrival = sample_times.astype(np.int64) - 7_000_000 - 20000                                       # from before frame 0
    byte_end = delivered[np.maximum(np.searchsorted(arrival, times), 1) - 1].astype(np.uint32)

    eng = aof.FlowEngine(aof.px4flow_params(cw, ch), 0)
    d_log = torch.zeros((N + 15) // 16 * 16, dtype=torch.uint8, device=device)
    d_log[:N].copy_(torch.from_numpy(log))
    d_byte_end = rig.up(torch, byte_end, device).view(torch.int32)
    d_samples = torch.zeros((M, 24), dtype=torch.uint8, device=device)
    d_end = torch.zeros(n, dtype=torch.int32, device=device)
    d_state = torch.zeros(128, dtype=torch.uint8, device=device)
    scratch = torch.empty(rig.scratch_bytes(aof, N), dtype=torch.uint8, device=device)
    rp = rig.params(N, M)

    def receive():
        assert rig.device(aof, eng, rp, n, d_log, d_byte_end, d_samples, d_end, d_state, scratch) == 0

    h_samples = torch.zeros((M, 24), dtype=torch.uint8).pin_memory()
    h_end = torch.zeros(n, dtype=torch.int32).pin_memory()
    h_state = np.zeros(128, np.uint8)

    def receive_host():
        assert rig.host(aof, rp, n, log, byte_end, h_samples.numpy(), h_end.numpy().view(np.uint32), h_state) == 0
        d_samples.copy_(h_samples, non_blocking=True)
        d_end.copy_(h_end, non_blocking=True)
        torch.cuda.synchronize()

    # the two ways agree before either is timed
    receive()
    torch.cuda.synchronize()
    got = (d_samples.cpu().numpy().tobytes(), d_end.cpu().numpy().tobytes(), d_state.cpu().numpy().tobytes())
    receive_host()
    assert got == (h_samples.numpy().tobytes(), h_end.numpy().tobytes(), h_state.tobytes()), "the device call and the host function differ"
    total = int(h_state[12:16].view(np.uint32)[0])
    assert total == T

    def windows(fn, per_window=1, events=False):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeats):
            if events:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(per_window):
                    fn()
                b.record()
                torch.cuda.synchronize()
                out.append(a.elapsed_time(b) / per_window)
            else:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out), min(out), max(out)

    results = {"D": windows(receive, args.inner, events=True), "H": windows(receive_host)}

    base, _ = synth.make_sequence(cam_w, cam_h, 64, 4, seed=31, max_step=3)
    camera = torch.from_numpy(base).to(device)[torch.arange(n, device=device) % 64].contiguous()
    sp = aof.sequence_params(cam_w, cam_h, cw, ch, FX, FY, 15, 0, 1, 100, 0)
    L = aof.sequence_layout(eng.params, sp, n)
    ws = torch.empty(L.total_bytes, dtype=torch.uint8, device=device)
    d_times = torch.from_numpy(times).to(device)
    imu_state = torch.zeros(64, dtype=torch.uint8, device=device)
    ip = imu_rig.params(M, 0, 1, 100, 0)

    def behind():
        eng.sequence(sp, camera, d_times, workspace=ws)
        assert imu_rig.device(aof, eng, sp, ip, n, d_times, d_samples, d_end, ws, imu_state) == 0

    def chain_device():
        receive()
        behind()

    def chain_host():
        receive_host()
        behind()

    results["D+S+I"] = windows(chain_device)
    results["H+S+I"] = windows(chain_host)
    torch.cuda.synchronize()
    count = ws[L.count:L.count + 16].cpu().numpy().view(np.uint32)
    lines = [f"# tools/bench_sequence_rx.py: a log of {N} bytes ({N / 1e6:.1f} MB, {T} HIGHRES_IMU frames at 250 Hz with other traffic) for "
             f"{n} frames; {torch.cuda.get_device_name(0)}; session {args.session}; medians of {args.repeats} windows; one box, one session",
             f"# leg D: device events around {args.inner} calls, per call; the others: a host clock around work that ends in a synchronise",
             f"# scratch {scratch.numel()} bytes ({100.0 * scratch.numel() / N:.1f} % of N); the chain: {int(count[0])} records, {int(count[1])} frames sent",
             f"# {'leg':6s} {'ms':>10s} {'(min..max)':>22s}"]
    for name in ("D", "H", "D+S+I", "H+S+I"):
        med, lo, hi = results[name]
        lines.append(f"  {name:6s} {med:10.3f} {f'({lo:.3f}..{hi:.3f})':>22s}")
    d, h = results["D"][0], results["H"][0]
    lines.append(f"# the device call {'beats' if d < h else 'LOSES TO'} the host way at this size: {d:.3f} ms against {h:.3f} ms "
                 f"({N / d / 1e6:.1f} GB/s of log through the device call); the chain: {results['D+S+I'][0]:.3f} ms against {results['H+S+I'][0]:.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    eng.close()


if __name__ == "__main__":
    main()
