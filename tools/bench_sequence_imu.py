#!/usr/bin/env python3
"""What the sequence pipeline's IMU call costs (aof_sequence_imu_device, csrc/k_sequence_imu.hip), one GPU, one process: a
recording of 65 536 frames of 64x64 out of 160x120 at 75 fps with HIGHRES_IMU samples at 250 Hz, three legs:
  S    aof_sequence_device alone (records only: d_gyro NULL, no vehicle time);
  S+I  the same call and aof_sequence_imu_device behind it on the stream;
  S+H  the host way: the sequence call, the records and count words copied down, a synchronise, then
       aof_sequence_imu_host on them (the frames then lie in host memory; nothing is copied back up).
Each leg is timed with a host clock around work that ends in a device synchronise, after a warm-up; the median of
--repeats runs (at least three), in ms.  One box, one session: a figure, not a gate.  Writes
profiles/sequence_imu_cost.txt (--out)."""
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
import sequence_imu_rig as rig   # noqa: E402

FX, FY = 216.6677, 216.2457


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d"), help="a name for this measuring session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_imu_cost.txt"))
    args = ap.parse_args()
    assert args.repeats >= 3, "at least three repeats"
    aof = ge.load_package()   # (raises where the library has not been built)
    synth = importlib.import_module("aero_optical_flow_amd.synth")
    device = torch.device("cuda:0")
    n, cw, ch, cam_w, cam_h = args.frames, 64, 64, 160, 120

    rng = np.random.default_rng(1)
    base, _ = synth.make_sequence(cam_w, cam_h, 64, 4, seed=31, max_step=3)
    camera = torch.from_numpy(base).to(device)[torch.arange(n, device=device) % 64].contiguous()
    times = np.cumsum(np.concatenate([[0], rng.integers(12000, 15000, n - 1)])).astype(np.int64)      # ~75 fps
    T = int(times[-1] // 4000) + 8
    samples = np.zeros(T, aof.IMU_SAMPLE_DTYPE)
    samples["time_usec"] = 7_000_000 - 20000 + np.cumsum(rng.integers(3900, 4100, T))                 # 250 Hz, from before frame 0
    samples["xgyro"], samples["ygyro"], samples["zgyro"] = rng.normal(0, 0.8, (3, T)).astype(np.float32)
    sample_end = np.searchsorted(samples["time_usec"].astype(np.int64) - 7_000_000, times).astype(np.uint32)

    eng = aof.FlowEngine(aof.px4flow_params(cw, ch), 0)
    sp = aof.sequence_params(cam_w, cam_h, cw, ch, FX, FY, 15, 0, 1, 100, 0)
    L = aof.sequence_layout(eng.params, sp, n)
    ws = torch.empty(L.total_bytes, dtype=torch.uint8, device=device)
    d_times = torch.from_numpy(times).to(device)
    d_samples = rig.up(torch, samples, device).view(-1, 24)
    d_end = rig.up(torch, sample_end, device).view(torch.int32)
    state = torch.zeros(64, dtype=torch.uint8, device=device)
    ip = rig.params(T, 0, 1, 100, 0)

    def sequence():
        eng.sequence(sp, camera, d_times, workspace=ws)

    def sequence_imu():
        sequence()
        assert rig.device(aof, eng, sp, ip, n, d_times, d_samples, d_end, ws, state) == 0

    host_frames = np.zeros((n, rig.FRAME_BYTES), np.uint8)
    host_state = np.zeros(1, aof.IMU_STATE_DTYPE)
    pinned = {name: torch.empty(size, dtype=torch.uint8).pin_memory() for name, size in (("count", 16), ("records", 32 * n))}
    host_len = np.zeros(n, np.uint8)

    def sequence_host():
        sequence()
        for name, offset in (("count", L.count), ("records", L.records)):
            pinned[name].copy_(ws[offset:offset + pinned[name].numel()], non_blocking=True)
        torch.cuda.synchronize()
        assert rig.host(aof, ip, n, times.view(np.uint64), samples, sample_end, pinned["records"].numpy().view(aof.SEQ_RECORD_DTYPE),
                        pinned["count"].numpy().view(np.uint32), host_frames, host_len, host_state) == 0

    legs = [("S", sequence), ("S+I", sequence_imu), ("S+H", sequence_host)]
    results = {name: timed(fn, args.repeats, args.warmup) for name, fn in legs}
    sequence_imu()
    torch.cuda.synchronize()
    count = ws[L.count:L.count + 16].cpu().numpy().view(np.uint32)
    lines = [f"# tools/bench_sequence_imu.py: {n} frames of {cw}x{ch} out of {cam_w}x{cam_h}, {T} samples at 250 Hz; "
             f"{torch.cuda.get_device_name(0)}; session {args.session}; medians of {args.repeats} runs, host clock around a synchronise; "
             f"one box, one session",
             f"# {int(count[0])} records, {int(count[1])} frames sent",
             f"# {'leg':4s} {'ms':>10s} {'(min..max)':>22s}"]
    for name, _ in legs:
        med, lo, hi = results[name]
        lines.append(f"  {name:4s} {med:10.3f} {f'({lo:.3f}..{hi:.3f})':>22s}")
    lines.append(f"# the IMU call on the device: S+I - S = {results['S+I'][0] - results['S'][0]:.3f} ms; the host way: S+H - S = "
                 f"{results['S+H'][0] - results['S'][0]:.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    eng.close()


if __name__ == "__main__":
    main()
