#!/usr/bin/env python3
"""What the sequence pipeline's motion field costs (aof_sequence_field_device, csrc/k_sequence_field.hip behind k_field.hip),
one GPU, one process, on two recordings at 75 fps and 15 Hz output: the one tools/bench_sequence_imu.py uses (65 536 frames of
64x64 out of 160x120) and a two-level one (128x128 out of 320x240, --frames-128 frames).  Legs:
  S      aof_sequence_device alone;
  S+F    the same call and aof_sequence_field_device behind it on the stream;
  F      the field call alone, on the workspace the sequence call left;
  fit    aof_field_batch_device alone over the workspace's block records: the field call's first launch;
  win    the window launch: F - fit, by difference (the C ABI has no call that makes it alone);
  S+H    the host way: the sequence call, the block records, sub-directions, flows, records and count words copied down, a
         synchronise, then aof_sequence_field_host on them.
Each leg is timed with a pair of HIP events around what it enqueues (S+H: a host clock around work that ends in a
synchronise), after a warm-up; the median of --repeats runs (at least three), in ms.  One box, one session: figures, not
gates.  Writes profiles/sequence_field_cost.txt (--out)."""
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
import field_ref as fr   # noqa: E402
import sequence_field_ref as ref   # noqa: E402
import sequence_field_rig as rig   # noqa: E402

FX, FY = 216.6677, 216.2457


def timed(fn, repeats, warmup, events=True):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        else:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def recording(aof, synth, device, n, cw, ch, cam_w, cam_h, levels, repeats, warmup):
    rng = np.random.default_rng(1)
    base, _ = synth.make_sequence(cam_w, cam_h, 64, 4, seed=31, max_step=3)
    camera = torch.from_numpy(base).to(device)[torch.arange(n, device=device) % 64].contiguous()
    times = np.cumsum(np.concatenate([[0], rng.integers(12000, 15000, n - 1)])).astype(np.int64)      # ~75 fps
    p = aof.px4flow_params(cw, ch) if levels == 1 else aof.px4flow_params(cw, ch, pyramid_levels=2, mean_subtract=1)
    eng = aof.FlowEngine(p, 0)
    nb = eng.nblocks(0)
    sp = aof.sequence_params(cam_w, cam_h, cw, ch, FX, FY, 15, 0, 1, 100, 0)
    L = aof.sequence_layout(p, sp, n)
    ws = torch.empty(L.total_bytes, dtype=torch.uint8, device=device)
    d_times = torch.from_numpy(times).to(device)
    fields = torch.zeros((n - 1, 64), dtype=torch.uint8, device=device)
    out = torch.zeros((n, 48), dtype=torch.uint8, device=device)
    state = torch.zeros(64, dtype=torch.uint8, device=device)
    at_b, at_s = rig.block_offsets(aof, p, L, n)
    d_blocks = ws[at_b:at_b + 4 * (n - 1) * nb].view(torch.int32).view(n - 1, nb)
    d_subdirs = ws[at_s:at_s + (n - 1) * nb].view(n - 1, nb) if p.subpixel else None
    d_flows = ws[L.flows:L.flows + 16 * (n - 1)]

    def sequence():
        eng.sequence(sp, camera, d_times, workspace=ws)

    def field():
        assert rig.device(aof, eng, sp, n, ws, fields, out, state) == 0

    def sequence_field():
        sequence()
        field()

    def fit():
        eng.field_batch(d_blocks, d_flows, subdirs=d_subdirs, fields=fields)

    sizes = (("count", L.count, 16), ("records", L.records, 32 * n), ("flows", L.flows, 16 * (n - 1)), ("blocks", at_b, 4 * (n - 1) * nb),
             ("subdirs", at_s, (n - 1) * nb))
    pinned = {name: torch.empty(size, dtype=torch.uint8).pin_memory() for name, _, size in sizes}

    def sequence_host():
        sequence()
        for name, offset, size in sizes:
            pinned[name].copy_(ws[offset:offset + size], non_blocking=True)
        torch.cuda.synchronize()
        M = int(pinned["count"].numpy().view(np.uint32)[0])
        rc = rig.host(aof, p, sp, n, pinned["blocks"].numpy().view(fr.BLOCK_DTYPE).reshape(n - 1, nb), pinned["subdirs"].numpy().reshape(n - 1, nb),
                      pinned["flows"].numpy().view(fr.FLOW_DTYPE), pinned["records"].numpy().view(ref.SEQ_RECORD_DTYPE)[:M])[0]
        assert rc == 0

    results = {"S": timed(sequence, repeats, warmup)}
    results["S+F"] = timed(sequence_field, repeats, warmup)
    results["F"] = timed(field, repeats, warmup)
    results["fit"] = timed(fit, repeats, warmup)
    results["S+H"] = timed(sequence_host, repeats, warmup, events=False)
    sequence_field()
    torch.cuda.synchronize()
    count = ws[L.count:L.count + 16].cpu().numpy().view(np.uint32)
    o = out.cpu().numpy().reshape(-1).view(rig.RECORD_DTYPE)[:int(count[0])]
    lines = [f"# {n} frames of {cw}x{ch} out of {cam_w}x{cam_h}, {levels} level(s), {nb} blocks a pair: {int(count[0])} records, "
             f"status word {int(count[2])}, {int((o['status'] >= 1).sum())} with a fit, longest window {int(o['pairs'].max())} pairs",
             f"# {'leg':4s} {'ms':>10s} {'(min..max)':>22s}"]
    for name in ("S", "S+F", "F", "fit", "S+H"):
        med, lo, hi = results[name]
        lines.append(f"  {name:4s} {med:10.3f} {f'({lo:.3f}..{hi:.3f})':>22s}")
    lines.append(f"# the field call behind the sequence call: S+F - S = {results['S+F'][0] - results['S'][0]:.3f} ms; the window launch: "
                 f"F - fit = {results['F'][0] - results['fit'][0]:.3f} ms; the host way: S+H - S = {results['S+H'][0] - results['S'][0]:.3f} ms")
    eng.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--frames-128", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d"), help="a name for this measuring session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_field_cost.txt"))
    args = ap.parse_args()
    assert args.repeats >= 3, "at least three repeats"
    aof = ge.load_package()   # (raises where the library has not been built)
    synth = importlib.import_module("aero_optical_flow_amd.synth")
    device = torch.device("cuda:0")
    lines = [f"# tools/bench_sequence_field.py: {torch.cuda.get_device_name(0)}; session {args.session}; medians of {args.repeats} runs, HIP "
             f"events around each leg (S+H: host clock around a synchronise); one box, one session",
             "# not measured: the long tail window of a stalled recording (one lane walking up to n - 1 pairs)"]
    lines += recording(aof, synth, device, args.frames, 64, 64, 160, 120, 1, args.repeats, args.warmup)
    lines += recording(aof, synth, device, args.frames_128, 128, 128, 320, 240, 2, args.repeats, args.warmup)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
