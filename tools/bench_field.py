#!/usr/bin/env python3
"""What the motion-field fit costs behind a batch (aof_field_batch_device, csrc/k_field.hip), one GPU, one process:
  F   the call on the block records aof_flow_batch_device left on the device -- C2 (1 024 VGA pairs, 4 661 blocks each), C5
      (256 pairs of 1280x960, 16x16 tiles, 4 661 blocks) and C1 in batch (8 192 pairs of 64x64, 25 blocks) --, timed with HIP
      events around a group of calls on the stream, after a warm-up; the median over the groups, in us per call;
  K3  the reduction kernel (k_reduce, through aof_kernel_ms's ring) on the SAME records in the same session: it reads the same
      bytes once and is the natural yardstick.  Where a configuration's search writes the flow records itself (small grids:
      no K3 launch), the context is put on the generic search for this leg, which keeps K3.
Both read n_pairs * nb * 4 bytes of records (+ nb sub-directions with half-pixel refinement); GB/s is that over the time.
One box, one session: a figure, not a gate.  Writes profiles/field_fit_cost.txt (--out)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402

CONFIGS = (
    # name, pairs, width, height, px4flow, overrides, synthetic reach
    ("c2", 1024, 640, 480, False, dict(), 4),
    ("c5", 256, 1280, 960, False, dict(tile=16, search=8, value_threshold=12000), 8),
    ("c1b", 8192, 64, 64, True, dict(), 4),
)


def frames(synth, w, h, n, reach, device, distinct=8):
    """n pairs on the device: `distinct` warped pairs (zoom and rotation: the field the fit is for) repeated."""
    pairs = [synth.make_warp_pair(w, h, reach=min(reach, 2), pair_index=k, noise=2) for k in range(distinct)]
    prev = torch.from_numpy(np.stack([p[0] for p in pairs])).to(device)
    cur = torch.from_numpy(np.stack([p[1] for p in pairs])).to(device)
    rep = -(-n // distinct)
    return prev.repeat(rep, 1, 1)[:n].contiguous(), cur.repeat(rep, 1, 1)[:n].contiguous()


def time_calls(fn, repeats, group, warmup):
    """Median over `repeats` groups of `group` calls, us per call, between two HIP events on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(group):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / group)
    return statistics.median(out), min(out), max(out)


def k3_us(aof, eng, prev, cur, blocks, sub, flows, repeats):
    """Median duration of K3 over `repeats` batches, us; None where no K3 launch happens."""
    eng.set_profiling(True, kernels=[aof.K_REDUCE])
    for _ in range(repeats + 3):
        eng.flow_batch(prev, cur, blocks=blocks, subdirs=sub, flows=flows)
    torch.cuda.synchronize()
    ms = eng.profile_ms(aof.K_REDUCE)[3:]
    eng.set_profiling(False)
    return statistics.median(ms) * 1000.0 if ms else None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=30, help="timed groups per leg (at least 20)")
    ap.add_argument("--group", type=int, default=20, help="calls per timed group")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--configs", default="c2,c5,c1b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_fit_cost.txt"))
    args = ap.parse_args()
    assert args.repeats >= 20, "at least 20 repeats"
    aof = ge.load_package()   # (raises where the library has not been built)
    import importlib
    synth = importlib.import_module("aero_optical_flow_amd.synth")
    device = torch.device("cuda:0")
    lines = [f"# tools/bench_field.py: aof_field_batch_device (F) against K3 on the same records; {torch.cuda.get_device_name(0)}; "
             f"medians of {args.repeats} groups of {args.group} calls (F) and of {args.repeats} launches (K3); one box, one session",
             f"# {'config':6s} {'pairs':>6s} {'blocks':>7s} {'MB read':>8s} {'F us':>9s} {'(min..max)':>17s} {'F GB/s':>8s} {'K3 us':>9s} {'K3 GB/s':>8s} {'F/K3':>6s}"]
    for name, n, w, h, px4, kw, reach in CONFIGS:
        if name not in args.configs.split(","):
            continue
        p = aof.px4flow_params(w, h, **kw) if px4 else aof.default_params(w, h, **kw)
        eng = aof.FlowEngine(p, 0)
        nb = eng.nblocks(0)
        prev, cur = frames(synth, w, h, n, reach, device)
        blocks = torch.empty((n, nb), dtype=torch.int32, device=device)
        flows = torch.empty((n, 16), dtype=torch.uint8, device=device)
        sub = torch.empty((n, nb), dtype=torch.uint8, device=device) if p.subpixel else None
        fields = torch.empty((n, 64), dtype=torch.uint8, device=device)
        fp = aof.field_params()
        k3 = k3_us(aof, eng, prev, cur, blocks, sub, flows, args.repeats)
        if k3 is None:   # the search wrote the flow records itself: the generic search keeps K3, the records are the same
            eng.force_generic(True)
            k3 = k3_us(aof, eng, prev, cur, blocks, sub, flows, args.repeats)
            eng.force_generic(False)
            eng.flow_batch(prev, cur, blocks=blocks, subdirs=sub, flows=flows)
        med, lo, hi = time_calls(lambda: eng.field_batch(blocks, flows, subdirs=sub, fields=fields, params=fp), args.repeats, args.group, args.warmup)
        f = aof.fields_view(fields)
        valid, refit = int((f["flags"] & 1 != 0).sum()), int((f["flags"] & 2 != 0).sum())
        mb = n * nb * (5 if sub is not None else 4) / 1e6
        gbs = lambda us: mb / 1e3 / (us * 1e-6) if us else float("nan")
        lines.append(f"  {name:6s} {n:6d} {nb:7d} {mb:8.2f} {med:9.2f} {f'({lo:.2f}..{hi:.2f})':>17s} {gbs(med):8.1f} "
                     f"{(k3 if k3 is not None else float('nan')):9.2f} {gbs(k3):8.1f} {(med / k3 if k3 else float('nan')):6.2f}"
                     f"   # {valid} of {n} records valid, {refit} refitted")
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
