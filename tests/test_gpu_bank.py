"""The stream bank (aof_bank_push_device / aof_bank_reset_device, include/aof.h): S live streams per tick from one
device launch, against what the reference's per-frame loop leaves for each stream on its own -- the CPU oracle's
calcFlow chain, one orc.Px4 per stream fed only that stream's active frames, with the independent MAVLink serializer of
tests/mavlink_model.py; for streams 0..5 also the C++ facade driven frame by frame with its own packer.  Every record of
every tick and every wire frame is compared by bytes, never by tolerance.  Inputs: tests/bank_ref.py; the rig: tests/bank_rig.py."""
import ctypes as C

import numpy as np
import pytest

import bank_ref as ref
from bank_cases import run_case
from bank_ref import FX, FY
from bank_rig import EINVAL, ENOSPC, LIMITED, OFFSET, BankRig, params_of, same_records
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

PARITY = [
    dict(id="px4-64-15Hz", cfg="px4-64", S=24, T=48, seed=1, census=LIMITED, facade=6),
    dict(id="opencv-128-15Hz", cfg="opencv-128", S=24, T=48, seed=2, census=LIMITED, facade=6),
    dict(id="rate0", cfg="px4-64", S=24, T=48, seed=3, rate=0, facade=6),
    dict(id="rate200", cfg="px4-64", S=24, T=48, seed=4, rate=200, facade=6),
    dict(id="offset0", cfg="px4-64", S=24, T=48, seed=5, offset=0, census=LIMITED, facade=6),
    dict(id="wrap", cfg="px4-64", S=24, T=48, seed=6, wrap=True, census=LIMITED, facade=6),
    dict(id="first_seq250", cfg="px4-64", S=24, T=48, seed=7, first_seq=250, census=LIMITED, facade=6),
    dict(id="no-gyro", cfg="opencv-128", S=24, T=48, seed=8, use_gyro=False, census=LIMITED, facade=6),
    dict(id="S1", cfg="px4-64", S=1, T=48, seed=9, census=LIMITED, facade=1),
    dict(id="S300-path1", cfg="px4-64", S=300, T=8, seed=10, path=1, facade=6),
    dict(id="S300-path2", cfg="px4-64", S=300, T=8, seed=10, path=2, facade=6),
    dict(id="stride", cfg="px4-64", S=24, T=48, seed=11, census=LIMITED, frame_stride=64 * 64 + 48),
]


@pytest.mark.parametrize("case", PARITY, ids=lambda c: c["id"])
def test_bank_equals_the_oracle_chain_and_the_facade_per_stream(aof, orc, synth, gpu_device, case):
    kw = {k: v for k, v in case.items() if k != "id"}
    want = run_case(aof, orc, synth, gpu_device, **kw)
    pub, held, _ = ref.census(want)
    if case["id"].startswith("S300"):
        # 8 ticks: over all streams some frame was held and some published beyond a first frame
        assert held.sum() > 0 and (pub > 1).any()
    if case["id"] in ("rate0", "rate200"):
        q = want["quality"]
        assert held.sum() == 0 and ((q == 0) & (want["frame"] > 1)).any(1).any(), "a quality-0 publication beyond a first frame"
    if case["id"] == "first_seq250":
        assert pub.min() > 6, "the sequence number wraps through 255"


@pytest.mark.parametrize("cfg,seed", [("px4-64", 21), ("opencv-128", 22)])
def test_both_paths_leave_identical_bytes_after_every_tick(aof, synth, gpu_device, cfg, seed):
    """aof_set_bank_path(1) and (2) over the same run: records, frames, lengths AND the bank's frames and state
    regions byte-identical after every tick."""
    p = params_of(aof, cfg)
    S, T = 40, 48
    run = ref.make_run(synth, p.width, p.height, S, T, seed)
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 3)
    engs, devs = [], []
    for path in (1, 2):
        eng = aof.FlowEngine(p, 0)
        eng.set_bank_path(path)
        engs.append(eng)
        devs.append(BankRig(aof, eng, run, bp, gpu_device))
    held = published = 0
    for k in range(T):
        (ra, wa, _, _), (rb, wb, _, _) = devs[0].push(k), devs[1].push(k)
        assert ra.tobytes() == rb.tobytes(), k
        assert wa == wb, k
        assert devs[0].bank.frames_bytes().tobytes() == devs[1].bank.frames_bytes().tobytes(), k
        assert devs[0].bank.state_bytes().tobytes() == devs[1].bank.state_bytes().tobytes(), k
        held += int((ra["quality"] == aof.TICK_HELD).sum())
        published += int(((ra["quality"] >= 0) & (ra["frame"] > 1)).sum())
    assert held > 10 * S and published > 3 * S
    for e in engs:
        e.close()


@pytest.mark.parametrize("cfg,seed", [("dense-192x160", 31), ("tile16-160x128", 32)])
def test_configurations_outside_the_one_workgroup_class_run_composed(aof, orc, synth, gpu_device, cfg, seed):
    """Path 1 requested there still gives the composed path, not an error."""
    for path in (0, 1):
        run_case(aof, orc, synth, gpu_device, cfg, 12, 24, seed, path=path, census=(3, 10, 4))


def test_reset_with_a_mask_mid_run(aof, orc, synth, gpu_device):
    """Masked streams continue exactly like a fresh oracle object, the others like an uninterrupted one."""
    import torch
    p = params_of(aof, "px4-64")
    S, T, first_seq = 24, 48, 9
    run = ref.make_run(synth, 64, 64, S, T, 41)
    mask = (np.arange(S) % 3 == 1).astype(np.uint8)
    new = lambda s=0: ref.oracle_chain(aof, orc, p, 15, OFFSET, first_seq)
    want, wire = ref.expected(run, [new() for _ in range(S)], resets={20: mask}, new_chain=new)
    for path in (1, 2):
        eng = aof.FlowEngine(p, 0)
        eng.set_bank_path(path)
        dev = BankRig(aof, eng, run, aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, first_seq), gpu_device)
        for k in range(T):
            if k == 20:
                before = dev.bank.state_bytes()
                eng.bank_reset(dev.bank, torch.from_numpy(mask).to(gpu_device))
                after = dev.bank.state_bytes()
                assert not after[mask == 1].any() and after[mask == 0].tobytes() == before[mask == 0].tobytes()
            got, sent, _, _ = dev.push(k)
            same_records(got, want[k], k, f"path {path}")
            assert sent == wire[k], (path, k)
        # the masked streams' first frame after the reset is a first frame again
        first_after = [int(np.flatnonzero(run.active[20:, s])[0]) + 20 for s in np.flatnonzero(mask)]
        assert all(want[k, s]["frame"] == 1 for k, s in zip(first_after, np.flatnonzero(mask)))
        eng.close()


@pytest.mark.parametrize("path", [1, 2])
def test_a_captured_tick_replays_on_new_inputs(aof, synth, gpu_device, path):
    """One tick captured with torch.cuda.graph (a linear graph: one stream, no parallel branches) and replayed for 20
    ticks with new frames, times and masks copied into the same input tensors equals the eager run."""
    import torch
    p = params_of(aof, "opencv-128")
    S, T = 24, 20
    run = ref.make_run(synth, 128, 128, S, T, 51)
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    eng = aof.FlowEngine(p, 0)
    eng.set_bank_path(path)
    eager = BankRig(aof, eng, run, bp, gpu_device)
    outs = [eager.push(k) for k in range(T)]
    dev = BankRig(aof, eng, run, bp, gpu_device)
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
    assert dev.bank.frames_bytes().tobytes() == eager.bank.frames_bytes().tobytes()
    assert dev.bank.state_bytes().tobytes() == eager.bank.state_bytes().tobytes()
    q = np.stack([o.recs["quality"] for o in outs])
    assert (q == aof.TICK_HELD).any() and (q == aof.TICK_IDLE).any() and (q[4:] >= 0).any()
    eng.close()


def test_bank_entry_points_argument_handling(aof, synth, gpu_device):
    """What the device entry points refuse, with which code, and that a refused call leaves the bank untouched."""
    import torch
    p = params_of(aof, "px4-64")
    S = 8
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    L = aof.bank_layout(p, bp)
    buf = torch.zeros(L.total_bytes + 256, dtype=torch.uint8, device=gpu_device)
    frames = torch.from_numpy(synth.make_sequence(64, 64, S, 4, seed=61, max_step=3)[0]).to(gpu_device)
    times = torch.arange(S, dtype=torch.int64, device=gpu_device) * 1000 + 70000
    recs = torch.zeros((S, 48), dtype=torch.uint8, device=gpu_device)
    wire = torch.zeros((S, 56), dtype=torch.uint8, device=gpu_device)
    lens = torch.zeros(S, dtype=torch.uint8, device=gpu_device)
    stream = torch.cuda.current_stream().cuda_stream
    push, reset = aof.lib.aof_bank_push_device, aof.lib.aof_bank_reset_device

    def args(**kw):
        b = kw.get("bp", bp)
        return [kw.get("ctx", eng._ctx), C.byref(b) if b is not None else None, kw.get("frames", frames.data_ptr()),
                kw.get("times", times.data_ptr()), None, None, kw.get("bank", buf.data_ptr()), kw.get("bytes", L.total_bytes),
                kw.get("recs", recs.data_ptr()), kw.get("wire", wire.data_ptr()), kw.get("lens", lens.data_ptr()), stream]

    assert reset(eng._ctx, C.byref(bp), None, buf.data_ptr(), L.total_bytes, stream) == 0
    assert push(*args()) == 0                                             # every stream's first frame
    torch.cuda.synchronize()
    snapshot = buf.clone()
    bad = lambda **kw: aof.bank_params(**{**dict(n_streams=S, focal_x=FX, focal_y=FY, output_rate=15, offset_timestamp_usec=OFFSET), **kw})
    refused = [
        (dict(ctx=None), EINVAL), (dict(bp=None), EINVAL), (dict(bank=None), EINVAL), (dict(frames=None), EINVAL),
        (dict(times=None), EINVAL), (dict(recs=None), EINVAL), (dict(lens=None), EINVAL),       # d_mavlink without its lengths
        (dict(bp=bad(n_streams=0)), EINVAL), (dict(bp=bad(frame_stride=4096 + 8)), EINVAL),
        (dict(bp=bad(frame_stride=4096 - 16)), EINVAL), (dict(bp=bad(focal_x=0.0)), EINVAL),
        (dict(bank=buf.data_ptr() + 16), EINVAL),                                               # 256-byte alignment
        (dict(bytes=L.total_bytes - 1), ENOSPC),
        (dict(bp=bad(n_streams=S + 1)), ENOSPC),                                                # a bank laid out for fewer streams
    ]
    for kw, code in refused:
        assert push(*args(**kw)) == code, kw
    assert reset(None, C.byref(bp), None, buf.data_ptr(), L.total_bytes, stream) == EINVAL
    assert reset(eng._ctx, None, None, buf.data_ptr(), L.total_bytes, stream) == EINVAL
    assert reset(eng._ctx, C.byref(bp), None, None, L.total_bytes, stream) == EINVAL
    assert reset(eng._ctx, C.byref(bp), None, buf.data_ptr() + 16, L.total_bytes, stream) == EINVAL
    assert reset(eng._ctx, C.byref(bp), None, buf.data_ptr(), L.total_bytes - 1, stream) == ENOSPC
    for path, code in ((0, 0), (1, 0), (2, 0), (3, EINVAL), (-1, EINVAL)):
        assert aof.lib.aof_set_bank_path(eng._ctx, path) == code
    torch.cuda.synchronize()
    assert torch.equal(buf, snapshot), "a refused call must leave the bank untouched"
    assert b"bank" in aof.lib.aof_last_error(eng._ctx)
    # the context is still usable, and NULL d_mavlink / d_active / d_gyro are fine
    a = args(wire=None, lens=None)
    times += 80000
    assert push(*a) == 0
    torch.cuda.synchronize()
    r = aof.ticks_view(recs)
    assert (r["frame"] == 2).all() and (r["quality"] >= 0).all() and (r["dt_us"] == times.cpu().numpy()).all()
    eng.close()


RANDOM = [   # S in 1..200, size, levels, rate, mask density, gyro on/off, path: drawn once from seed 2024 and written down
    dict(cfg="px4-64", S=137, T=41, rate=15, density=0.8, use_gyro=True, path=0),
    dict(cfg="px4-96x80-2", S=23, T=48, rate=30, density=0.6, use_gyro=False, path=1),
    dict(cfg="opencv-128", S=200, T=30, rate=15, density=0.9, use_gyro=True, path=2),
    dict(cfg="px4-96x80", S=1, T=44, rate=12, density=0.7, use_gyro=True, path=1),
    dict(cfg="px4-128", S=64, T=36, rate=20, density=0.5, use_gyro=False, path=0),
    dict(cfg="opencv-64", S=181, T=33, rate=10, density=0.95, use_gyro=True, path=0),
    dict(cfg="px4-64", S=97, T=47, rate=40, density=0.3, use_gyro=True, path=2),
    dict(cfg="opencv-128", S=9, T=39, rate=25, density=0.75, use_gyro=False, path=1),
]


@pytest.mark.parametrize("n", range(len(RANDOM)))
def test_seeded_random_cases_against_the_oracle_chain(aof, orc, synth, gpu_device, n):
    case = RANDOM[n]
    want = run_case(aof, orc, synth, gpu_device, seed=100 + n, first_seq=(37 * n) & 0xFF, **case)
    pub, held, _ = ref.census(want)
    assert (pub > 1).any() and held.sum() > 0, "the whole case holds and publishes"
