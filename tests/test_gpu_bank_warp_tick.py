"""The one-launch tick with the lens inside it on the device (include/aof.h, "the stream bank with a lens";
csrc/k_bank_tick_warp.hip): aof_set_bank_path is honoured with meshes bound and the staging region stays untouched, the
one-launch kernel against the composed launches on twin banks byte for byte (every designed mesh, a refused record, a
stream with a frame every other tick, ticks and bursts, packed and raw pixel formats, no records at all, first frames and
masked resets, a replayed graph, both instantiations), and against the CPU oracle's calcFlow chain fed the numpy model's
warped crops (tests/bank_warp_ref.py).  Shapes are those of tests/test_gpu_bank_warp.py (tests/bank_warp_rig.py restates its
rig): S = 5, 64 x 64 crops out of 96 x 80 planes at every alignment, T = 6."""
import numpy as np
import pytest

import bank_camera_ref as cref
import bank_ref as ref
import bank_warp_ref as wref
import crop_source_ref as csr
from bank_ref import FX, FY
from bank_rig import OFFSET, BankRig, up
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)
from bank_sensor_rig import same_rigs, table_tensor
from bank_warp_rig import H, INTERVAL, PH, PW, RATE, S, T, W, WarpRig, clamp_meshes, format_rows, mixed_meshes, planes_run

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
COUNTS = np.array([[1, 2, 3, 2, 3], [3, 3, 2, 0, 1]], np.uint8)   # burst 0, burst 1 (the issue's counts)


def params(aof, cfg):
    if cfg == "px4-64":
        return aof.px4flow_params(W, H)
    if cfg == "opencv-64":                      # two levels, mean-subtracted: the warped crop's pixel sums and level-1 image
        return aof.px4flow_params(W, H, pyramid_levels=2, mean_subtract=1)
    if cfg == "px4-64-integer":                 # no half-pixel refinement: the other instantiation
        return aof.px4flow_params(W, H, subpixel=0)
    raise KeyError(cfg)


def setup(aof, paths, cfg="px4-64"):
    p = params(aof, cfg)
    cam = aof.bank_camera_params(72, 66, W, H, 0, INTERVAL, cref.DEROTATE, FX, FY)   # (scalars no stream has)
    bp = aof.bank_params(S, FX, FY, RATE, OFFSET, 1, 100, 0)
    engs = [aof.FlowEngine(p, 0) for _ in paths]
    for e, path in zip(engs, paths):
        assert e.last_bank_path() == 0, "a fresh context has made no push"
        e.set_bank_path(path)
    return p, cam, bp, engs


MESHES = {"mixed": mixed_meshes, "clamped": clamp_meshes}


def break_stream_3(rig, dev, fmt=csr.GREY8):
    """Stream 3's record one byte beyond camera_bytes (inside the allocation's slack): AOF_TICK_BAD_SENSOR."""
    bad = rig.recs[3].copy()
    bad["offset"] = rig.camera_bytes - csr.extent(bad, fmt) + 1
    assert not csr.valid(bad, fmt, 1, W, H, rig.camera_bytes) and rig.alloc.numel() - 1 - rig.camera_bytes >= 64
    rig.recs = rig.recs.copy()
    rig.recs[3] = bad
    rig.table = table_tensor(dev, rig.recs)


def fill_staging(bank):
    bank.buffer[bank.staging:].fill_(SENTINEL)


def staging_untouched(bank):
    return bool((bank.buffer[bank.staging:] == SENTINEL).all().item())


def twins(aof, synth, dev, cfg, design, seed, make=None, fmt=csr.GREY8, ticks=T, bursts=(1, 0), reset_at=None):
    """`ticks` ticks, then bursts of K = 3 with COUNTS and a padded round stride, on twin banks: path 1 (a) against path 2
    (b).  Stream 3's record is outside camera_bytes, stream 4 has a frame every other tick.  reset_at: before that tick
    streams 1 and 4 are reset on both.  Every comparison on raw bytes (same_rigs); a's staging region keeps its sentinel."""
    make = make or (lambda eng, run, bp, cam, **kw: WarpRig(aof, eng, run, bp, dev, cam, **kw))
    p, cam, bp, (ea, eb) = setup(aof, (1, 2), cfg)
    run = planes_run(synth, seed, every_other=4)
    a, b = make(ea, run, bp, cam), make(eb, run, bp, cam)
    for r in (a, b):
        r.give_meshes(MESHES[design](r))
        break_stream_3(r, dev, fmt)
        r.bind()
    fill_staging(a.bank)
    for k in range(ticks):
        if k == reset_at:
            mask = up(dev, np.array([0, 1, 0, 0, 1], np.uint8))
            ea.bank_reset(a.bank, mask), eb.bank_reset(b.bank, mask)
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, (cfg, design, "tick", k))
        assert ea.last_bank_path() == 1 and eb.last_bank_path() == 2, (k, ea.last_bank_path(), eb.last_bank_path())
    assert (a.read().recs["quality"][3] == aof.TICK_BAD_SENSOR), "the refused stream"
    K = COUNTS.max()
    ka, kb = (make(e, run, bp, cam, K=int(K), pad=37, bank=r.bank) for e, r in ((ea, a), (eb, b)))
    for r in (ka, kb):
        r.give_meshes(a.meshes)
        break_stream_3(r, dev, fmt)
        r.bind()
    for n in bursts:
        ka.load(n, COUNTS), ka.enqueue()
        kb.load(n, COUNTS), kb.enqueue()
        same_rigs(ka, kb, (cfg, design, "burst", n))
        assert ea.last_bank_path() == 1 and eb.last_bank_path() == 2
    assert staging_untouched(a.bank), "the one-launch warped push neither reads nor writes the staging region"
    assert not staging_untouched(b.bank), "the composed path stages its crops"
    ea.close(), eb.close()


# ---- 1. the path is honoured ----

def test_the_path_is_honoured_and_path_1_leaves_the_staging_region_alone(aof, synth, gpu_device):
    """Meshes bound: path 1 runs one-launch kernels (a tick, a burst of K = 3), path 2 the composed launches, path 0 what
    the measured crossover says for S = 5 (aof_bank_warp_crossover).  Under path 1 the staging region, pre-filled with a
    sentinel, is byte for byte untouched."""
    p, cam, bp, engs = setup(aof, (1, 2, 0))
    run = planes_run(synth, 37)
    want = (1, 2, 1 if aof.bank_warp_crossover() >= S else 2)
    assert aof.bank_warp_one_launch(p)[0]
    for eng, path, asked in zip(engs, want, (1, 2, 0)):
        a = WarpRig(aof, eng, run, bp, gpu_device, cam)
        a.give_meshes(mixed_meshes(a))
        a.bind()
        fill_staging(a.bank)
        for k in range(2):
            a.load(k), a.enqueue()
            assert eng.last_bank_path() == path, (path, "tick", k)
        ka = WarpRig(aof, eng, run, bp, gpu_device, cam, meshes=a.meshes, K=3, pad=37, bank=a.bank)
        ka.bind()
        ka.load(1, COUNTS), ka.enqueue()
        assert eng.last_bank_path() == path, (path, "burst")
        a.torch.cuda.synchronize()
        assert staging_untouched(a.bank) == (path == 1), path
        # a refused push leaves the answer as it was
        big = up(gpu_device, np.concatenate([a.meshes, a.meshes[:1]]).view(np.uint8).reshape(S + 1, -1))
        eng.set_bank_warps(big, S + 1)
        with pytest.raises(aof.AofError):
            ka.enqueue()
        assert eng.last_bank_path() == path
        # nothing bound: the forms that were there before answer too
        eng.set_bank_warps(None)
        a.load(2), a.enqueue()
        assert eng.last_bank_path() == (2 if asked == 2 else 1)
        eng.close()


# ---- 2. one launch against the composed launches ----

@pytest.mark.parametrize("design", list(MESHES))
@pytest.mark.parametrize("cfg", ["px4-64", "opencv-64"])
def test_one_launch_equals_the_composed_path_on_twin_banks(aof, synth, gpu_device, cfg, design):
    twins(aof, synth, gpu_device, cfg, design, seed=38)


def test_the_integer_instantiation_equals_the_composed_path(aof, synth, gpu_device):
    """No half-pixel refinement: k_bank_tick_warped<false>."""
    twins(aof, synth, gpu_device, "px4-64-integer", "mixed", seed=39, ticks=4, bursts=(1,))


def test_first_frames_and_a_masked_reset_mid_run(aof, synth, gpu_device):
    """Streams 1 (warped) and 4 (every other tick) start over before tick 3: their next frames are first frames again --
    gather -> LDS -> slot, histogram, tail -- beside streams that go on."""
    twins(aof, synth, gpu_device, "opencv-64", "mixed", seed=40, bursts=(1,), reset_at=3)


# ---- 3. pixel formats ----

class FormatWarpRig(WarpRig):
    """WarpRig with planes of one pixel format (crop_source_ref.put_grey writes them): ROWS' alignments with pitches in the
    format's row bytes and crop origins on a pixel group; the format array is bound beside the records."""

    def __init__(self, aof, eng, run, bp, dev, cam, fmt, **kw):
        super().__init__(aof, eng, run, bp, dev, cam, fmt=fmt, rows=format_rows(fmt), **kw)


@pytest.mark.parametrize("fmt", [csr.LUMA16_LO, csr.Y10, csr.Y10P], ids=["luma16-lo", "y10", "y10p"])
def test_one_launch_equals_the_composed_path_on_other_pixel_formats(aof, synth, gpu_device, fmt):
    make = lambda eng, run, bp, cam, **kw: FormatWarpRig(aof, eng, run, bp, gpu_device, cam, fmt, **kw)
    twins(aof, synth, gpu_device, "px4-64", "mixed", seed=41, make=make, fmt=fmt, ticks=4, bursts=(1,))


def test_one_launch_equals_the_composed_path_without_sensor_records(aof, synth, gpu_device):
    """No records bound: a stream's plane is the camera parameters' frame at camera + s * camera_stride (three bytes into
    its allocation), and the unwarped stream takes the centred crop."""
    p, _, bp, (ea, eb) = setup(aof, (1, 2), "opencv-64")
    cam = aof.bank_camera_params(PW, PH, W, H, 0, INTERVAL, cref.DEROTATE, FX, FY)
    run = planes_run(synth, 42, every_other=4)
    sensors = type("Planes", (), dict(cam_w=PW, cam_h=PH, sensor=staticmethod(lambda k: run.frames[k])))
    a, b = (BankRig(aof, e, run, bp, gpu_device, camera=(cam, sensors), skew=3) for e in (ea, eb))
    x0, y0 = PW // 2 - W // 2, PH // 2 - H // 2
    d = wref.designs(W, H, PW, PH, x0, y0)
    none = d["barrel"].copy()
    none[0, 0]["x"] = wref.NONE
    meshes = np.stack([d["barrel"], d["far-outside"], none, d["quarter-turn"], d["smooth-random"]])
    points = up(gpu_device, meshes.view(np.uint8).reshape(S, -1))
    ea.set_bank_warps(points, S), eb.set_bank_warps(points, S)
    fill_staging(a.bank)
    for k in range(4):
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, ("tick", k))
    assert ea.last_bank_path() == 1 and eb.last_bank_path() == 2
    # the stored frames are the model's: the warped crops of the planes, the centred crop of the unwarped stream
    frames = a.bank.frames_bytes()[:S * W * H].reshape(S, H, W)
    flat = run.frames[3].reshape(-1)
    for s in range(4):   # (stream 4 has no frame in tick 3)
        want = wref.warp(flat, csr.record(s * PW * PH, PW, PW, PH, x0, y0), csr.GREY8, meshes[s], W, H)
        assert np.array_equal(frames[s], want), s
    assert staging_untouched(a.bank)
    ea.close(), eb.close()


# ---- 4. against the oracle chain ----

@pytest.mark.parametrize("cfg", ["px4-64", "opencv-64"])
def test_one_launch_warped_streams_are_the_oracle_chain_on_the_models_crops(aof, orc, synth, gpu_device, cfg):
    """test_warped_streams_are_the_oracle_chain_on_the_models_crops (tests/test_gpu_bank_warp.py) under path 1, with its
    seeds: its conditions -- enough published and held records, due and not-due frames -- hold on the oracle's records
    alone.  The stored frames are the model's warped crops; the refused stream's slot and state are untouched."""
    p, cam, bp, (eng,) = setup(aof, (1,), cfg)
    run = planes_run(synth, 33, every_other=4)
    a = WarpRig(aof, eng, run, bp, gpu_device, cam)
    a.give_meshes(mixed_meshes(a))
    break_stream_3(a, gpu_device)
    a.bind()
    chains = [ref.oracle_chain(aof, orc, p, RATE, OFFSET, 0) for _ in range(S)]
    due, _ = cref.gate(run.times, run.active, INTERVAL)
    px = W * H
    before_frames, before_state = a.bank.frames_bytes().copy(), a.bank.state_bytes().copy()
    published = held = 0
    for k in range(T):
        got = a.push(k)
        assert eng.last_bank_path() == 1
        frames = a.bank.frames_bytes()
        for s in range(S):
            what = (cfg, "tick", k, "stream", s)
            if s == 3:
                idle = np.zeros((), got.recs.dtype)
                idle["quality"] = aof.TICK_BAD_SENSOR
                assert got.recs[s].tobytes() == idle.tobytes() and got.wire[s] == b"", what
                assert not got.exposure[s].tobytes().strip(b"\0"), what
                continue
            if not run.active[k, s]:
                assert got.recs[s]["quality"] == aof.TICK_IDLE and got.wire[s] == b"", what
                continue
            rec, wire = chains[s].push(a.warped[0][s], run.times[k, s], run.gyro[k, s])
            assert got.recs[s].tobytes() == rec.tobytes(), what + (got.recs[s], rec)
            assert got.wire[s] == wire, what
            published += int(rec["quality"]) >= 0
            held += int(rec["quality"]) == ref.TICK_HELD
            assert frames[s * px:(s + 1) * px].tobytes() == a.warped[0][s].tobytes(), what + ("stored frame",)
            assert int(got.exposure[s]["due"]) == int(due[k, s]), what
            if due[k, s]:
                hist = wref.histogram(a.warped[0][s])
                assert got.exposure[s]["hist"].tolist() == hist.tolist(), what
                assert got.exposure[s]["msv"].tobytes() == np.float32(aof.exposure_msv(hist)).tobytes(), what
    assert published >= 2 * (S - 1) and held >= S - 1, (published, held)
    assert due[:, :3].sum() > 3 and (1 - due[:, :3])[run.active[:, :3] > 0].sum() > 3, "frames that are due and frames that are not"
    assert a.bank.frames_bytes()[3 * px:4 * px].tobytes() == before_frames[3 * px:4 * px].tobytes(), "the refused stream's stored frame"
    assert a.bank.state_bytes()[3].tobytes() == before_state[3].tobytes(), "the refused stream's state"
    eng.close()


# ---- 5. a captured graph follows the array ----

def test_a_replayed_one_launch_graph_follows_rewritten_nodes(aof, synth, gpu_device):
    """The path-1 camera push captured once after one eager tick; between replays stream 1's nodes are rewritten and
    stream 2's first node becomes AOF_WARP_NONE.  Every replay leaves what the eager pushes of a composed twin leave."""
    import torch
    p, cam, bp, (ea, eb) = setup(aof, (1, 2))
    run = planes_run(synth, 34)
    a, b = (WarpRig(aof, e, run, bp, gpu_device, cam) for e in (ea, eb))
    for r in (a, b):
        r.give_meshes(mixed_meshes(r))
        r.bind()

    def rewrite(r, k):
        if k == 2:
            r.put_mesh(1, wref.designs(W, H, PW, PH, 3, 5)["mirror"])
        if k == 3:
            none = r.meshes[2].copy()
            none[0, 0]["x"] = wref.NONE
            r.put_mesh(2, none)
    outs, crops = [], []
    for k in range(5):
        rewrite(b, k)
        b.load(k), b.enqueue()
        outs.append(b.raw())
        crops.append(b.warped[0].copy())
    final = b.bank_bytes()
    a.load(0), a.enqueue()                       # (the kernel has run before the capture)
    a.eng.bank_reset(a.bank)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.enqueue()
    assert ea.last_bank_path() == 1
    for k in range(5):
        rewrite(a, k)
        a.load(k)
        g.replay()
        assert a.raw() == outs[k], ("replay", k)
        assert a.bank.frames_bytes()[:S * W * H].reshape(S, H, W)[1].tobytes() == crops[k][1].tobytes(), ("the stored frame follows the nodes", k)
    assert a.bank_bytes() == final
    ea.close(), eb.close()
