"""The stream bank with a lens on the device (include/aof.h, "the stream bank with a lens"): the warp kernel against the
numpy model (tests/bank_warp_ref.py, held to aof_warp_host on the CPU by tests/test_bank_warp_ref.py) byte for byte, and
everything behind the warped crop against what exists already -- a twin bank with nothing bound, the CPU oracle's calcFlow
chain fed the model's crops.  Sizes are the smallest that reach every path of the kernel: 64 x 64 out of 96 x 80 planes
(16-byte stores), 20 x 12 (a lane per pixel; the width a multiple of neither 8 nor 16) and 16 x 136 (two strips: the
histogram through atomics), and the edges of the launch plan as tests/warp_plan_ref.py lists them (WARP_CASES: second trips,
node trips, a mask edge inside an item, a halved strip, the widest crops served and the first refused); S = 5.  Every camera buffer is allocated with slack behind camera_bytes."""
import numpy as np
import pytest

import bank_camera_ref as cref
import bank_ref as ref
import bank_warp_ref as wref
import crop_source_ref as csr
import warp_plan_ref as wplan
from bank_ref import FX, FY
from bank_rig import EINVAL, OFFSET, Guarded, put, same, untouched, up
from bank_sensor_rig import SLACK, SensorRig, same_rigs, table_tensor
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

S, W, H, PW, PH = 5, 64, 64, 96, 80
RATE, INTERVAL, T = 15, 50_000, 6
# sensor width, height, pitch, offset mod 16, crop origin: padded rows, every alignment, the plain crop at and off the centre
# (stream 2's last nodes are the plane's last pixel: an identity mesh is the plain crop while its nodes lie inside the plane)
ROWS = [(PW, PH, PW, 0, None), (PW, PH, PW + 8, 8, (3, 5)), (PW, PH, PW + 1, 1, (31, 15)), (PW, PH, PW + 35, 7, (0, 0)), (PW, PH, PW, 15, None)]
ORDER = [0, 1, 4, 3, 2]


# ---- 1. the stateless form against the model ----

CASES = {c["id"]: c for c in wplan.WARP_CASES}      # the edges of the launch plan (tests/warp_plan_ref.py names what each is there for)
SIZES = {cid: (c["w"], c["h"], *c["plane"]) for cid, c in CASES.items()}
FORMATS = (csr.GREY8, csr.LUMA16_LO, csr.Y10, csr.Y10P)
WIDE_FORMATS = (csr.GREY8, csr.Y10P)
RUNS = [(cid, fmt) for cid, c in CASES.items() for fmt in FORMATS if not c["wide"] or fmt in WIDE_FORMATS]
FORMAT_IDS = {csr.GREY8: "grey8", csr.LUMA16_LO: "luma16-lo", csr.Y10: "y10", csr.Y10P: "y10p"}


@pytest.mark.parametrize("size,fmt", RUNS, ids=[f"{cid}-{FORMAT_IDS[fmt]}" for cid, fmt in RUNS])
def test_ingest_warped_is_the_model_on_every_design(aof, gpu_device, size, fmt):
    """One frame per design (and one not warped, and one whose record is not valid) in one launch: planes of `fmt` at
    non-zero offsets with padded pitches in a noise buffer, into dirty guarded outputs; crops byte for byte, histograms as
    exact integers, ok flags.  The refused frame: not read, its crop not written.  A case the plan refuses (a crop too
    wide): EINVAL before any launch, no output byte and no ok flag touched."""
    import torch
    case, plan = CASES[size], wplan.case_warp_plan(CASES[size])
    w, h, width, height = SIZES[size]
    rb = csr.row_bytes(fmt, width)
    x0, y0 = width // 2 - w // 2, height // 2 - h // 2
    designs = wref.designs(w, h, width, height, x0, y0)
    names = [k for k in designs if not case["wide"] or k in wplan.WIDE_DESIGNS] + ["none", "refused"]
    n = len(names)
    assert n == wplan.case_frames(case)
    recs, cursor = np.zeros(n, csr.SENSOR_DTYPE), 0
    for i in range(n):
        off = cursor + 1 + i % 5
        recs[i] = csr.record(off, rb + (3 * i) % 11, width, height, x0, y0)
        cursor = off + csr.extent(recs[i], fmt)
    nbytes = cursor
    recs[n - 1]["height"] += 1                                     # one row more than the buffer holds behind it
    assert [csr.valid(r, fmt, 1, w, h, nbytes) for r in recs] == [True] * (n - 1) + [False]
    buf = np.random.default_rng([n, w, fmt]).integers(0, 256, nbytes + SLACK, dtype=np.uint8)
    buf[::7] = 255                                                 # saturated bytes among the noise: counted in no bin
    none = designs["smooth-random"].copy()
    none[0, 0]["x"] = wref.NONE
    meshes = np.stack([designs[k] for k in names[:-2]] + [none, designs["barrel"]])
    points = up(gpu_device, meshes.view(np.uint8).reshape(-1))
    assert points.data_ptr() % 16 == 0
    skew = case["skew"] or (3 if w % 16 else 0)
    crops, hist, ok = Guarded(gpu_device, (n, h, w), skew=skew), Guarded(gpu_device, (n, 40)), Guarded(gpu_device, (n,))
    assert crops.tensor.data_ptr() % 16 == skew and bool(plan["vec"]) == (w % 16 == 0 and skew == 0)
    formats = up(gpu_device, np.concatenate([[0xEE], np.full(n, fmt, np.uint8)]).astype(np.uint8))[1:]
    call = lambda: aof.ingest_warped(up(gpu_device, buf), table_tensor(gpu_device, recs), points, w, h, camera_bytes=nbytes, cropped=crops.tensor,
                                     hist=hist.tensor.view(torch.int32), ok=ok.tensor, want_cropped=False, want_hist=False, formats=formats)
    if plan["verdict"] != "ok":
        with pytest.raises(aof.AofError) as e:
            call()
        torch.cuda.synchronize()
        assert e.value.code == EINVAL, "a crop too wide"
        assert untouched(crops.read()) and untouched(hist.read()) and untouched(ok.read()), "a refused call writes nothing"
        return
    call()
    torch.cuda.synchronize()
    assert ok.read().tolist() == [1] * (n - 1) + [0]
    got_c, got_h = crops.read(), hist.read().view("<u4")
    for i, name in enumerate(names[:-1]):
        want = wref.warp(buf, recs[i], fmt, meshes[i], w, h)
        same(got_c[i], want, ("crop", name))
        same(got_h[i], wref.histogram(want), ("histogram", name))
        assert name in ("identity", "none") or not np.array_equal(want, csr.crop(buf, recs[i], fmt, 1, w, h)), (name, "the mesh matters")
    assert np.array_equal(got_c[n - 2], csr.crop(buf, recs[n - 2], fmt, 1, w, h)), "not warped: the plain crop"
    assert untouched(got_c[n - 1]), "a refused frame: no byte of its crop is written"
    # its histogram: untouched where a workgroup owns a frame; zeros where several strips add to words zeroed in front of them
    assert not got_h[n - 1].any() if plan["zero_hist"] else untouched(got_h[n - 1])


def test_ingest_warped_without_a_crop_or_without_a_histogram(aof, gpu_device):
    """Either output alone (the bank's push without exposure records asks for no histogram)."""
    import torch
    w, h, width, height = SIZES["vector-64x64"]
    rec = csr.record(5, width + 3, width, height, 16, 8)
    buf = np.random.default_rng(9).integers(0, 256, 5 + csr.extent(rec) + SLACK, dtype=np.uint8)
    mesh = wref.designs(w, h, width, height, 16, 8)["barrel"]
    want = wref.warp(buf, rec, csr.GREY8, mesh, w, h)
    cam, table, points = up(gpu_device, buf), table_tensor(gpu_device, np.array([rec])), up(gpu_device, mesh.view(np.uint8).reshape(-1))
    c, _, _ = aof.ingest_warped(cam, table, points, w, h, camera_bytes=len(buf) - SLACK, want_hist=False, want_ok=False)
    _, hh, _ = aof.ingest_warped(cam, table, points, w, h, camera_bytes=len(buf) - SLACK, want_cropped=False, want_ok=False)
    torch.cuda.synchronize()
    assert np.array_equal(c.cpu().numpy()[0], want) and hh.cpu().numpy()[0].tolist() == wref.histogram(want).tolist()


# ---- the rig of the bank tests: grey planes of moving texture behind sensor records, a mesh per stream ----

def planes_run(synth, seed, every_other=None):
    """bank_ref.Run whose `frames` are whole sensor planes [T, S, PH, PW] of moving texture (the warp reads anywhere in
    them); every stream has a frame in every tick but `every_other`, which has one in the even ticks."""
    rng = np.random.default_rng(seed)
    frames = np.zeros((T, S, PH, PW), np.uint8)
    times, active = np.zeros((T, S), np.int64), np.ones((T, S), np.uint8)
    gyro = rng.normal(0, 0.004, (T, S, 4)).astype(np.float32)
    gyro[..., 3] = 0.013
    for s in range(S):
        seq, _ = synth.make_sequence(PW, PH, T, 4, seed=1000 * seed + s, max_step=2)
        if s == every_other:
            active[1::2, s] = 0
        frames[np.flatnonzero(active[:, s]), s] = seq[:int(active[:, s].sum())]
        times[:, s] = np.cumsum(rng.integers(20000, 30000, T))
    return ref.Run(frames, times, gyro, active)


class WarpRig(SensorRig):
    """SensorRig on ROWS whose buffer holds the run's whole planes; meshes: [S, ny, nx] (POINT_DTYPE) or None: no array.
    self.warped[r]: the model's crops of round r's buffer by the records and meshes the HOST knows (self.recs,
    self.meshes; zeros for a record that is not valid)."""

    def __init__(self, aof, eng, run, bp, dev, cam, meshes=None, K=None, pad=0, bank=None):
        super().__init__(aof, eng, run, bp, dev, cam, None, K=K, pad=pad, bank=bank, tables=[(ROWS, ORDER)])
        self.meshes = None if meshes is None else np.ascontiguousarray(meshes, wref.POINT_DTYPE).copy()
        self.points = None if meshes is None else up(dev, self.meshes.view(np.uint8).reshape(S, -1))
        self.warped = [None] * (K or 1)

    def bind(self):
        super().bind()
        if self.points is not None:
            assert self.points.data_ptr() % 16 == 0
            self.eng.set_bank_warps(self.points, S)

    def put_mesh(self, s, mesh):
        self.meshes[s] = mesh
        put(self.points, s, self.meshes[s])

    def fill_frames(self, k, sensors=None):
        R = self.K or 1
        for r in range(R):
            n = k * R + r
            buf = np.random.default_rng([self.seed, n]).integers(0, 256, self.layout_bytes, dtype=np.uint8)
            for s, rec in enumerate(self.layouts[0]):
                csr.put_grey(buf, int(rec["offset"]) + np.arange(PH)[:, None] * int(rec["pitch"]), csr.GREY8, np.arange(PW)[None, :], self.run.frames[n, s])
            self.warped[r] = np.stack([self.model(buf, s, r) for s in range(S)])
            self.frames[r * self.round:r * self.round + self.layout_bytes].copy_(self.torch.from_numpy(buf))

    def model(self, buf, s, r=0):
        if not csr.valid(self.recs[s], csr.GREY8, 1, W, H, self.camera_bytes - r * self.round):
            return np.zeros((H, W), np.uint8)
        mesh = self.meshes[s] if self.meshes is not None else wref.identity(W, H, int(self.recs[s]["x0"]), int(self.recs[s]["y0"]))
        return wref.warp(buf, self.recs[s], csr.GREY8, mesh, W, H)


def setup(aof, path, n=2, cfg="px4-64"):
    p = aof.px4flow_params(W, H) if cfg == "px4-64" else aof.px4flow_params(W, H, pyramid_levels=2, mean_subtract=1)
    cam = aof.bank_camera_params(72, 66, W, H, 0, INTERVAL, cref.DEROTATE, FX, FY)   # (scalars no stream has)
    bp = aof.bank_params(S, FX, FY, RATE, OFFSET, 1, 100, 0)
    engs = [aof.FlowEngine(p, 0) for _ in range(n)]
    for e in engs:
        e.set_bank_path(path)
    return p, cam, bp, engs


def identities(rig):
    return np.stack([wref.identity(W, H, int(r["x0"]), int(r["y0"])) for r in rig.layouts[0]])


# ---- 2. identity meshes change nothing ----

@pytest.mark.parametrize("path", [0, 1, 2])
def test_identity_meshes_leave_the_bytes_of_a_bank_with_nothing_bound(aof, synth, gpu_device, path):
    """Ticks, then a burst of K = 3 on the same banks: records, wire frames and lengths, exposure records, de-rotated
    pairs, the stored frames, the states and the gates of a bank with identity meshes bound against a twin without."""
    p, cam, bp, (ea, eb) = setup(aof, path)
    run = planes_run(synth, 31, every_other=4)
    a = WarpRig(aof, ea, run, bp, gpu_device, cam)
    a.meshes = identities(a)
    a.points = up(gpu_device, a.meshes.view(np.uint8).reshape(S, -1))
    b = WarpRig(aof, eb, run, bp, gpu_device, cam)
    a.bind(), b.bind()
    for k in range(3):
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, (path, "tick", k))
        assert np.array_equal(a.warped[0], np.stack([csr.crop(a.frames[:a.layout_bytes].cpu().numpy(), r, 0, 1, W, H) for r in a.recs]))
    K = 3
    ka = WarpRig(aof, ea, run, bp, gpu_device, cam, meshes=a.meshes, K=K, pad=37, bank=a.bank)
    kb = WarpRig(aof, eb, run, bp, gpu_device, cam, K=K, pad=37, bank=b.bank)
    ka.bind(), kb.bind()
    given = np.array([[3, 3, 2, 0, 1]] * 2, np.uint8)
    ka.load(1, given), ka.enqueue()
    kb.load(1, given), kb.enqueue()
    same_rigs(ka, kb, (path, "burst"))
    ea.close(), eb.close()


def test_identity_meshes_without_sensor_records(aof, synth, gpu_device):
    """No records bound: a mesh's plane is the camera parameters' frame, and an unwarped stream takes the centred crop."""
    from bank_rig import BankRig
    p, _, bp, (ea, eb) = setup(aof, 0)
    cam = aof.bank_camera_params(PW, PH, W, H, 0, INTERVAL, cref.DEROTATE, FX, FY)
    run = planes_run(synth, 32)
    sensors = type("Planes", (), dict(cam_w=PW, cam_h=PH, sensor=staticmethod(lambda k: run.frames[k])))
    a, b = (BankRig(aof, e, run, bp, gpu_device, camera=(cam, sensors), skew=3) for e in (ea, eb))
    meshes = np.stack([wref.identity(W, H, PW // 2 - W // 2, PH // 2 - H // 2)] * S)
    meshes[2][0, 0]["x"] = wref.NONE
    points = up(gpu_device, meshes.view(np.uint8).reshape(S, -1))
    ea.set_bank_warps(points, S)
    for k in range(3):
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, ("tick", k))
    ea.close(), eb.close()


# ---- 3. warped streams against the oracle chain ----

def mixed_meshes(rig):
    """Stream 0 not warped, 1 the helper's barrel lens, 2 a quarter turn, 3 (whose record the test breaks) a half-pixel
    shift, 4 a smooth random mesh."""
    d = [wref.designs(W, H, PW, PH, int(r["x0"]), int(r["y0"]), seed=s) for s, r in enumerate(rig.layouts[0])]
    none = d[0]["half-both"].copy()
    none[0, 0]["x"] = wref.NONE
    return np.stack([none, d[1]["barrel"], d[2]["quarter-turn"], d[3]["half-both"], d[4]["smooth-random"]])


@pytest.mark.parametrize("cfg", ["px4-64", "opencv-64"])
def test_warped_streams_are_the_oracle_chain_on_the_models_crops(aof, orc, synth, gpu_device, cfg):
    """Six ticks of the mixed bank: every stream's records and wire frames are those of an oracle chain of its own fed the
    model's warped crops; exposure records carry the warped crop's histogram and MSV where the gate's model says due;
    the stored frames are the warped crops.  Stream 3's record lies outside camera_bytes: AOF_TICK_BAD_SENSOR in every
    tick, its bank bytes untouched; stream 4 has a frame every other tick."""
    p, cam, bp, (eng,) = setup(aof, 0, n=1, cfg=cfg)
    run = planes_run(synth, 33, every_other=4)
    a = WarpRig(aof, eng, run, bp, gpu_device, cam)
    a.meshes = mixed_meshes(a)
    a.points = up(gpu_device, a.meshes.view(np.uint8).reshape(S, -1))
    bad = a.recs[3].copy()
    bad["offset"] = a.camera_bytes - csr.extent(bad) + 1
    assert not csr.valid(bad, 0, 1, W, H, a.camera_bytes) and a.alloc.numel() - 1 - a.camera_bytes >= 64
    a.recs = a.recs.copy()
    a.recs[3] = bad
    a.table = table_tensor(gpu_device, a.recs)
    a.bind()
    chains = [ref.oracle_chain(aof, orc, p, RATE, OFFSET, 0) for _ in range(S)]
    due, _ = cref.gate(run.times, run.active, INTERVAL)
    px = W * H
    before_frames, before_state = a.bank.frames_bytes().copy(), a.bank.state_bytes().copy()
    published = held = 0
    for k in range(T):
        got = a.push(k)
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


# ---- 4. a captured graph follows the array ----

def test_a_replayed_graph_follows_rewritten_nodes(aof, synth, gpu_device):
    """The camera push captured once; between replays stream 1's nodes are rewritten and stream 2's first node becomes
    AOF_WARP_NONE.  Every replay leaves what the eager pushes of a twin with the same arrays leave."""
    import torch
    p, cam, bp, (ea, eb) = setup(aof, 0)
    run = planes_run(synth, 34)
    a, b = (WarpRig(aof, e, run, bp, gpu_device, cam) for e in (ea, eb))
    for r in (a, b):
        r.meshes = mixed_meshes(r)
        r.points = up(gpu_device, r.meshes.view(np.uint8).reshape(S, -1))
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
    a.load(0), a.enqueue()                       # (every kernel of the tick has run before the capture)
    a.eng.bank_reset(a.bank)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.enqueue()
    for k in range(5):
        rewrite(a, k)
        a.load(k)
        g.replay()
        assert a.raw() == outs[k], ("replay", k)
        assert a.bank.frames_bytes()[:S * W * H].reshape(S, H, W)[1].tobytes() == crops[k][1].tobytes(), ("the stored frame follows the nodes", k)
    assert a.bank_bytes() == final
    ea.close(), eb.close()


# ---- 5. refusals and unbinding ----

def test_refusals_leave_the_bank_untouched_and_unbinding_gives_the_unbound_bytes(aof, synth, gpu_device):
    p, cam, bp, (ea, eb) = setup(aof, 0)
    run = planes_run(synth, 35)
    a, b = (WarpRig(aof, e, run, bp, gpu_device, cam) for e in (ea, eb))
    a.meshes = mixed_meshes(a)
    a.points = up(gpu_device, a.meshes.view(np.uint8).reshape(S, -1))
    a.bind(), b.bind()
    a.load(0), a.enqueue()
    b.load(0), b.enqueue()
    assert a.raw() != b.raw(), "the meshes matter"
    a.load(1)
    before = (a.raw(), a.bank_bytes())

    def refused(what):
        with pytest.raises(aof.AofError) as e:
            a.enqueue()
        assert e.value.code == EINVAL, what
        assert (a.raw(), a.bank_bytes()) == before, (what, "nothing was written")
    bins = up(gpu_device, np.ones(S, np.uint8))
    ea.set_bank_binning(bins, S)
    refused("a binning bound as well")
    ea.set_bank_binning(None)
    big = up(gpu_device, np.concatenate([a.meshes, a.meshes[:1]]).view(np.uint8).reshape(S + 1, -1))
    ea.set_bank_warps(big, S + 1)
    refused("a wrong stream count")
    raw = up(gpu_device, np.zeros(a.points.numel() + 16, np.uint8))
    with pytest.raises(aof.AofError) as e:
        ea._check(aof.lib.aof_set_bank_warps(ea._ctx, raw.data_ptr() + 8, S))
    assert e.value.code == EINVAL, "a misaligned array"
    refused("the refused binding left the wrong count bound")
    with pytest.raises(aof.AofError):
        ea._check(aof.lib.aof_set_bank_warps(ea._ctx, raw.data_ptr(), 0))
    # unbound: both banks start over and leave the same bytes
    ea.set_bank_warps(None)
    for e, r in ((ea, a), (eb, b)):
        e.bank_reset(r.bank)
    for k in range(2):
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        same_rigs(a, b, ("unbound", k))
    ea.close(), eb.close()


# ---- 6. the facade ----

def test_the_facade_with_lenses_equals_an_object_fed_the_models_crops(aof, synth, gpu_device):
    """OpticalFlowBank, S = 5, 64 x 64 out of 96 x 80 sensor frames: setStreamLens on stream 0, setStreamWarp on streams
    1, 2 and 4 (stream 2's taken back with NULL before the first push, stream 3 never set), pushCamera() against an object
    whose push() is fed the model's crops: the published entries entry by entry on raw bytes.  The refusals leave the
    object as it was."""
    run = planes_run(synth, 36, every_other=4)
    a, b = (aof.OpticalFlowBank(FX, FY, RATE, W, H, S) for _ in range(2))
    for bank in (a, b):
        assert bank.engineOk(), bank.lastError()
        bank.setTimestampOffset(OFFSET)
    p = aof.px4flow_params(W, H)
    x0, y0 = PW // 2 - W // 2, PH // 2 - H // 2
    d = wref.designs(W, H, PW, PH, x0, y0)
    assert a.setStreamWarp(0, d["mirror"]) == EINVAL and a.setStreamLens(0, 60.0, 60.0, 48.0, 40.0) == EINVAL, "not before enabling"
    assert a.enableCamera(PW, PH, 100, 4, INTERVAL) == 0, a.lastError()
    lens = dict(fx=58.0, fy=58.5, cx=PW / 2.0 + 1.3, cy=PH / 2.0 - 0.7, k1=-0.28, k2=0.07, p1=0.002, p2=-0.001, k3=0.0)
    assert a.setStreamLens(0, **lens) == 0, a.lastError()
    assert a.setStreamLens(S, **lens) == EINVAL and a.setStreamLens(-1, **lens) == EINVAL and a.setStreamWarp(S, d["mirror"]) == EINVAL
    assert a.setStreamLens(1, **dict(lens, fx=0.0)) == EINVAL and a.setStreamLens(1, **dict(lens, fy=float("nan"))) == EINVAL and a.engineOk()
    assert a.setStreamBinning(1, 2) == EINVAL and a.engineOk(), "binning and warp do not compose"
    assert a.setStreamWarp(1, d["quarter-turn"]) == 0 and a.setStreamWarp(2, d["mirror"]) == 0 and a.setStreamWarp(2, None) == 0
    assert a.setStreamWarp(4, d["smooth-random"]) == 0
    none = d["identity"].copy()
    none[0, 0]["x"] = wref.NONE
    meshes = [aof.warp_mesh_from_lens(p, **lens), d["quarter-turn"], none, none, d["smooth-random"]]
    assert np.abs(wref.as_xy(meshes[0]) - wref.as_xy(wref.from_lens(W, H, wref.lens(w=W, h=H, **lens)))).max() <= 1
    recs = [csr.record(s * PW * PH, PW, PW, PH, x0, y0) for s in range(S)]
    entries_seen = 0
    for k in range(T):
        planes = run.frames[k]
        flat = planes.reshape(-1)
        crops = np.stack([wref.warp(flat, recs[s], csr.GREY8, meshes[s], W, H) for s in range(S)])
        assert np.array_equal(crops[3], planes[3, y0:y0 + H, x0:x0 + W]) and not np.array_equal(crops[0], planes[0, y0:y0 + H, x0:x0 + W])
        na, ea = a.pushCamera(planes, run.times[k], run.active[k], run.gyro[k])
        nb, eb = b.push(crops, run.times[k], run.active[k], run.gyro[k])
        assert na == nb >= 0, (k, a.lastError(), b.lastError())
        assert ea.tobytes() == eb.tobytes(), ("entries", k)
        entries_seen += na
    assert entries_seen >= 2 * S
    a.close(), b.close()
