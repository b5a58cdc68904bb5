"""k_ingest.hip on the device at every trip, strip, flush, alignment and buffer edge (tests/ingest_ref.py names them
and tests/test_ingest_ref.py holds the case lists to them), byte for byte against the numpy model.  No tolerance anywhere.

Stateless form (k_ingest<false>): aof_ingest_batch_device called directly, every buffer pre-filled with 0xEE -- the
histogram included -- with guard bytes around it.
PYRAMID form (k_ingest<true>): through FlowEngine.sequence() with set_split_coarse(True), so that a short sequence plans
K1 and the ingest kernel takes K1's place; its level-1 frames and pixel sums are read out of the flow workspace inside the
sequence workspace and compared with the model directly.  That K1 did NOT run is shown by the context's own profiling
(aof_profile_count(AOF_K_PYRAMID) == 0 while the searches were counted); a crop the ingest kernel cannot serve shows the
same offsets filled by K1 (count >= 1), which validates where this file reads."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import ingest_ref as ref

pytestmark = pytest.mark.gpu

GUARD, FRONT, FILL, LIMIT_S = 64, 16, 0xEE, 120
FX, FY = 216.6677, 216.2457


@pytest.fixture(autouse=True)
def time_limit():
    """Every test's device work under a limit of its own.  The exit is deliberate: a step that hangs on the device ends
    the whole process at once (os._exit behind a traceback), so that nothing more is started on a card that hung -- the
    tests behind it go without a report, which is the lesser evil.  Each test runs a second or two; the limit is far
    above that and only a hang reaches it."""
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---------------------------------------------------------------------------------------------------------------
# the model's answers, computed once per case and shared (read-only)
# ---------------------------------------------------------------------------------------------------------------

_want = {}


def want_of(c):
    if c["id"] not in _want:
        frames = ref.frames_for(c)
        got = [ref.ingest(f, c["crop"][0], c["crop"][1]) for f in frames]
        crops, hists = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
        for a in (frames, crops, hists):
            a.setflags(write=False)
        _want[c["id"]] = (frames, crops, hists)
    return _want[c["id"]]


# ---------------------------------------------------------------------------------------------------------------
# stateless form
# ---------------------------------------------------------------------------------------------------------------

class Out:
    """A device buffer of `size` payload bytes at `shift` bytes behind a 16-byte aligned address, FRONT bytes in front of
    it and GUARD bytes behind, everything pre-filled with 0xEE."""

    def __init__(self, torch, dev, size, shift=0):
        self.size, self.off = size, FRONT + shift
        self.alloc = torch.full((FRONT + shift + size + GUARD,), FILL, dtype=torch.uint8, device=dev)
        assert self.alloc.data_ptr() % 16 == 0
        self.ptr = self.alloc.data_ptr() + self.off

    def refill(self):
        self.alloc.fill_(FILL)

    def read(self, what):
        """The payload, after checking that every byte around it is still 0xEE."""
        a = self.alloc.cpu().numpy()
        assert (a[:self.off] == FILL).all(), (what, "bytes in front of the buffer were written", np.flatnonzero(a[:self.off] != FILL))
        assert (a[self.off + self.size:] == FILL).all(), (what, "guard bytes behind the buffer were written")
        return a[self.off:self.off + self.size]


class Ingest:
    """One case's frames on the device and aof_ingest_batch_device on them."""

    def __init__(self, aof, dev, frames, camera_stride=None):
        import torch
        self.aof, self.torch, self.dev = aof, torch, dev
        self.n, self.cam_h, self.cam_w = frames.shape
        frame = self.cam_w * self.cam_h
        self.camera_stride = frame if camera_stride is None else camera_stride
        host = np.full(self.n * self.camera_stride + GUARD, FILL, np.uint8)
        for i, f in enumerate(frames):
            host[i * self.camera_stride:i * self.camera_stride + frame] = f.reshape(-1)
        self.camera = torch.from_numpy(host).to(dev)
        assert self.camera.data_ptr() % 16 == 0      # what ingest_ref.reach()'s source alignments assume

    def __call__(self, crop, what, *, want_crop=True, hist=None, want_hist=True, shift=0, cropped_stride=None, n=None,
                 camera_stride=None, expect=0):
        """Runs the entry point; returns (crops [n][h][w] or None, hist [n][10] or None, the raw crop payload, the Out
        of the histogram).  Guards are checked on the way."""
        torch = self.torch
        cw, ch = crop
        n = self.n if n is None else n
        stride = cw * ch if cropped_stride is None else cropped_stride
        cam_stride = self.camera_stride if camera_stride is None else camera_stride
        out = Out(torch, self.dev, max(n, 1) * max(stride, cw * ch), shift) if want_crop else None
        if hist is None and want_hist:
            hist = Out(torch, self.dev, 40 * max(n, 1))
        p = self.aof.IngestParams(self.cam_w, self.cam_h, cw, ch)
        rc = self.aof.lib.aof_ingest_batch_device(C.byref(p), self.camera.data_ptr(), cam_stride, n, out.ptr if out else None,
                                                  stride, hist.ptr if (hist and want_hist) else None,
                                                  torch.cuda.current_stream(self.dev).cuda_stream)
        assert rc == expect, (what, rc)
        torch.cuda.synchronize()
        raw = out.read(what + ": crop") if out else None
        crops = None
        if raw is not None and n:
            step = max(stride, cw * ch)
            crops = np.stack([raw[i * step:i * step + cw * ch].reshape(ch, cw) for i in range(n)])
        h = hist.read(what + ": histogram").view(np.uint32).reshape(-1, 10) if hist else None
        return crops, h, raw, hist


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError((what, "first of", len(bad), "differences at", tuple(int(v) for v in bad[0]),
                              "got", got[tuple(bad[0])], "want", want[tuple(bad[0])]))


@pytest.mark.parametrize("c", ref.STATELESS, ids=lambda c: c["id"])
def test_stateless_ingest_equals_the_model_in_every_output_form(aof, orc, gpu_device, c):
    """Both outputs, histogram-only, crop-only, and the histogram into a dirty buffer twice."""
    frames, crops, hists = want_of(c)
    run = Ingest(aof, gpu_device, frames)
    crop = c["crop"]
    # 1. both outputs (the histogram buffer starts as 0xEE: one strip must overwrite, several must zero first)
    gc, gh, _, hbuf = run(crop, "both")
    same(gc, crops, "crop")
    same(gh, hists, "histogram")
    for i in range(len(frames)):
        assert np.float32(aof.exposure_msv(gh[i])).tobytes() == np.float32(orc.exposure_msv(hists[i])).tobytes(), i
    # 4. once more into the same buffer, dirtied again in between
    hbuf.refill()
    gc2, gh2, _, _ = run(crop, "second run into the same histogram", hist=hbuf)
    same(gh2, hists, "histogram of the second run")
    same(gc2, crops, "crop of the second run")
    # 2. histogram-only (d_cropped = NULL)
    _, gh3, _, _ = run(crop, "histogram-only", want_crop=False)
    same(gh3, hists, "histogram-only")
    # 3. crop-only.  The entry point gets NULL for the histogram, so `idle` is a buffer it never heard of: that it stays
    #    0xEE is only a guard on neighbouring allocations, not a check of the histogram path
    idle = Out(run.torch, gpu_device, 40 * len(frames))
    gc4, gh4, _, _ = run(crop, "crop-only", hist=idle, want_hist=False)
    same(gc4, crops, "crop-only")
    assert (gh4.view(np.uint8) == FILL).all()


VEC_CAPABLE = [c for c in ref.STATELESS if c["crop"][0] % 16 == 0]


@pytest.mark.parametrize("c", VEC_CAPABLE, ids=lambda c: c["id"])
def test_stateless_ingest_follows_the_callers_buffers(aof, gpu_device, c):
    """crop_w % 16 == 0 with buffers that rule the vector stores out or move the frames apart."""
    frames, crops, hists = want_of(c)
    cw, ch = crop = c["crop"]
    cam_w, cam_h = c["cam"]
    n = len(frames)
    run = Ingest(aof, gpu_device, frames)
    # 5. d_cropped at an odd address: the scalar path; Out.read() checks the bytes in front of it
    gc, gh, _, _ = run(crop, "base + 1", shift=1)
    same(gc, crops, "crop at base + 1")
    same(gh, hists, "histogram at base + 1")
    # 6. padded strides on both sides; the gaps of the output stay 0xEE
    padded = Ingest(aof, gpu_device, frames, camera_stride=cam_w * cam_h + 37)
    stride = cw * ch + 8
    gc, gh, raw, _ = padded(crop, "padded strides", cropped_stride=stride)
    same(gc, crops, "crop with padded strides")
    same(gh, hists, "histogram with padded strides")
    gaps = np.concatenate([raw[i * stride + cw * ch:(i + 1) * stride] for i in range(n)])
    assert (gaps == FILL).all(), "gap bytes between the cropped frames were written"
    #    ... and the vector path itself from frames 37 bytes apart (no crop output: the buffer has no say)
    _, gh, _, _ = padded(crop, "histogram-only from a padded camera", want_crop=False)
    same(gh, hists, "histogram-only from a padded camera")
    #    ... and the vector stores into frames 16 bytes apart
    stride = cw * ch + 16
    gc, gh, raw, _ = padded(crop, "padded camera, 16-byte padded crop", cropped_stride=stride)
    same(gc, crops, "crop, vector path, padded")
    same(gh, hists, "histogram, vector path, padded")
    assert (np.concatenate([raw[i * stride + cw * ch:(i + 1) * stride] for i in range(n)]) == FILL).all()
    # 7. one frame with both strides 0
    gc, gh, _, _ = run(crop, "one frame, strides 0", n=1, cropped_stride=0, camera_stride=0)
    same(gc, crops[:1], "crop of one frame")
    same(gh, hists[:1], "histogram of one frame")
    # 8. no frames: returns 0, writes nothing
    _, gh, raw, _ = run(crop, "no frames", n=0)
    assert (raw == FILL).all() and (gh.view(np.uint8) == FILL).all()


# ---------------------------------------------------------------------------------------------------------------
# PYRAMID form
# ---------------------------------------------------------------------------------------------------------------

def align256(v):
    return (v + 255) // 256 * 256


def flow_ws_offset(aof, p, sp, n):
    """Where the flow workspace starts inside the sequence workspace -- not in the public layout, derived from it two
    ways that must agree: forwards over the scratch regions in front of it (aof_sequence.cpp: jump[2], hops[2], rank of
    4 (n + 1) bytes each, reached of n + 1), backwards from the end."""
    L = aof.sequence_layout(p, sp, n)
    FL = aof.workspace_layout(p, n - 1)
    forwards = 5 * align256(4 * (n + 1)) + align256(n + 1)
    backwards = L.total_bytes - L.scratch - align256(FL.total_bytes)
    assert forwards == backwards, ("the flow workspace is not where this test derives it", forwards, backwards)
    assert L.scratch + forwards + FL.total_bytes <= L.total_bytes
    return L, FL, L.scratch + forwards


def run_sequence(aof, orc, gpu_device, c, n, form, *, split_coarse, k1_runs):
    """One sequence() call on a workspace of 0xEE; every output of the ingest kernel (or of K1 where k1_runs) against the
    model, every flow record against the oracle on the model's crops."""
    import torch
    cw, ch = c["crop"]
    cam_w, cam_h = c["cam"]
    kw = ref.PYRAMID_FORMS[form]
    p = aof.px4flow_params(cw, ch, **kw)
    two, eq = p.pyramid_levels == 2, p.mean_subtract != 0
    frames = ref.sequence_frames_for(c, n)
    crops = ref.crops_of(frames, c["crop"])
    hists = np.stack([ref.ingest(f, cw, ch)[1] for f in frames])
    l1, sums = ref.pyramid(crops)

    eng = aof.FlowEngine(p, 0)
    try:
        if split_coarse:
            eng.set_split_coarse(True)
        sp = aof.sequence_params(cam_w, cam_h, cw, ch, FX, FY, 15, 5_000_000, 1, 100, 0)
        L, FL, fws = flow_ws_offset(aof, p, sp, n)
        ws = torch.full((L.total_bytes + GUARD,), FILL, dtype=torch.uint8, device=gpu_device)
        cam = torch.from_numpy(frames).to(gpu_device)
        assert cam.data_ptr() % 16 == 0 and ws.data_ptr() % 256 == 0
        times = torch.arange(n, dtype=torch.int64, device=gpu_device) * 13333
        eng.set_profiling(True)
        eng.sequence(sp, cam, times, workspace=ws[:L.total_bytes])
        torch.cuda.synchronize()
        k1 = aof.lib.aof_profile_count(eng._ctx, aof.K_PYRAMID)
        searches = aof.lib.aof_profile_count(eng._ctx, aof.K_SEARCH)
        eng.set_profiling(False)
        out = eng.sequence_outputs(sp, ws[:L.total_bytes], L, n)
        raw = ws.cpu().numpy()
    finally:
        eng.close()

    what = (c["id"], form, n)
    assert (raw[L.total_bytes:] == FILL).all(), (what, "guard bytes behind the workspace were written")
    assert searches >= 1, (what, "profiling does not see the sequence path")
    if k1_runs:
        assert k1 >= 1, (what, "K1 was expected to run")
    else:
        assert k1 == 0, (what, "K1 ran: the ingest kernel did not take its place", k1)
    assert out["status"] == 0, what
    same(out["cropped"], crops, what + ("cropped",))
    same(out["exposure"], hists, what + ("exposure",))
    po = orc.params_from(p)
    assert len(out["flows"]) == n - 1
    for k in range(n - 1):
        assert out["flows"][k].tobytes() == orc.flow_pair(po, crops[k], crops[k + 1])["flow"].tobytes(), what + ("flow", k)
    # K1's outputs, wherever they came from
    got_sums = raw[fws + FL.sums:fws + FL.sums + 16 * (n - 1)]
    if eq:   # (a one-level form gets the level-1 column as well: the kernel adds pyr_sum1 whether or not it stores level 1)
        same(got_sums.view(np.uint32).reshape(n - 1, 2, 2), sums, what + ("sums",))
    else:    # sums == nullptr: the region is nobody's
        assert (got_sums == FILL).all(), what + ("the pixel sums were written without mean_subtract",)
    if two:
        l1_frame = (cw // 2) * (ch // 2)
        got_l1 = raw[fws + FL.l1_prev:fws + FL.l1_prev + n * l1_frame].reshape(n, ch // 2, cw // 2)
        same(got_l1, l1, what + ("level-1 frames",))
        assert fws + FL.l1_prev + n * l1_frame <= fws + FL.l1_blocks
        assert (raw[fws + FL.l1_prev + n * l1_frame:fws + FL.l1_blocks] == FILL).all(), what + ("bytes behind the last level-1 frame",)
    else:
        assert FL.l1_cur == FL.l1_prev or FL.l1_blocks == FL.l1_prev     # no room, nothing to write
    return out, k1


@pytest.mark.parametrize("n", ref.PYRAMID_FRAMES, ids=lambda n: f"n{n}")
@pytest.mark.parametrize("form", list(ref.PYRAMID_FORMS))
@pytest.mark.parametrize("c", ref.PYRAMID, ids=lambda c: c["id"])
def test_pyramid_ingest_leaves_what_k1_would(aof, orc, gpu_device, c, form, n):
    assert ref.reach(c["cam"], c["crop"])["pyramid_supported"]
    run_sequence(aof, orc, gpu_device, c, n, form, split_coarse=True, k1_runs=False)


def test_pyramid_ingest_on_the_production_route(aof, orc, gpu_device):
    """More than 128 pairs, two levels, no split_coarse: how a long recording gets into the same kernel."""
    run_sequence(aof, orc, gpu_device, ref.PYRAMID_LONG, ref.PYRAMID_LONG_FRAMES, "l1_and_sums", split_coarse=False, k1_runs=False)


@pytest.mark.parametrize("n", ref.PYRAMID_FRAMES, ids=lambda n: f"n{n}")
def test_k1_fills_the_same_offsets_where_the_ingest_kernel_cannot_serve(aof, orc, gpu_device, n):
    """A crop width that is no multiple of 16: the stateless ingest and K1 itself run, and K1's outputs are found --
    and equal the model -- exactly where the tests above read the ingest kernel's."""
    c = ref.K1_VALIDATION
    assert not ref.reach(c["cam"], c["crop"])["pyramid_supported"]
    run_sequence(aof, orc, gpu_device, c, n, "l1_and_sums", split_coarse=True, k1_runs=True)
