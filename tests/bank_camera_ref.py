"""Inputs and expected outputs of the stream bank's camera push (aof_bank_push_camera_device; tests/test_bank_camera_ref.py,
tests/test_gpu_bank_camera.py): a bank_ref.Run turned into raw sensor frames, the exposure gate restated in integers, and
what the reference's per-frame loop leaves in front of and behind calcFlow() -- the centre crop and the masked histogram
with its mean sample value (orc.ingest, orc.exposure_msv; mainloop.cpp:197-220,273-274,295-298) and the published PX4Flow
gyro compensation of the pair's pixel record (orc.derotate).  Nothing here touches the GPU."""
import numpy as np

EXPOSURE_INTERVAL_US = 200_000        # mainloop.cpp:274
DEROTATE = (4.5, 0.3)                 # max_flow (search radius + 0.5 px), rate threshold (rad/s): at dt_s = 0.013 about one
                                      # gyro sample in three (sigma 0.004 rad) passes 0.3 * 0.013, the others leave the flow alone


def crop_origin(cam_w, cam_h, w, h):
    return cam_w // 2 - w // 2, cam_h // 2 - h // 2        # mainloop.cpp:295-296 (orc_crop_rect)


def mask_rect(w, h):
    """The exposure mask inside the crop: the centred 128 x 128 region, clipped (mainloop.cpp:203-206)."""
    mx0, my0 = w // 2 - 64, h // 2 - 64
    return max(mx0, 0), max(my0, 0), min(mx0 + 128, w), min(my0 + 128, h)


def add_saturated_patches(run):
    """Every fifth frame a stream is given carries a patch of value-255 pixels inside the mask: cv::calcHist drops them,
    so those histograms do not sum to the mask's size.  Changes run.frames in place (before any chain sees them)."""
    h, w = run.frames.shape[2:]
    mx0, my0, mx1, my1 = mask_rect(w, h)
    for s in range(run.S):
        n = 0
        for k in range(run.T):
            if not run.active[k, s]:
                continue
            n += 1
            if n % 5 == 0:
                y, x = my0 + (3 * n + s) % (my1 - my0 - 6), mx0 + (5 * n + 2 * s) % (mx1 - mx0 - 9)
                run.frames[k, s, y:y + 6, x:x + 9] = 255
    return run


class CameraRun:
    """The sensor frames of a Run: each active stream's frame embedded at the crop origin of a seeded-noise sensor
    frame; idle streams' sensor frames are noise.  Made tick by tick (a 640 x 480 run does not fit comfortably)."""

    def __init__(self, run, cam_w, cam_h, seed):
        self.run, self.cam_w, self.cam_h, self.seed = run, cam_w, cam_h, seed
        self.h, self.w = run.frames.shape[2:]
        assert self.w <= cam_w and self.h <= cam_h
        self.x0, self.y0 = crop_origin(cam_w, cam_h, self.w, self.h)

    def sensor(self, k):
        """[S, cam_h, cam_w] u8 of tick k."""
        rng = np.random.default_rng([self.seed, k])
        cam = rng.integers(0, 256, (self.run.S, self.cam_h, self.cam_w), dtype=np.uint8)
        for s in np.flatnonzero(self.run.active[k]):
            cam[s, self.y0:self.y0 + self.h, self.x0:self.x0 + self.w] = self.run.frames[k, s]
        return cam


def gate(times, active, interval, resets=None):
    """The exposure gate in integers (_exposure_update, mainloop.cpp:199-201,273-274): an active frame of 64-bit time t
    is due iff t >= next; a due frame sets next = t + interval.  Returns due [T, S] u8 and next [T, S] u64 (the gate
    behind tick k).  resets: {tick: mask [S]}: the gate of masked streams is 0 again before that tick."""
    T, S = active.shape
    due, after = np.zeros((T, S), np.uint8), np.zeros((T, S), np.uint64)
    nxt = [0] * S
    for k in range(T):
        if resets and k in resets:
            for s in np.flatnonzero(resets[k]):
                nxt[s] = 0
        for s in range(S):
            t = int(times[k, s])
            if active[k, s] and t >= nxt[s]:
                due[k, s] = 1
                nxt[s] = (t + interval) & 0xFFFFFFFFFFFFFFFF
            after[k, s] = nxt[s]
    return due, after


def expected_exposure(aof, orc, cam, run, k, due_k):
    """Tick k's exposure records [S] (aof.EXPOSURE_DTYPE): histogram and MSV of the due frames, zeros elsewhere.  Also
    asserts that the oracle's crop of every active stream's sensor frame IS the run's frame."""
    out = np.zeros(run.S, aof.EXPOSURE_DTYPE)
    h, w = run.frames.shape[2:]
    for s in np.flatnonzero(run.active[k]):
        crop, hist = orc.ingest(cam[s], w, h)
        assert np.array_equal(crop, run.frames[k, s]), ("the oracle's crop is the run's frame", k, s)
        if due_k[s]:
            out[s]["hist"], out[s]["msv"], out[s]["due"] = hist, np.float32(orc.exposure_msv(hist)), 1
    return out


def expected_derotated(orc, recs_k, gyro_k, fx, fy, derotate=DEROTATE, use_gyro=True):
    """Tick k's de-rotated pairs [S, 2] f32 from the oracle's records of the tick: orc.derotate on the pair's pixel
    record and the tick's gyro sample for every active frame that is not a first frame, 0, 0 elsewhere."""
    out = np.zeros((len(recs_k), 2), np.float32)
    for s, r in enumerate(recs_k):
        if r["quality"] == -2 or r["frame"] <= 1:       # idle, or the stream's first frame
            continue
        g = gyro_k[s] if use_gyro else np.zeros(4, np.float32)
        out[s] = orc.derotate(float(r["pixel"]["flow_x"]), float(r["pixel"]["flow_y"]), float(g[0]), float(g[1]), float(g[3]),
                              fx, fy, derotate[0], derotate[1])
    return out
