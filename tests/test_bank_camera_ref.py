"""The host-only side of the stream bank's camera push (include/aof.h, "the stream bank with sensor frames"): the
camera layout, the two new structs, what aof_bank_camera_layout and the entry point refuse without a context, the
exposure gate restated on literal time stamps, hand MSVs, and the input recipe of tests/bank_camera_ref.py -- no device."""
import ctypes as C

import numpy as np
import pytest

import bank_camera_ref as cref
import bank_ref as ref

EINVAL = -22


def test_structs_match_the_header(aof):
    assert C.sizeof(aof.BankCamera) == 48                  # 4 i32, i64, u32, u8 + pad, 4 f32
    assert aof.BankCamera.camera_stride.offset == 16 and aof.BankCamera.exposure_interval_us.offset == 24
    assert aof.BankCamera.derotate.offset == 28 and aof.BankCamera.derotate_params.offset == 32
    assert aof.EXPOSURE_DTYPE.itemsize == 48               # sizeof(aof_exposure_record)
    assert aof.EXPOSURE_DTYPE.fields["msv"][1] == 40 and aof.EXPOSURE_DTYPE.fields["due"][1] == 44
    assert aof.BANK_STATE_BYTES == 64                      # the gate took the record's spare bytes


def test_header_declares_and_the_documents_list_the_camera_push(aof):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "aof.h")).read()
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    for name in ("aof_bank_camera_layout", "aof_bank_push_camera_device"):
        assert re.search(r"\bint " + name + r"\(", text), name
        assert name in aof.EXPORTS and name in doc
    assert "#define AOF_VERSION 102" in text


@pytest.mark.parametrize("size,sensor,kw", [((64, 64), (320, 240), {}), ((64, 64), (322, 242), {}), ((64, 64), (64, 64), {}),
                                            ((128, 128), (640, 480), dict(pyramid_levels=2, mean_subtract=1)),
                                            ((192, 160), (256, 224), None), ((160, 128), (224, 192), dict(tile=16, search=8))])
def test_camera_layout_keeps_the_bank_layout_and_adds_staging(aof, size, sensor, kw):
    w, h = size
    p = aof.default_params(w, h, subpixel=1) if kw is None else (
        aof.px4flow_params(w, h, **kw) if "tile" not in kw else aof.default_params(w, h, **kw))
    for S in (1, 2, 24, 300, 4096):
        for stride in (0, w * h, w * h + 48):
            for cam_stride in (0, sensor[0] * sensor[1], sensor[0] * sensor[1] + 37):
                bp = aof.bank_params(n_streams=S, frame_stride=stride)
                cam = aof.bank_camera_params(sensor[0], sensor[1], w, h, camera_stride=cam_stride)
                L0 = aof.bank_layout(p, bp)
                L, staging = aof.bank_camera_layout(p, bp, cam)
                assert (L.frames, L.state, L.scratch) == (L0.frames, L0.state, L0.scratch)
                assert staging == L0.total_bytes and staging % 256 == 0        # behind everything the plain bank has
                # u8 [S][frame_stride], then u32 [S][10]
                assert L.total_bytes - staging >= S * (stride or w * h) + 40 * S and L.total_bytes % 256 == 0


def test_camera_layout_refuses_bad_arguments(aof):
    p = aof.px4flow_params(64, 64)
    bp = aof.bank_params(n_streams=4)
    call = aof.lib.aof_bank_camera_layout
    L, st = aof.BankLayout(), C.c_size_t()
    ok = aof.bank_camera_params(320, 240, 64, 64)
    assert call(C.byref(p), C.byref(bp), C.byref(ok), C.byref(L), C.byref(st)) == 0
    assert call(None, C.byref(bp), C.byref(ok), C.byref(L), C.byref(st)) == EINVAL
    assert call(C.byref(p), None, C.byref(ok), C.byref(L), C.byref(st)) == EINVAL
    assert call(C.byref(p), C.byref(bp), None, C.byref(L), C.byref(st)) == EINVAL
    assert call(C.byref(p), C.byref(bp), C.byref(ok), None, C.byref(st)) == EINVAL
    assert call(C.byref(p), C.byref(bp), C.byref(ok), C.byref(L), None) == EINVAL
    bad = [aof.bank_camera_params(320, 240, 64, 48),                      # crop size != the context's frame size
           aof.bank_camera_params(320, 240, 128, 128),
           aof.bank_camera_params(64, 48, 64, 64),                        # crop larger than the sensor frame
           aof.bank_camera_params(32, 240, 64, 64),
           aof.bank_camera_params(320, 240, 64, 64, camera_stride=320 * 240 - 1),   # below one sensor frame
           aof.bank_camera_params(320, 240, 64, 64, camera_stride=-76800)]
    for cam in bad:
        assert call(C.byref(p), C.byref(bp), C.byref(cam), C.byref(L), C.byref(st)) == EINVAL
        with pytest.raises(aof.AofError):
            aof.bank_camera_layout(p, bp, cam)
    # everything aof_bank_layout refuses
    for kw in (dict(n_streams=0), dict(n_streams=4, frame_stride=4096 + 8), dict(n_streams=4, focal_x=0.0)):
        assert call(C.byref(p), C.byref(aof.bank_params(**kw)), C.byref(ok), C.byref(L), C.byref(st)) == EINVAL, kw
    buf = np.zeros(1 << 16, np.uint8)                                     # the entry point checks the context first
    assert aof.lib.aof_bank_push_camera_device(None, C.byref(bp), C.byref(ok), buf.ctypes.data, buf.ctypes.data, None, None,
                                               buf.ctypes.data, buf.size, buf.ctypes.data, None, None, None, None, None) == EINVAL


def test_the_gate_restated_on_literal_time_stamps():
    times = np.array([[0], [150_000], [200_000], [399_999], [400_000], [(1 << 32) + 5]], np.int64)
    active = np.ones((6, 1), np.uint8)
    due, after = cref.gate(times, active, 200_000)
    assert due[:, 0].tolist() == [1, 0, 1, 0, 1, 1]
    assert after[:, 0].tolist() == [200_000, 200_000, 400_000, 400_000, 600_000, (1 << 32) + 200_005]
    due0, _ = cref.gate(times, active, 0)
    assert due0[:, 0].tolist() == [1] * 6                                 # interval 0: every frame
    # an idle tick neither is due nor moves the gate; a reset makes the next frame due
    active[2, 0] = 0
    due, after = cref.gate(times, active, 200_000, resets={4: np.array([1], np.uint8)})
    assert due[:, 0].tolist() == [1, 0, 0, 1, 1, 1] and after[2, 0] == 200_000 and after[3, 0] == 599_999


def test_hand_msv(aof, orc):
    hist = np.zeros(10, np.uint32)
    hist[4] = 16384                                                       # all mask pixels in bin 4
    assert aof.exposure_msv(hist) == 5.0 == orc.exposure_msv(hist)
    crop = np.full((64, 64), 254, np.uint8)                               # a 64 x 64 crop, every pixel in bin 9
    _, h = orc.ingest(crop, 64, 64)
    assert h.tolist() == [0] * 9 + [4096]
    assert aof.exposure_msv(h) == 2.5 == orc.exposure_msv(h)              # 4 096 * 10 / 16 384
    assert orc.ingest(np.full((64, 64), 255, np.uint8), 64, 64)[1].sum() == 0   # calcHist drops 255


def test_the_recipe_embeds_the_frames_and_saturates_every_fifth(aof, orc, synth):
    run = cref.add_saturated_patches(ref.make_run(synth, 64, 64, 6, 24, 71))
    cam = cref.CameraRun(run, 322, 242, 71)
    assert (cam.x0, cam.y0) == (129, 89)                                  # a crop origin on an odd byte
    due, _ = cref.gate(run.times, run.active, 0)
    short = 0
    for k in range(run.T):
        sensor = cam.sensor(k)
        e = cref.expected_exposure(aof, orc, sensor, run, k, due[k])       # (asserts crop == frame)
        act = run.active[k] == 1
        assert (e["due"] == run.active[k]).all() and not e[~act]["hist"].any()
        short += int((e[act]["hist"].sum(1) < 4096).sum())
        assert np.array_equal(sensor, cam.sensor(k)), "deterministic per tick"
    assert short >= run.S * 2, "saturated patches: histograms that do not sum to the mask's size"
