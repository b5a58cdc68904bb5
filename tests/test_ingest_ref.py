"""The numpy model of frame ingest (tests/ingest_ref.py) and the case lists of tests/test_gpu_ingest_edges.py, without
a device: the model equals the oracle on every geometry and frame family the device tests use, every case reaches the
path of k_ingest.hip it is listed for, and the lists together reach every path -- a path nobody reaches fails here."""
import numpy as np
import pytest

import ingest_ref as ref
import npref

ALL_PYRAMID = ref.PYRAMID + [ref.PYRAMID_LONG]


@pytest.mark.parametrize("c", ref.STATELESS, ids=lambda c: c["id"])
def test_model_equals_the_oracle_on_every_stateless_case(orc, c):
    frames = ref.frames_for(c)
    assert 3 <= len(frames) <= 4
    cw, ch = c["crop"]
    mx0, my0, mx1, my1 = ref.reach(c["cam"], c["crop"])["mask"]
    for i, f in enumerate(frames):
        crop, hist = ref.ingest(f, cw, ch)
        ocrop, ohist = orc.ingest(f, cw, ch)
        assert crop.shape == (ch, cw) and np.array_equal(crop, ocrop), i
        assert hist.dtype == np.uint32 and np.array_equal(hist, ohist), (i, hist, ohist)
        assert hist.sum() == (mx1 - mx0) * (my1 - my0) - np.count_nonzero(crop[my0:my1, mx0:mx1] == 255)
    # the families are what they say: nothing counts / one bin / dropped values inside the mask
    h37 = ref.ingest(frames[-2], cw, ch)[1]
    assert h37[1] == (mx1 - mx0) * (my1 - my0) and h37.sum() == h37[1]          # 37 * 10 / 255 = 1.45
    if len(frames) == 4:
        assert ref.ingest(frames[1], cw, ch)[1].sum() == 0
    band = ref.ingest(frames[-1], cw, ch)
    assert np.count_nonzero(band[0][my0:my1, mx0:mx1] == 255) >= mx1 - mx0


@pytest.mark.parametrize("c", ALL_PYRAMID + [ref.K1_VALIDATION], ids=lambda c: c["id"])
def test_model_equals_the_oracle_on_every_pyramid_case(orc, c):
    cw, ch = c["crop"]
    lengths = ref.PYRAMID_FRAMES + ((ref.PYRAMID_LONG_FRAMES,) if c is ref.PYRAMID_LONG else ())   # (the contents depend on n)
    for n in lengths:
        frames = ref.sequence_frames_for(c, n)
        crops = ref.crops_of(frames, c["crop"])
        for f, crop in zip(frames, crops):
            ocrop, ohist = orc.ingest(f, cw, ch)
            assert np.array_equal(crop, ocrop) and np.array_equal(ref.ingest(f, cw, ch)[1], ohist)
        l1, sums = ref.pyramid(crops)
        assert l1.shape == (n, ch // 2, cw // 2) and l1.dtype == np.uint8
        assert sums.shape == (n - 1, 2, 2) and sums.dtype == np.uint32
        for k in range(n):
            assert np.array_equal(l1[k], orc.pyramid_down(crops[k])), k
            assert np.array_equal(l1[k], npref.pyramid_down(crops[k])), k
        for k in range(n - 1):
            for side in range(2):
                assert sums[k, side, 0] == crops[k + side].sum(dtype=np.uint64)
                assert sums[k, side, 1] == orc.pyramid_down(crops[k + side]).sum(dtype=np.uint64)
        # a scene and the same scene moved: the pair the flow has something to find in
        assert np.array_equal(frames[1], np.roll(frames[0], (-1, 2), (0, 1)))


def test_pyramid_model_by_hand():
    crops = np.array([[[1, 2, 255, 255], [3, 4, 255, 254]], [[0, 0, 0, 1], [0, 1, 1, 1]], [[9, 9, 9, 9], [9, 9, 9, 9]]], np.uint8)
    l1, sums = ref.pyramid(crops)
    assert l1.tolist() == [[[3, 255]], [[0, 1]], [[9, 9]]]      # (10 + 2) >> 2 = 3; (1019 + 2) >> 2 = 255; (1 + 2) >> 2 = 0; (3 + 2) >> 2 = 1
    assert sums.tolist() == [[[1029, 258], [4, 1]], [[4, 1], [72, 18]]]


@pytest.mark.parametrize("c", ref.STATELESS, ids=lambda c: c["id"])
def test_every_stateless_case_reaches_the_paths_it_is_listed_for(c):
    r = ref.reach(c["cam"], c["crop"])
    assert c["paths"], "a case without a path has no reason to be in the list"
    for name in c["paths"]:
        assert ref.STATELESS_PATHS[name](r), (c["id"], name, r)
    if c["crop"][0] % 16 == 0:   # what the device test's base + 1 and odd-stride forms rely on
        assert r["vec"] and not ref.reach(c["cam"], c["crop"], dst_aligned=False)["vec"]
        assert ref.reach(c["cam"], c["crop"], dst_aligned=False, want_crop=False)["vec"]   # histogram-only: the buffer has no say


@pytest.mark.parametrize("c", ALL_PYRAMID, ids=lambda c: c["id"])
def test_every_pyramid_case_reaches_the_paths_it_is_listed_for(c):
    r = ref.reach(c["cam"], c["crop"])
    assert r["vec"] and r["pyramid_supported"], c["id"]
    assert c["paths"]
    for name in c["paths"]:
        assert ref.PYRAMID_PATHS[name](r), (c["id"], name, r)


def test_reach_on_the_geometries_worked_out_by_hand():
    r = ref.reach((2048, 128), (2048, 128))
    assert (r["pieces"], r["items"], r["trips"], r["rounds"], r["flushes_in_loop"]) == (128, [16384], [16], [64], [1])
    r = ref.reach((4096, 192), (4096, 192))
    assert (r["pieces"], r["nstrips"], r["rounds"], r["flushes_in_loop"]) == (256, 2, [128, 64], [2, 1])
    r = ref.reach((640, 480), (640, 480))          # the widest crop of tests/test_ingest.py: 20 rounds, no flush in the loop
    assert r["rounds"] == [20, 20, 20, 16] and r["flushes_in_loop"] == [0, 0, 0, 0]   # (the last strip has 96 rows)
    r = ref.reach((259, 201), (192, 160))
    assert (r["pieces"], r["items"], r["trips"], r["ragged_last_trip"]) == (12, [1536, 384], [2, 1], [True, True])
    assert (r["x0"], r["y0"]) == (33, 20) and r["src_align"] == list(range(16))
    r = ref.reach((640, 480), (400, 258))
    assert (r["pieces"], r["strip_rows"], r["items"], r["trips"]) == (25, [128, 128, 2], [3200, 3200, 50], [4, 4, 1])
    r = ref.reach((322, 242), (128, 128))
    assert r["x0"] == 97 and r["src_align"] == [1, 3, 5, 7, 9, 11, 13, 15]
    r = ref.reach((323, 243), (144, 96))
    assert r["mask"] == (8, 0, 136, 96) and r["pieces"] == 9 and r["mask_edge_in_piece"]
    r = ref.reach((320, 240), (128, 128))          # every vec geometry of test_gpu_ingest_parity: one even alignment
    assert r["src_align"] == [0] and r["items"] == [1024] and r["ragged_last_trip"] == [False]
    for cam, crop in (((640, 480), (128, 128)), ((160, 120), (64, 64)), ((1280, 960), (256, 192)), ((320, 240), (144, 136)), ((640, 480), (400, 128))):
        assert [a % 8 for a in ref.reach(cam, crop)["src_align"]] == [0], (cam, crop)
    assert not ref.reach((322, 242), (100, 90))["vec"]
    assert not ref.reach((100, 90), (100, 90))["pyramid_supported"] and not ref.reach((64, 64), (64, 63))["pyramid_supported"]


def test_the_case_lists_reach_every_path_between_them():
    """The census: every path named in the model is claimed by a case (and the tests above hold each claim to reach())."""
    for paths, cases in ((ref.STATELESS_PATHS, ref.STATELESS), (ref.PYRAMID_PATHS, ALL_PYRAMID)):
        claimed = {name for c in cases for name in c["paths"]}
        assert claimed <= set(paths), claimed - set(paths)
        assert not set(paths) - claimed, f"paths no case reaches: {sorted(set(paths) - claimed)}"
        reached = {name for c in cases for name, pred in paths.items() if pred(ref.reach(c["cam"], c["crop"]))}
        assert reached == set(paths)
    # forms the device test runs on top of the geometries
    assert set(ref.PYRAMID_FORMS) == {"l1_and_sums", "l1_only", "sums_only"}
    assert ref.PYRAMID_FORMS["l1_only"].get("mean_subtract", 0) == 0 and ref.PYRAMID_FORMS["sums_only"].get("pyramid_levels", 1) == 1
    assert 2 in ref.PYRAMID_FRAMES and max(ref.PYRAMID_FRAMES) >= 4 and ref.PYRAMID_LONG_FRAMES - 1 > 128
    assert len({c["id"] for c in ref.STATELESS}) == len(ref.STATELESS) and len({c["id"] for c in ref.PYRAMID}) == len(ref.PYRAMID)
    # the largest input of the device tests: three frames of 4096 x 192
    sizes = [ref.frames_for(c).nbytes for c in ref.STATELESS]
    assert max(sizes) == 3 * 4096 * 192


def test_the_parameter_check_accepts_every_pyramid_case_in_every_form(aof):
    """PX4 parameters at the crop size, as the device test creates its contexts.  48 x 32 (three pieces at the smallest
    height first proposed) is refused at two levels, and so is 48 x 36: 48 x 38 is the smallest that is not."""
    for c in ALL_PYRAMID + [ref.K1_VALIDATION]:
        for form, kw in ref.PYRAMID_FORMS.items():
            assert aof.check_params(aof.px4flow_params(c["crop"][0], c["crop"][1], **kw)) == 0, (c["id"], form)
    assert aof.check_params(aof.px4flow_params(48, 32, pyramid_levels=2)) == -22
    assert aof.check_params(aof.px4flow_params(48, 36, pyramid_levels=2)) == -22
    assert aof.check_params(aof.px4flow_params(48, 38, pyramid_levels=2)) == 0
    assert ref.K1_VALIDATION["crop"][0] % 16 != 0     # the ingest kernel's PYRAMID form cannot serve it: K1 runs
