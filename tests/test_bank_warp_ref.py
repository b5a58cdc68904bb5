"""The warp rule on the CPU (include/aof.h, "the stream bank with a lens"): single pixels worked by hand, the identity
mesh against slicing, aof_warp_host -- the header the kernel compiles, built for the host -- against the numpy model
(tests/bank_warp_ref.py) on every designed mesh and every AOF_PIXEL_*, and the lens helper against the model's doubles."""
import numpy as np
import pytest

import bank_warp_ref as wref
import crop_source_ref as csr
import warp_plan_ref as wplan

FORMATS = (csr.GREY8, csr.LUMA16_LO, csr.LUMA16_HI, csr.Y10, csr.Y12, csr.Y14, csr.Y10P, csr.Y12P)
# crop w, h, plane width, height: the GPU tests' sizes (16-byte stores; a lane per pixel; two strips), then the edges of the
# warp launch's plan and of the warped tick's (tests/warp_plan_ref.py): the reference the GPU tests lean on is held to the host
# build at every size they run.  The very wide ones take three designs and two formats.
SIZES = tuple(dict.fromkeys([(64, 64, 96, 80), (20, 12, 44, 36), (16, 136, 40, 150)] + [(c["w"], c["h"], *c["plane"]) for c in wplan.WARP_CASES] +
                            [(c["w"], c["h"], c["w"] + 32, c["h"] + 16) for c in wplan.TICK_CASES]))
WIDE = {(c["w"], c["h"], *c["plane"]) for c in wplan.WARP_CASES if c["wide"]}
WIDE_FORMATS = (csr.GREY8, csr.Y10P)
RUNS = [(size, fmt) for size in SIZES for fmt in FORMATS if size not in WIDE or fmt in WIDE_FORMATS]


def one_pixel(aof, plane, X, Y):
    """Crop pixel (0, 0) of a 1 x 1 crop whose four nodes all say (X, Y), from the library and from the model."""
    plane = np.asarray(plane, np.uint8)
    H, W = plane.shape
    rec = csr.record(0, W, W, H, 0, 0)
    mesh = wref.as_points(np.full((2, 2, 2), (X, Y), np.int64))
    got, hist = aof.warp_host(plane.reshape(-1), rec, 1, 1, mesh)
    want = wref.warp(plane.reshape(-1), rec, csr.GREY8, mesh, 1, 1)
    assert got.shape == (1, 1) and got[0, 0] == want[0, 0]
    assert hist.tolist() == wref.histogram(want).tolist()
    return int(got[0, 0])


def test_single_pixels_worked_by_hand(aof):
    assert one_pixel(aof, [[10, 21]], 16, 0) == 16                      # (10 + 21) / 2 = 15.5, half up
    assert one_pixel(aof, [[10, 21]], 8, 0) == 13                       # 10 * 24/32 + 21 * 8/32 = 12.75
    assert one_pixel(aof, [[10], [21]], 0, 16) == 16
    assert one_pixel(aof, [[0, 100], [200, 255]], 16, 16) == 139        # 555 / 4 = 138.75
    assert one_pixel(aof, [[0, 100], [200, 255]], 31, 1) == 102         # (0 + 100*31*31 + 200*1*1 + 255*31*1 + 512) >> 10 = 104717 >> 10
    assert one_pixel(aof, [[255, 255], [255, 255]], 13, 29) == 255      # weights sum to 1024: no value leaves 0..255


def test_the_second_tap_is_clamped_at_the_last_pixel(aof):
    plane = [[1, 2, 3, 250]]
    assert one_pixel(aof, plane, 3 * 32, 0) == 250                       # X = xmax * 32: xi = xmax, x1 = xmax
    assert one_pixel(aof, plane, 3 * 32 - 16, 0) == (3 + 250 + 1) // 2   # half a pixel in front of it: both taps
    assert one_pixel(aof, [[7], [9], [200]], 0, 2 * 32) == 200           # the same on y


def test_nodes_are_clamped_from_below_and_from_above(aof):
    plane = [[11, 12, 13], [21, 22, 23]]
    assert one_pixel(aof, plane, -1, -1) == 11
    assert one_pixel(aof, plane, wref.I32_MIN + 1, 32) == 21
    assert one_pixel(aof, plane, wref.I32_MAX, wref.I32_MAX) == 23
    assert one_pixel(aof, plane, 2 * 32 + 1, 0) == 13                    # one unit over: clamped to xmax * 32, no fraction left
    assert one_pixel(aof, plane, 32, 10 ** 9) == 22


def test_a_plane_wider_than_the_coordinate_range_replicates_pixel_32767(aof):
    plane = np.zeros((1, 32770), np.uint8)
    plane[0, 32766:] = (5, 77, 99, 99)
    assert one_pixel(aof, plane, wref.I32_MAX, 0) == 77
    assert one_pixel(aof, plane, 32767 * 32 - 16, 0) == (5 + 77 + 1) // 2


def frame_of(fmt, w, h, width, height, seed):
    """A noise buffer holding one plane of `fmt` with a padded pitch at a non-zero offset, its record with the centred
    plain crop, and the designs for it."""
    rb = csr.row_bytes(fmt, width)
    pitch, offset = rb + 7, 37
    rec = csr.record(offset, pitch, width, height, width // 2 - w // 2, height // 2 - h // 2)
    buf = np.random.default_rng([seed, fmt]).integers(0, 256, offset + csr.extent(rec, fmt), dtype=np.uint8)
    assert csr.valid(rec, fmt, 1, w, h, len(buf))
    return buf, rec, wref.designs(w, h, width, height, int(rec["x0"]), int(rec["y0"]))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s[:2])
def test_identity_mesh_equals_slicing(aof, size):
    w, h, width, height = size
    plane = np.random.default_rng(size).integers(0, 256, (height, width), dtype=np.uint8)
    rec = csr.record(0, width, width, height, 5, 3)
    mesh = wref.identity(w, h, 5, 3)
    got, hist = aof.warp_host(plane.reshape(-1), rec, w, h, mesh)
    assert np.array_equal(got, plane[3:3 + h, 5:5 + w])
    assert np.array_equal(wref.warp(plane.reshape(-1), rec, csr.GREY8, mesh, w, h), plane[3:3 + h, 5:5 + w])
    assert hist.tolist() == wref.histogram(plane[3:3 + h, 5:5 + w]).tolist()
    p = aof.px4flow_params(64, 64)
    p.width, p.height = w, h
    assert aof.warp_mesh_size(p) == wref.mesh_size(w, h)
    assert aof.warp_mesh_identity(p, 5, 3).tobytes() == mesh.tobytes()
    none = mesh.copy()
    none[0, 0]["x"] = wref.NONE                                          # not warped: the record's plain crop, whatever else the mesh says
    none[1:, 1:]["y"] = 12345
    got, _ = aof.warp_host(plane.reshape(-1), rec, w, h, none)
    assert np.array_equal(got, plane[3:3 + h, 5:5 + w])


@pytest.mark.parametrize("size,fmt", RUNS, ids=["%dx%d-%d" % (s[0], s[1], f) for s, f in RUNS])
def test_warp_host_is_the_model_on_every_design(aof, size, fmt):
    w, h, width, height = size
    buf, rec, designs = frame_of(fmt, w, h, width, height, 11)
    assert len(designs) == 10
    if size in WIDE:
        designs = {k: designs[k] for k in wplan.WIDE_DESIGNS + ("identity",)}
    seen = set()
    for name, mesh in designs.items():
        want = wref.warp(buf, rec, fmt, mesh, w, h)
        got, hist = aof.warp_host(buf, rec, w, h, mesh, format=fmt)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:3])
        assert hist.tolist() == wref.histogram(want).tolist(), name
        seen.add(want.tobytes())
    assert len(seen) >= len(designs) - 1, "the designs are different images"
    assert np.array_equal(wref.warp(buf, rec, fmt, designs["identity"], w, h), csr.crop(buf, rec, fmt, 1, w, h))
    assert aof.warp_host(buf, rec, w, h, designs["barrel"], format=fmt, camera_bytes=len(buf) - 1) is None, "an invalid record: nothing is read"


def test_the_lens_helper_is_the_model_within_one_unit(aof):
    """Both sides are IEEE doubles; a compiler may contract a multiply and an add into one rounding, which can move a value
    across ONE boundary of the final floor."""
    for w, h, width, height in SIZES + ((128, 128, 640, 480),):
        p = aof.px4flow_params(64, 64)
        p.width, p.height = w, h
        for k1, k2 in ((-0.28, 0.07), (0.11, -0.02), (0.0, 0.0)):
            l = wref.barrel(w, h, width, height, k1, k2)
            got = aof.warp_mesh_from_lens(p, **l)
            want = wref.from_lens(w, h, l)
            assert got.shape == want.shape
            assert np.abs(wref.as_xy(got) - wref.as_xy(want)).max() <= 1, (w, h, k1)
        huge = aof.warp_mesh_from_lens(p, 1e300, 1e300, 0.0, 0.0, k1=1.0, out_fx=1.0, out_fy=1.0)       # saturates, never wraps
        assert set(np.unique(wref.as_xy(huge))) <= {wref.I32_MIN + 1, wref.I32_MIN, 0, wref.I32_MAX}


def test_without_coefficients_and_with_equal_cameras_the_lens_is_the_identity(aof):
    for w, h, width, height in SIZES:
        p = aof.px4flow_params(64, 64)
        p.width, p.height = w, h
        x0, y0 = width // 2 - w // 2, height // 2 - h // 2
        # the sensor camera's principal point is the virtual one's, moved by the crop origin
        got = aof.warp_mesh_from_lens(p, 70.0, 70.0, x0 + w / 2.0, y0 + h / 2.0)
        assert got.tobytes() == wref.identity(w, h, x0, y0).tobytes() == aof.warp_mesh_identity(p, x0, y0).tobytes()
