"""The numpy model of the stream bank's warp (include/aof.h, "the stream bank with a lens"): the rule in 64-bit integers
that cannot wrap, the lens helper in Python floats (IEEE doubles, every operation rounded on its own), and the designed
meshes the CPU and GPU tests share.  A plane's grey values come through crop_source_ref.grey: the header's table of pixel
formats, byte by byte.  Nothing here touches the GPU or the library under test."""
import math

import numpy as np

import crop_source_ref as csr

POINT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4")])
CELL, FRAC, ONE, LAST_MAX = 8, 5, 32, 32767
NONE = -2**31
I32_MIN, I32_MAX = -2**31, 2**31 - 1
MASK = 128


def mesh_size(w, h):
    return (w + 7) // 8 + 1, (h + 7) // 8 + 1


def as_points(xy):
    """[ny, nx, 2] integers -> [ny, nx] of POINT_DTYPE (values must be int32)."""
    xy = np.asarray(xy, np.int64)
    assert (xy >= I32_MIN).all() and (xy <= I32_MAX).all()
    out = np.zeros(xy.shape[:2], POINT_DTYPE)
    out["x"], out["y"] = xy[..., 0], xy[..., 1]
    return out


def as_xy(points):
    points = np.asarray(points, POINT_DTYPE)
    return np.stack([points["x"].astype(np.int64), points["y"].astype(np.int64)], axis=-1)


def identity(w, h, x0, y0):
    nx, ny = mesh_size(w, h)
    cy, cx = np.mgrid[0:ny, 0:nx]
    return as_points(np.stack([(x0 + 8 * cx) * ONE, (y0 + 8 * cy) * ONE], axis=-1))


def coordinates(mesh, w, h, width, height):
    """(X, Y) [h, w]: the rule's sensor-plane coordinates of every crop pixel, in 1/32 pixel."""
    xmax, ymax = min(width - 1, LAST_MAX), min(height - 1, LAST_MAX)
    n = as_xy(mesh)
    n[..., 0] = np.clip(n[..., 0], 0, xmax * ONE)
    n[..., 1] = np.clip(n[..., 1], 0, ymax * ONE)
    y, x = np.mgrid[0:h, 0:w]
    cx, cy, i, j = x >> 3, y >> 3, (x & 7)[..., None], (y & 7)[..., None]
    A, B, C, D = n[cy, cx], n[cy, cx + 1], n[cy + 1, cx], n[cy + 1, cx + 1]
    N = (8 - i) * (8 - j) * A + i * (8 - j) * B + (8 - i) * j * C + i * j * D
    P = (N + 32) >> 6
    return P[..., 0], P[..., 1]


def warp(buffer, rec, fmt, mesh, w, h, base=0):
    """The warped crop [h, w] of the plane `rec` describes in the flat buffer, read in format fmt.  A mesh whose first
    node has x == NONE: the plain crop of the record."""
    buffer = np.asarray(buffer, np.uint8).reshape(-1)
    mesh = np.asarray(mesh, POINT_DTYPE)
    if int(mesh.reshape(-1)[0]["x"]) == NONE:
        return csr.crop(buffer, rec, fmt, 1, w, h, base)
    width, height, pitch = int(rec["width"]), int(rec["height"]), int(rec["pitch"])
    xmax, ymax = min(width - 1, LAST_MAX), min(height - 1, LAST_MAX)
    X, Y = coordinates(mesh, w, h, width, height)
    xi, fx, yi, fy = X >> FRAC, X & (ONE - 1), Y >> FRAC, Y & (ONE - 1)
    x1, y1 = np.minimum(xi + 1, xmax), np.minimum(yi + 1, ymax)
    origin = base + int(rec["offset"])
    p = lambda yy, xx: csr.grey(buffer, origin + yy * pitch, fmt, xx).astype(np.int64)
    v = (p(yi, xi) * (ONE - fx) * (ONE - fy) + p(yi, x1) * fx * (ONE - fy) + p(y1, xi) * (ONE - fx) * fy + p(y1, x1) * fx * fy + 512) >> 10
    assert (v >= 0).all() and (v <= 255).all()
    return v.astype(np.uint8)


def histogram(crop):
    """The masked 10-bin exposure histogram of a crop (mainloop.cpp:203-214): bin v * 10 // 255, 255 counted nowhere."""
    h, w = crop.shape
    mx0, my0 = max(w // 2 - MASK // 2, 0), max(h // 2 - MASK // 2, 0)
    mx1, my1 = min(w // 2 - MASK // 2 + MASK, w), min(h // 2 - MASK // 2 + MASK, h)
    b = crop[my0:my1, mx0:mx1].astype(np.int64) * 10 // 255
    return np.bincount(b.reshape(-1), minlength=11)[:10].astype(np.uint32)


def node_unit(v):
    """floor(v * 32 + 0.5) saturated to int32; a NaN: 0."""
    r = v * 32.0 + 0.5
    if r != r:
        return 0
    if r <= I32_MIN:
        return I32_MIN
    if r >= I32_MAX:
        return I32_MAX
    return int(math.floor(r))


def lens(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, out_fx=None, out_fy=None, out_cx=None, out_cy=None, w=None, h=None):
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, k1=k1, k2=k2, p1=p1, p2=p2, k3=k3, out_fx=fx if out_fx is None else out_fx,
                out_fy=fy if out_fy is None else out_fy, out_cx=w / 2.0 if out_cx is None else out_cx,
                out_cy=h / 2.0 if out_cy is None else out_cy)


def from_lens(w, h, l):
    """The header's lens helper, operation by operation in doubles."""
    nx, ny = mesh_size(w, h)
    out = np.zeros((ny, nx), POINT_DTYPE)
    for cy in range(ny):
        for cx in range(nx):
            u, v = float(8 * cx), float(8 * cy)
            xn, yn = (u - l["out_cx"]) / l["out_fx"], (v - l["out_cy"]) / l["out_fy"]
            r2 = xn * xn + yn * yn
            rad = 1.0 + r2 * (l["k1"] + r2 * (l["k2"] + r2 * l["k3"]))
            xd = xn * rad + 2.0 * l["p1"] * xn * yn + l["p2"] * (r2 + 2.0 * xn * xn)
            yd = yn * rad + l["p1"] * (r2 + 2.0 * yn * yn) + 2.0 * l["p2"] * xn * yn
            out[cy, cx] = (node_unit(l["fx"] * xd + l["cx"]), node_unit(l["fy"] * yd + l["cy"]))
    if int(out[0, 0]["x"]) == NONE:
        out[0, 0]["x"] = NONE + 1
    return out


def barrel(w, h, width, height, k1=-0.28, k2=0.07):
    """The lens of a short downward camera: the sensor's principal point a little off its centre, the virtual camera at
    the crop's centre with the same focal length."""
    f = 0.9 * max(w, h)
    return lens(f, f * 1.01, width / 2.0 + 1.3, height / 2.0 - 0.7, k1, k2, 0.002, -0.001, 0.0, w=w, h=h)


def designs(w, h, width, height, x0, y0, seed=3):
    """{name: mesh [ny, nx]} for a w x h crop of a width x height plane whose plain crop starts at (x0, y0): every design
    the tests hold the kernel and the host form to.  Each reaches a path of the rule of its own."""
    nx, ny = mesh_size(w, h)
    cy, cx = np.mgrid[0:ny, 0:nx]
    ident = as_xy(identity(w, h, x0, y0))
    d = {"identity": ident}
    d["half-x"] = ident + [16, 0]
    d["half-y"] = ident + [0, 16]
    d["half-both"] = ident + [16, 16]
    # crop x along sensor y, fractions zero; the plane must hold 8 * (nx - 1) rows and 8 * (ny - 1) columns from its origin
    d["quarter-turn"] = np.stack([(8 * cy) * ONE, (8 * cx) * ONE], axis=-1)
    d["mirror"] = np.stack([(x0 + w - 1 - 8 * cx) * ONE, (y0 + 8 * cy) * ONE], axis=-1)
    d["minify-2x"] = np.stack([(16 * cx) * ONE + 16, (16 * cy) * ONE + 16], axis=-1)   # (runs off a small plane: the border replicates)
    rng = np.random.default_rng(seed)
    d["smooth-random"] = ident + rng.integers(-5 * ONE, 5 * ONE + 1, ident.shape) + (rng.integers(-40, 41, 2) * (cx + cy)[..., None])
    far = ident.copy()
    far[0, :, 1] = -(10 ** 6)
    far[-1, :, 1] = 10 ** 8
    far[:, 0, 0] = I32_MIN + 1
    far[:, -1, 0] = I32_MAX
    d["far-outside"] = far
    d["barrel"] = as_xy(from_lens(w, h, barrel(w, h, width, height)))
    return {k: as_points(v) for k, v in d.items()}
