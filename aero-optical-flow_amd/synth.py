"""Synthetic frame pairs for the flow path (BASELINE.md "Synthetic inputs").

A seeded uniform-random u8 field on a (W+2R)x(H+2R) canvas is 3x3 box-blurred
so that sub-tile structure exists, then cropped twice at an integer offset:
``cur(x, y) == prev(x - dx, y - dy)`` wherever both are defined, so every
textured interior block must report exactly (dx, dy) -- an analytic
known-answer test that does not depend on any implementation.
"""
from __future__ import annotations

import numpy as np

SEED_BASE = 0xA0F


def canvas(width, height, reach, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    raw = rng.integers(0, 256, size=(height + 2 * reach + 2, width + 2 * reach + 2), dtype=np.int32)
    acc = np.zeros((height + 2 * reach, width + 2 * reach), dtype=np.int32)
    for oy in range(3):
        for ox in range(3):
            acc += raw[oy:oy + acc.shape[0], ox:ox + acc.shape[1]]
    return ((acc + 4) // 9).astype(np.uint8)


def make_pair(width, height, reach=4, pair_index=0, shift=None, noise=0, brightness=0, contrast=1.0,
              half=(0, 0)):
    """Returns (prev, cur, (dx, dy)).  ``shift=None`` draws (dx, dy) uniformly from
    [-reach, reach]^2 with the pair's RNG.  ``noise``: +-noise LSB added to cur;
    ``brightness``: constant added to cur (saturating) -- the exposure step the
    reference's auto-exposure loop produces (/root/reference/src/mainloop.cpp:197-275);
    ``half``: (hx, hy) in {-1,0,1}: an extra half-pixel displacement, made by averaging
    the crop with its one-pixel neighbour (needs |shift| < reach on that axis)."""
    seed = SEED_BASE + int(pair_index)
    c = canvas(width, height, reach, seed)
    rng = np.random.Generator(np.random.PCG64(seed ^ 0x5EED))
    if shift is None:
        dx, dy = (int(v) for v in rng.integers(-reach, reach + 1, size=2))
    else:
        dx, dy = int(shift[0]), int(shift[1])
    assert abs(dx) <= reach and abs(dy) <= reach
    prev = c[reach:reach + height, reach:reach + width].copy()
    cur = c[reach - dy:reach - dy + height, reach - dx:reach - dx + width].astype(np.int32)
    if half != (0, 0):
        hx, hy = half
        assert abs(dx + hx) <= reach and abs(dy + hy) <= reach
        nb = c[reach - dy - hy:reach - dy - hy + height, reach - dx - hx:reach - dx - hx + width]
        cur = (cur + nb.astype(np.int32)) >> 1
    if contrast != 1.0:
        cur = np.rint((cur - 128) * contrast + 128).astype(np.int32)
    if noise:
        cur = cur + rng.integers(-noise, noise + 1, size=cur.shape)
    cur = np.clip(cur + brightness, 0, 255).astype(np.uint8)
    return prev, cur, (dx, dy)


def make_batch(width, height, n_pairs, reach=4, first_index=0, **kw):
    prevs = np.empty((n_pairs, height, width), dtype=np.uint8)
    curs = np.empty_like(prevs)
    shifts = np.empty((n_pairs, 2), dtype=np.int32)
    for i in range(n_pairs):
        prevs[i], curs[i], shifts[i] = make_pair(width, height, reach, first_index + i, **kw)
    return prevs, curs, shifts


def make_sequence(width, height, n_frames, reach=4, seed=0, max_step=None):
    """A frame SEQUENCE (camera panning over one canvas): frame k+1 is frame k
    displaced by a per-step shift of at most ``max_step`` (default ``reach``)."""
    if max_step is None:
        max_step = reach
    rng = np.random.Generator(np.random.PCG64(SEED_BASE + 7919 * (seed + 1)))
    steps = rng.integers(-max_step, max_step + 1, size=(n_frames - 1, 2))
    pos = np.zeros((n_frames, 2), dtype=np.int64)
    pos[1:] = np.cumsum(steps, axis=0)
    span = int(np.abs(pos).max()) + 1
    c = canvas(width, height, span, SEED_BASE + 104729 * (seed + 1))
    frames = np.empty((n_frames, height, width), dtype=np.uint8)
    for k in range(n_frames):
        ox, oy = span - int(pos[k, 0]), span - int(pos[k, 1])
        frames[k] = c[oy:oy + height, ox:ox + width]
    return frames, steps.astype(np.int32)


# ---- camera-like input families -------------------------------------------------------------------------------------
#
# The frames the reference's caller delivers are crops of a downward camera under an auto-exposure loop: 1/f-like
# spectra, zoom and rotation on top of the shift, low-texture regions, fractional shifts, vignetting with exposure
# steps.  Each family below has the call shape of make_pair and returns (prev, cur, truth).  Every pixel comes out of
# integer arithmetic only (box sums, Q8 / Q16 fixed point with stated rounding, integer quantiles): the same seed gives
# the same bytes on every machine with the same numpy generator streams.  ``noise`` is make_pair's: +-noise LSB
# uniform on cur, then clamped to u8.

FAMILIES = ("natural", "lowtex", "warp", "subpel", "vignette", "terrace")
_FAMILY_TAG = {"natural": 1, "lowtex": 2, "warp": 3, "subpel": 4, "vignette": 5, "camera": 6, "terrace": 7}

# warp presets: (a00, a01, a10, a11) of the Q16 matrix A that maps a pixel of cur (about the frame centre) to its source
# in the canvas: cur(x) = C(c + A (x - c) - shift).  A > 1 shows less of the scene: the camera zooms out.
WARP_PRESETS = {
    "zoom_in_2": (64251, 0, 0, 64251),             # scale 1 / 1.02
    "zoom_out_1": (66191, 0, 0, 66191),            # scale 1.01
    "rotate_2": (65496, -2287, 2287, 65496),       # +2 degrees
    "rotate_m1": (65526, 1144, -1144, 65526),      # -1 degree
    "zoom_rotate": (65187, -1138, 1138, 65187),    # zoom in 0.5 %, +1 degree
}


def _rng(family, pair_index):
    return np.random.Generator(np.random.PCG64(SEED_BASE + 1000003 * _FAMILY_TAG[family] + int(pair_index)))


def _box_mean(noise, s, height, width):
    """Rounded mean of every s x s box whose top-left corner lies in [0, height) x [0, width) (integral image)."""
    ii = np.zeros((noise.shape[0] + 1, noise.shape[1] + 1), dtype=np.int32)   # (|sum| < 2^31 for these fields)
    ii[1:, 1:] = noise.cumsum(axis=0, dtype=np.int32).cumsum(axis=1, dtype=np.int32)
    tot = ii[s:s + height, s:s + width] - ii[:height, s:s + width] - ii[s:s + height, :width] + ii[:height, :width]
    return (tot + (s * s) // 2) // (s * s)


def _to_u8(acc, lo_frac=(1, 200), hi_frac=(199, 200)):
    """Map an integer field onto 0..255 between two of its integer quantiles (rounded half up, clamped)."""
    flat = np.sort(acc.ravel())
    lo = int(flat[flat.size * lo_frac[0] // lo_frac[1]])
    hi = int(flat[flat.size * hi_frac[0] // hi_frac[1] - 1])
    span = max(hi - lo, 1)
    return np.clip(((acc - lo) * 255 + span // 2) // span, 0, 255).astype(np.uint8)


def natural_field(width, height, rng, alpha2=2, octaves=9):
    """Signed integer field with a 1/f^alpha amplitude spectrum, alpha = alpha2 / 2: octave k is seeded white noise
    box-averaged twice over 2^k x 2^k pixels (a tent, whose side lobes fall fast enough not to flatten the spectrum)
    and weighted isqrt(2^(alpha2 k))."""
    import math
    acc = np.zeros((height, width), dtype=np.int64)
    for k in range(octaves):
        s = 1 << k
        noise = rng.integers(-128, 128, size=(height + 2 * s, width + 2 * s), dtype=np.int64).astype(np.int32)
        once = _box_mean(noise, s, height + s, width + s)
        acc += math.isqrt(1 << (alpha2 * k)) * _box_mean(once, s, height, width)
    return acc


def natural_canvas(width, height, rng, alpha2=2):
    return _to_u8(natural_field(width, height, rng, alpha2))


def _draw_shift(rng, reach, shift):
    if shift is None:
        return tuple(int(v) for v in rng.integers(-reach, reach + 1, size=2))
    return int(shift[0]), int(shift[1])


def _finish(cur, rng, noise):
    cur = np.asarray(cur, dtype=np.int64)
    if noise:
        cur = cur + rng.integers(-noise, noise + 1, size=cur.shape)
    return np.clip(cur, 0, 255).astype(np.uint8)


def _crop_pair(c, width, height, margin, dx, dy):
    prev = c[margin:margin + height, margin:margin + width].copy()
    cur = c[margin - dy:margin - dy + height, margin - dx:margin - dx + width]
    return prev, cur


def _sample_q16(c, sx, sy):
    """Bilinear sample of the u8 canvas at Q16 coordinates (Q8 weights, rounded half up)."""
    ix, iy = sx >> 16, sy >> 16
    fx, fy = (sx >> 8) & 0xFF, (sy >> 8) & 0xFF
    c = c.astype(np.int64)
    top = c[iy, ix] * (256 - fx) + c[iy, ix + 1] * fx
    bot = c[iy + 1, ix] * (256 - fx) + c[iy + 1, ix + 1] * fx
    return (top * (256 - fy) + bot * fy + 32768) >> 16


def make_natural_pair(width, height, reach=4, pair_index=0, noise=0, alpha=1.0, shift=None):
    """A 1/f^alpha texture (alpha 1.0 or 1.5) cropped at an integer shift: truth = (dx, dy) as in make_pair."""
    alpha2 = int(round(2 * alpha))
    assert alpha2 in (2, 3)
    rng = _rng("natural", 2 * pair_index + (alpha2 - 2))
    c = natural_canvas(width + 2 * reach, height + 2 * reach, rng, alpha2)
    dx, dy = _draw_shift(rng, reach, shift)
    prev, cur = _crop_pair(c, width, height, reach, dx, dy)
    return prev, _finish(cur, rng, noise), (dx, dy)


def _lowtex_canvas(width, height, rng):
    """A box texture under a seeded smooth mask (Q8): where the mask is low the frame is near-flat (+-2 LSB of the
    texture at the mask's floor of 4 / 256), where it is high the texture is whole; the mask's ramp is centred on its
    own median, so about half of the area is near-flat."""
    raw = rng.integers(0, 256, size=(height + 2, width + 2), dtype=np.int64)
    tex = _box_mean(raw, 3, height, width) - 128
    m = natural_field(width, height, rng, alpha2=4, octaves=9)
    flat = np.sort(m.ravel())
    med = int(flat[flat.size // 2])
    spread = max(int(flat[flat.size * 9 // 10]) - int(flat[flat.size // 10]), 1)
    mask = np.clip(4 + ((m - med) * 8 * 252 + spread // 2) // spread, 4, 256)
    return (128 + ((tex * mask + 128) >> 8)).astype(np.uint8)


def make_lowtex_pair(width, height, reach=4, pair_index=0, noise=0, shift=None):
    """Texture multiplied by a smooth mask: large near-flat regions beside textured ones.  truth = (dx, dy)."""
    rng = _rng("lowtex", pair_index)
    c = _lowtex_canvas(width + 2 * reach, height + 2 * reach, rng)
    dx, dy = _draw_shift(rng, reach, shift)
    prev, cur = _crop_pair(c, width, height, reach, dx, dy)
    return prev, _finish(cur, rng, noise), (dx, dy)


def _warp_margin(width, height, a, reach):
    cx, cy = width // 2, height // 2
    worst = 0
    for x in (-cx, width - 1 - cx):
        for y in (-cy, height - 1 - cy):
            ex = abs((a[0] - 65536) * x + a[1] * y)
            ey = abs(a[2] * x + (a[3] - 65536) * y)
            worst = max(worst, ex, ey)
    return reach + 2 + (worst >> 16) + 1


def warp_truth(width, height, a, shift):
    """Displacement field (float32 [H, W, 2]: dx, dy) of every pixel p of prev: the point x of cur with
    c + A (x - c) - shift = p lies at p + truth[p]."""
    cx, cy = width // 2, height // 2
    inv = np.linalg.inv(np.array([[a[0], a[1]], [a[2], a[3]]], dtype=np.float64) / 65536.0)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    px, py = xx - cx + shift[0], yy - cy + shift[1]
    tx = inv[0, 0] * px + inv[0, 1] * py + cx - xx
    ty = inv[1, 0] * px + inv[1, 1] * py + cy - yy
    return np.stack([tx, ty], axis=-1).astype(np.float32)


def make_warp_pair(width, height, reach=4, pair_index=0, noise=0, preset=None, shift=None):
    """A 1/f texture; cur is the canvas resampled through a zoom and / or rotation about the frame centre (a Q16 matrix
    from WARP_PRESETS, by pair index unless named) plus the pair's integer shift.  truth: warp_truth's field."""
    rng = _rng("warp", pair_index)
    if preset is None:
        preset = sorted(WARP_PRESETS)[int(pair_index) % len(WARP_PRESETS)]
    a = WARP_PRESETS[preset]
    dx, dy = _draw_shift(rng, reach, shift)
    margin = _warp_margin(width, height, a, reach)
    c = natural_canvas(width + 2 * margin, height + 2 * margin, rng)
    cx, cy = width // 2, height // 2
    yy, xx = np.mgrid[0:height, 0:width].astype(np.int64)
    sx = ((margin + cx - dx) << 16) + a[0] * (xx - cx) + a[1] * (yy - cy)
    sy = ((margin + cy - dy) << 16) + a[2] * (xx - cx) + a[3] * (yy - cy)
    prev = c[margin:margin + height, margin:margin + width].copy()
    return prev, _finish(_sample_q16(c, sx, sy), rng, noise), warp_truth(width, height, a, (dx, dy))


# quarter-pixel phases by pair index: half pixels on both axes (every direction and near-ties between them), on one
# axis, quarter pixels (the integer position wins) and none
SUBPEL_PHASES = ((2, 2), (2, 0), (0, -2), (1, 3), (-2, 2), (3, 2), (0, 0), (2, -1))


def make_subpel_pair(width, height, reach=4, pair_index=0, noise=0, quarter=None):
    """A 1/f texture shifted by (qx / 4, qy / 4) pixels through the bilinear sampler (quarter pixels are exact in
    Q8).  ``quarter=None``: whole pixels drawn from [1 - reach, reach - 1] (so that the half-pixel ring stays inside the
    reach) plus SUBPEL_PHASES[pair_index % 8].  truth = (qx / 4, qy / 4)."""
    rng = _rng("subpel", pair_index)
    if quarter is None:
        ix, iy = (int(v) for v in rng.integers(1 - reach, reach, size=2))
        fx, fy = SUBPEL_PHASES[int(pair_index) % len(SUBPEL_PHASES)]
        qx, qy = 4 * ix + fx, 4 * iy + fy
    else:
        qx, qy = int(quarter[0]), int(quarter[1])
    margin = reach + 2
    c = natural_canvas(width + 2 * margin, height + 2 * margin, rng)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.int64)
    sx = ((xx + margin) << 16) - (qx << 14)
    sy = ((yy + margin) << 16) - (qy << 14)
    prev = c[margin:margin + height, margin:margin + width].copy()
    return prev, _finish(_sample_q16(c, sx, sy), rng, noise), (qx / 4, qy / 4)


# exposure steps of cur by pair index: (Q8 gain, offset in LSB).  Equalisation adds one constant to a whole frame, so a
# pair can clamp at one end only: a longer exposure (gain > 1) clamps the darkest pixels at 0, a shorter one clamps the
# highlights, which stay saturated in both frames, at 255.
VIGNETTE_STEPS = ((384, 0), (192, 0), (352, -4), (224, 6))


def make_vignette_pair(width, height, reach=4, pair_index=0, noise=0, step=None, shift=None):
    """A 1/f scene whose radiance runs past the sensor's range (integer levels 0 ... 1023, a tenth of them at 0 and a
    fifth above 255: shadows and highlights under automatic exposure), at an integer shift.  prev is the scene clamped
    to u8.  cur's gain falls from 256 / 256 at the centre to 154 / 256 (0.6) in the corners, quadratically in the
    radius; then the exposure step (Q8 gain, offset) of VIGNETTE_STEPS, by pair index unless given, is applied (Q16
    product, rounded half up) and the result clamped.  truth = (dx, dy)."""
    rng = _rng("vignette", pair_index)
    gain_q8, offset = VIGNETTE_STEPS[int(pair_index) % len(VIGNETTE_STEPS)] if step is None else step
    acc = natural_field(width + 2 * reach, height + 2 * reach, rng)
    flat = np.sort(acc.ravel())
    lo, hi = int(flat[flat.size // 10]), int(flat[flat.size * 8 // 10])
    span = max(hi - lo, 1)
    scene = np.clip(((acc - lo) * 255 + span // 2) // span, 0, 1023)
    dx, dy = _draw_shift(rng, reach, shift)
    prev, cur = _crop_pair(scene, width, height, reach, dx, dy)
    cx, cy = width // 2, height // 2
    yy, xx = np.mgrid[0:height, 0:width].astype(np.int64)
    r2 = (xx - cx) ** 2 + (yy - cy) ** 2
    rc2 = max(cx * cx + cy * cy, 1)
    gain = 256 - (102 * r2 + rc2 // 2) // rc2
    lit = np.clip(((cur * gain * int(gain_q8) + 32768) >> 16) + int(offset), 0, 255)
    return np.minimum(prev, 255).astype(np.uint8), _finish(lit, rng, noise), (dx, dy)


def make_terrace_pair(width, height, reach=4, pair_index=0, noise=0, levels=6, step=1, stripe=48, half=None):
    """Blocks on the bound: a 1/f field posterised into ``levels`` exactly flat terraces ``step`` LSB apart (128 +- a few
    LSB), and cur cut from it in vertical stripes of ``stripe`` pixels, each at its own integer shift (neighbouring lanes
    of a wave match in different dy rows).  Inside a terrace every candidate ties at SAD 0; across its 1-LSB edges the
    best SADs are small integers, and half-pixel averages (make_pair's ``half``, by pair index unless given: none, one
    axis, both) tie the integer match.  truth: float32 [H, W, 2] displacement of every pixel of cur's stripes."""
    rng = _rng("terrace", pair_index)
    m = natural_field(width + 2 * reach, height + 2 * reach, rng)
    flat = np.sort(m.ravel())
    edges = np.array([int(flat[flat.size * k // levels]) for k in range(1, levels)], dtype=np.int64)
    c = (128 + step * (np.searchsorted(edges, m, side="right") - levels // 2)).astype(np.int64)
    if half is None:
        half = ((0, 0), (1, 0), (1, -1))[int(pair_index) % 3]
    hx, hy = half
    cur = np.empty((height, width), dtype=np.int64)
    truth = np.zeros((height, width, 2), dtype=np.float32)
    for x0 in range(0, width, stripe):
        x1 = min(x0 + stripe, width)
        # (|d| <= reach and |d + h| <= reach on both axes)
        dx = int(rng.integers(-reach + max(-hx, 0), reach - max(hx, 0) + 1))
        dy = int(rng.integers(-reach + max(-hy, 0), reach - max(hy, 0) + 1))
        a = c[reach - dy:reach - dy + height, reach - dx + x0:reach - dx + x1]
        if (hx, hy) != (0, 0):
            a = (a + c[reach - dy - hy:reach - dy - hy + height, reach - dx - hx + x0:reach - dx - hx + x1]) >> 1
        cur[:, x0:x1] = a
        truth[:, x0:x1] = (dx + hx / 2, dy + hy / 2)
    prev = c[reach:reach + height, reach:reach + width].astype(np.uint8)
    return prev, _finish(cur, rng, noise), truth


_MAKERS = {"natural": make_natural_pair, "lowtex": make_lowtex_pair, "warp": make_warp_pair,
           "subpel": make_subpel_pair, "vignette": make_vignette_pair, "terrace": make_terrace_pair}


def make_family_pair(family, width, height, reach=4, pair_index=0, noise=0, **kw):
    return _MAKERS[family](width, height, reach, pair_index, noise, **kw)


def make_family_batch(family, width, height, n_pairs, reach=4, first_index=0, noise=0, **kw):
    """n_pairs pairs of one family (pair indices first_index ...): (prevs, curs, truths as a list)."""
    prevs = np.empty((n_pairs, height, width), dtype=np.uint8)
    curs = np.empty_like(prevs)
    truths = []
    for i in range(n_pairs):
        prevs[i], curs[i], t = make_family_pair(family, width, height, reach, first_index + i, noise, **kw)
        truths.append(t)
    return prevs, curs, truths


def make_camera_sequence(width, height, n_frames, seed=0, max_step=2, zoom_q16=328):
    """A frame SEQUENCE of a camera that pans over a 1/f scene and zooms in steadily: frame k samples the canvas at
    c + A_k (x - c) + pos_k with A_k = (65536 - k zoom_q16) / 65536 (0.5 % per frame by default) and pos_k an integer
    walk of steps of at most ``max_step`` pixels.  Returns (frames, positions [n, 2])."""
    rng = _rng("camera", seed)
    steps = rng.integers(-max_step, max_step + 1, size=(n_frames - 1, 2))
    pos = np.zeros((n_frames, 2), dtype=np.int64)
    pos[1:] = np.cumsum(steps, axis=0)
    cx, cy = width // 2, height // 2
    margin = int(np.abs(pos).max()) + 3 + ((max(cx, cy) * zoom_q16 * n_frames) >> 16)
    c = natural_canvas(width + 2 * margin, height + 2 * margin, rng)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.int64)
    frames = np.empty((n_frames, height, width), dtype=np.uint8)
    for k in range(n_frames):
        s = 65536 - k * zoom_q16
        sx = ((margin + cx + int(pos[k, 0])) << 16) + s * (xx - cx)
        sy = ((margin + cy + int(pos[k, 1])) << 16) + s * (yy - cy)
        frames[k] = _sample_q16(c, sx, sy).astype(np.uint8)
    return frames, pos.astype(np.int32)
