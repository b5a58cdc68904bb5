"""Designed inputs for the wave-per-block search (csrc/k_search_generic.hip) and their census: what each input is there for,
asserted on the CPU oracle's records before any device is compared (tests/test_generic_edges_ref.py runs the census alone,
tests/test_gpu_generic_edges.py runs it and then the device).

The kernel's edges and the inputs that sit on them:

  candidate trips   (2S+1)^2 candidates over 64 lanes: every radius 1..8 of both tiles.  "corners": clean translations to the
                    four corners of the reach and to its centre (winner index 0, side-1, ncand-side, ncand-1).  "ties":
                    period-2 textures against themselves; the winner must be the first zero of the scan, and from S = 4 on
                    the zeros of the y- and xy-periodic pairs lie in two trips or more (an x-periodic texture that is random
                    along y ties inside one scan row of 2S+1 consecutive indices only, so its zeros share a trip unless a
                    multiple of 64 falls into that row, as at S = 5).
  key width         "contrast": a B-pixel checkerboard against its inverse.  No shift of a pure inverse gives a block whose
                    BEST SAD is B*B*255 (a uniform tile needs a uniform window of B+2S > B pixels), so the window of one
                    block is filled with the inverse of its tile: 65 280 / 16 320 at every candidate, candidate 0 wins.
  rejected, gated   unrelated noise (SAD >= threshold, direction 8), a flat pair (skipped).
  refinement        "half": prev is the direction-k half-pixel image of cur's texture, displaced by S times the direction:
                    the only integer neighbour of the true displacement inside the reach is the corner (or edge) candidate,
                    so match and direction are designed (a block of a smooth texture may still prefer a neighbour ALONG the
                    edge: the census asks for the designed pair among the blocks), and the ring of directions 1 and 5 lies on
                    the last and first row and column of the staged window.  Two more pairs sit at the centre (direction k from the match or the
                    opposite one from its neighbour).  "equalities": four blocks of flat tiles in noise frames, searched with
                    the gradient gate off: one ring byte decides direction 5 at (-S, -S) and direction 1 at (S, S) (the ring's
                    first and last byte are the window's; at the base width the frame's), two directions tie below the match
                    and the lower wins, every direction EQUALS the match's SAD and none wins.
  inside / predictor  two levels: translations of 2S (level 1 hands level 0 a predictor of both signs, edge blocks' windows
                    leave the frame), brightness steps of +-90 that clip (the equalising delta has both signs).  Level 1
                    absorbs a whole-frame translation, so on those pairs level 0 only confirms the predictor; the "residual"
                    pairs move one block by a further (+-S, +-S): under a non-zero predictor level 0's winner is each corner
                    of its scan and |dx|, |dy| reach the two-level reach of 3S.  With half-pixel refinement one more pair
                    lies half a pixel short of (2S, -2S): level 0 chooses directions under a predictor.
  handover          every reason of the 16x16 plan's refusal but "lds" (tests/test_gpu_tile16_plan.py) and "frame" (more than
                    2^31 pixels); the lane-per-block kernels' own refusal needs more than 4 GB between a wave's first and last
                    pair and is out of reach of a test of a few seconds.
  launch shape      1, 2 and 37 pairs; the 32 768-pair split over grid y / z is held by tests/test_gpu_parity.py's
                    large-batch test.

Both direction equalities (a direction sum equal to the match's SAD, two directions tied below it) are designed for EVERY
half-pixel configuration of the sweep, not only for 8x8 +-3 and 16x16 +-5; the filled block of "contrast" adds a second
equality (all eight sums 255*B*B) to each."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import batch_plan_ref as plan_ref
import small_plan_ref as small

DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))     # (hx, hy) of direction k (x right, y down)
SKIPPED = 0xFFFF
LEVELS = dict(A=60, C=100, D=140, B=180)                                          # the flat levels of the equality blocks (far apart: no block matches another's)


# ---- configurations -------------------------------------------------------------------------------------------------------

def config(tile, search, sub, forced=False, w=None, h=None, **kw):
    """One level, dense grid of 3 x 2 blocks on the smallest frame unless w / h say otherwise."""
    M = search + (1 if sub else 0)
    c = dict(tile=tile, search=search, sub=int(sub), forced=forced, w=2 * M + 3 * tile if w is None else w, h=2 * M + 2 * tile if h is None else h,
             px4=False, num_blocks=5, levels=1, eq=0)
    c.update(kw)
    c.setdefault("id", f"{tile}x{tile}-s{search}-sub{int(sub)}" + ("-forced" if forced else ""))
    return c


def sweep_configs():
    out = [config(t, s, sub) for t, radii in ((8, (1, 2, 3, 5, 6, 7, 8)), (16, range(1, 8))) for s in radii for sub in (0, 1)]
    return out + [config(t, s, sub, forced=True) for t, s in ((8, 4), (16, 8)) for sub in (0, 1)]


def two_level_configs():
    out = []
    for t, s in ((8, 1), (8, 3), (8, 8), (16, 2), (16, 7)):
        for eq in (0, 1):
            for sub in (0, 1):
                side = 4 * (s + sub) + 4 * t            # level 1: 2 x 2 blocks
                out.append(config(t, s, sub, w=side, h=side, levels=2, eq=eq, id=f"{t}x{t}-s{s}-eq{eq}-sub{sub}-two-levels"))
    return out


def _width(w0, rem):
    return next(w for w in range(w0, w0 + 16) if w % 16 == rem)


def handover_configs():
    """(config, frame layout, reason): every refusal of the 16x16 plan that a small frame reaches, and the same strides and
    pointer offsets on 8x8 +-3 (reason None: generic whatever the layout)."""
    out = []
    for sub in (0, 1):
        for nb in (1, 5, 8):
            out.append((config(16, 8, sub, w=96, h=80, px4=True, num_blocks=nb, id=f"16x16-px4-{nb}-sub{sub}"), dict(), "grid"))
        base = config(16, 8, sub)
        for rem in (1, 8, 15):
            out.append((config(16, 8, sub, w=_width(base["w"], rem), id=f"16x16-width-{rem}-mod-16-sub{sub}"), dict(), "width"))
        for tile, s, w, h in ((16, 8, 80 if sub else 64, 50 if sub else 48), (8, 3, None, None)):
            c0 = config(tile, s, sub, w=w, h=h)
            assert tile == 8 or (c0["w"] % 16 == 0 and c0["w"] * c0["h"] % 16 == 0)
            name = f"{tile}x{tile}-s{s}-sub{sub}"
            for extra in (4, 1):
                out.append((dict(c0, id=f"{name}-stride-plus-{extra}"), dict(stride_extra=extra), "stride" if tile == 16 else None))
            for off in (1, 4, 8):
                out.append((dict(c0, id=f"{name}-prev-plus-{off}"), dict(prev_off=off), "prev" if tile == 16 else None))
                out.append((dict(c0, id=f"{name}-cur-plus-{off}"), dict(cur_off=off), "cur" if tile == 16 else None))
    return out


def grid_of(c, w=None, level=0):
    return small.grid_for_level(c["w"] if w is None else w, c["h"], level, c["px4"], c["sub"], c["tile"], c["search"], c["num_blocks"])


def params_kw(c, group="std", w=None):
    """std: the gates as published (30; 3 000 or 12 000).  gate-off: the gradient gate at 0 (flat tiles are searched).
    open: gate 0 and SAD threshold 70 000 (the full-contrast family)."""
    kw = dict(width=c["w"] if w is None else w, height=c["h"], tile=c["tile"], search=c["search"], subpixel=c["sub"], min_valid=0,
              value_threshold=70000 if group == "open" else 3000 if c["tile"] == 8 else 12000, feature_threshold=30 if group == "std" else 0)
    if c["levels"] == 2:
        kw.update(pyramid_levels=2, mean_subtract=c["eq"])
    if c["px4"]:
        kw.update(grid_mode=1, num_blocks=c["num_blocks"])
    return kw


def groups_of(c):
    return ("std", "open") + (("gate-off",) if c["sub"] and not c["px4"] and c["levels"] == 1 else ())


def plan_call(c, n_pairs, w=None, stride_extra=0, prev_off=0, cur_off=0):
    """The call as the plan model sees it (tests/batch_plan_ref.py)."""
    w = c["w"] if w is None else w
    return plan_ref.call(c["id"], w, c["h"], n_pairs, tile=c["tile"], search=c["search"], px4=c["px4"], num_blocks=c["num_blocks"], subpixel=c["sub"],
                         levels=c["levels"], mean_subtract=c["eq"], force_generic=c["forced"], stride=w * c["h"] + stride_extra,
                         prev=plan_ref.BASE + prev_off, cur=plan_ref.BASE + (1 << 32) + cur_off)


# ---- frames -----------------------------------------------------------------------------------------------------------------

def _box(a, k):
    s = np.cumsum(np.cumsum(np.pad(a, ((1, 0), (1, 0))), axis=0), axis=1)
    return s[k:, k:] - s[:-k, k:] - s[k:, :-k] + s[:-k, :-k]


def textured(h, w, seed, k=5):
    """Seeded noise under a k x k tent: smooth (a half-pixel average stays near its pixels) and without a period (no
    second match inside +-8), stretched to 20 .. 235."""
    a = np.random.default_rng(seed).integers(0, 256, (h + 2 * (k - 1), w + 2 * (k - 1))).astype(np.int64)
    a = _box(_box(a, k), k)
    return ((a - a.min()) * 215 // (a.max() - a.min()) + 20).astype(np.uint8)


def half_images(c):
    """The eight half-pixel images of the interior of canvas c, by the published averages (floor at every step)."""
    c = c.astype(np.int32)
    p, R, L, D, U = c[1:-1, 1:-1], c[1:-1, 2:], c[1:-1, :-2], c[2:, 1:-1], c[:-2, 1:-1]
    DR, DL, UL, UR = c[2:, 2:], c[2:, :-2], c[:-2, :-2], c[:-2, 2:]
    s0, s1, s2, s3, s4, s5, s6, s7 = (p + R) >> 1, (D + DR) >> 1, (p + D) >> 1, (D + DL) >> 1, (p + L) >> 1, (U + UL) >> 1, (p + U) >> 1, (U + UR) >> 1
    return [x.astype(np.uint8) for x in (s0, (s0 + s1) >> 1, s2, (s3 + s4) >> 1, s4, (s4 + s5) >> 1, s6, (s7 + s0) >> 1)]


def half_pair(canvas, images, h, w, S, k, ox, oy):
    """cur: the canvas; prev: its direction-k half-pixel image displaced by (-ox, -oy): from the match (ox, oy) direction k
    has SAD 0."""
    R = S + 1
    return images[k][R + oy - 1:R + oy - 1 + h, R + ox - 1:R + ox - 1 + w].copy(), canvas[R:R + h, R:R + w].copy()


def _seed(c, w):
    return 7000 + 1000 * c["tile"] + 100 * c["search"] + 10 * c["sub"] + w


def std_pairs(c, w, synth):
    """[(name, prev, cur, meta)] under the published gates."""
    S, B, h = c["search"], c["tile"], c["h"]
    seed = _seed(c, w)
    rng = np.random.default_rng(seed)
    out = []
    for q, shift in enumerate(((-S, -S), (S, -S), (-S, S), (S, S), (0, 0))):
        prev, cur, _ = synth.make_pair(w, h, S, seed + q, shift=shift)
        out.append((f"shift{shift}", prev, cur, dict(kind="shift", shift=shift)))
    out.append(("unrelated", rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8), dict(kind="unrelated")))
    out.append(("flat", np.full((h, w), 90, np.uint8), np.full((h, w), 90, np.uint8), dict(kind="flat")))
    yy, xx = np.mgrid[0:h, 0:w]
    lo, hi = rng.integers(0, 100, (2, max(h, w))), rng.integers(150, 256, (2, max(h, w)))
    per = 2 if S >= 2 else 1                 # (+-1 holds one multiple of 2 only: at S = 1 the tied axis is constant)
    px2 = np.where(xx % per == 0, lo[0][yy], hi[0][yy]).astype(np.uint8)        # period 2 in x, random along y
    py2 = np.where(yy % per == 0, lo[1][xx], hi[1][xx]).astype(np.uint8)        # period 2 in y, random along x
    pxy = np.array([[20, 230], [180, 90]], np.uint8)[yy % 2, xx % 2]
    for name, img in (("period2-x", px2), ("period2-y", py2)) + ((("period2-xy", pxy),) if S >= 2 else ()):
        out.append((name, img, img.copy(), dict(kind="tie", axis=name[8:])))
    if c["sub"]:
        canvas = textured(h + 2 * S + 2, w + 2 * S + 2, seed + 20)
        images = half_images(canvas)
        for k, (hx, hy) in enumerate(DIRS):
            prev, cur = half_pair(canvas, images, h, w, S, k, S * hx, S * hy)
            out.append((f"half{k}-at-the-reach", prev, cur, dict(kind="half-edge", k=k, match=(S * hx, S * hy))))
        for k in (0, 3):
            prev, cur = half_pair(canvas, images, h, w, S, k, 0, 0)
            out.append((f"half{k}-at-the-centre", prev, cur, dict(kind="half-centre", k=k)))
    return out


def open_pairs(c, w, g):
    """Full contrast: a B-pixel checkerboard whose cells are the tiles of block `at`'s row and column, against its inverse;
    in "filled" the search window (and ring) of block `at` holds the inverse of its tile everywhere."""
    B, S, h, m = c["tile"], c["search"], c["h"], 1 if c["sub"] else 0
    x0, y0, sx, sy, nx, ny = g
    at = (min(1, nx - 1), 0)
    i, j = x0 + at[0] * sx, y0 + at[1] * sy
    yy, xx = np.mgrid[0:h, 0:w]
    chk = ((((xx - i) // B + (yy - j) // B) % 2) * 255).astype(np.uint8)
    filled = 255 - chk
    filled[j - S - m:j + B + S + m, i - S - m:i + B + S + m] = 255 - chk[j, i]
    shifted = 255 - np.roll(chk, (3, 5), axis=(0, 1))
    return [("contrast-filled", chk, filled, dict(kind="contrast", block=at[1] * nx + at[0])), ("contrast-shifted", chk, shifted, dict(kind="searched"))]


def equality_pair(c, w, g):
    """Noise frames with four designed blocks (dense 3 x 2 grid, half-pixel): see the module docstring.  Written in the
    order A, C, D, B: where two neighbourhoods share a byte at S = 1 the later block's value is the one both census hold.

    The oracle's eight direction sums at each block's match (orc.subpixel; "far": 25 B or more, a ring row or column at
    V + 50 is averaged in; the census asserts the relations, these are the values at every radius of both tiles):

      block    match      SAD   sum 0  1    2    3    4    5    6    7     direction
      A (0,0)  (-S, -S)   1     far  far  far  far  1    0    1    far   5   ring byte (-1, -1) = V + 4: the window's first byte
      C (1,0)  (0, 0)     2     1    2*   1    far  far  far  far  far   0   0 and 2 tie below the match, the lower index wins
      D (0,1)  (-S, S)    1     1    1    1    1    1    1    1    1     8   every sum equals the match: none is below it
      B (2,1)  (S, S)     1     1    0    1    far  far  far  far  far   1   ring byte (B, B) = V + 4: the window's last byte

    (* 34 at S = 1, where B's far corner byte is C's ring corner.)  A and B: tile flat V but for the corner pixel V + 1 next to
    the ring byte, so the diagonal average there is havg(V, havg(V, V + 4)) = V + 1.  C: tile pixels (r, B-1) and (B-1, q) are
    V + 1; the ring bytes beside them are V + 2 (havg(V, V + 2) = V + 1: direction 0 mends the first, direction 2 the second),
    the rest of the right ring column and bottom ring row V + 1 (havg(V, V + 1) = V: no other pixel moves, and the candidates
    one step right or down cost B - 1 or more).  D: ring V + 1 all round, one tile pixel V + 1."""
    B, S, h = c["tile"], c["search"], c["h"]
    x0, y0, sx, sy, nx, ny = g
    assert (sx, sy) == (B, B) and nx >= 3 and ny >= 2 and c["sub"]
    rng = np.random.default_rng(_seed(c, w) + 40)
    prev, cur = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
    spot = lambda bx, by, dx, dy: (x0 + bx * B, y0 + by * B, x0 + bx * B + dx, y0 + by * B + dy)
    # A: block (0, 0), match (-S, -S), direction 5 by the ring's first byte
    i, j, mx, my = spot(0, 0, -S, -S)
    V = LEVELS["A"]
    prev[j:j + B, i:i + B] = V
    prev[j, i] = V + 1
    cur[my - 1:my + B + 1, mx - 1:mx + B + 1] = V + 50
    cur[my - 1:my + B, mx - 1:mx + B] = V
    cur[my - 1, mx - 1] = V + 4
    # C: block (1, 0), match (0, 0): directions 0 and 2 tie at 1 below the match's 2
    i, j, mx, my = spot(1, 0, 0, 0)
    r, q, V = 2, 3, LEVELS["C"]
    prev[j:j + B, i:i + B] = V
    prev[j + r, i + B - 1] = prev[j + B - 1, i + q] = V + 1
    cur[my - 1:my + B + 1, mx - 1:mx + B + 1] = V + 50
    cur[my:my + B + 1, mx:mx + B + 1] = V
    cur[my:my + B, mx + B] = V + 1
    cur[my + B, mx:mx + B] = V + 1
    cur[my + r, mx + B] = cur[my + B, mx + q] = V + 2
    # D: block (0, 1), match (-S, S): every direction's sum equals the match's SAD of 1
    i, j, mx, my = spot(0, 1, -S, S)
    V = LEVELS["D"]
    prev[j:j + B, i:i + B] = V
    prev[j + B // 2, i + B // 2] = V + 1
    cur[my - 1:my + B + 1, mx - 1:mx + B + 1] = V + 1
    cur[my:my + B, mx:mx + B] = V
    # B: block (2, 1), match (S, S), direction 1 by the ring's last byte
    i, j, mx, my = spot(2, 1, S, S)
    V = LEVELS["B"]
    prev[j:j + B, i:i + B] = V
    prev[j + B - 1, i + B - 1] = V + 1
    cur[my - 1:my + B + 1, mx - 1:mx + B + 1] = V + 50
    cur[my:my + B + 1, mx:mx + B + 1] = V
    cur[my + B, mx + B] = V + 4
    meta = dict(kind="equalities", blocks={0: ((-S, -S), 1, 5), 1: ((0, 0), 2, 0), nx: ((-S, S), 1, 8), 2 * nx - 1: ((S, S), 1, 1)},
                tie=1, equal=nx, last_byte=(my + B, mx + B))
    return [("equalities", prev, cur, meta)]


def two_level_pairs(c, synth):
    S, w, h = c["search"], c["w"], c["h"]
    R, seed = 2 * S + 1, _seed(c, w) + 500
    out = []
    for q, shift in enumerate(((2 * S, -2 * S), (-2 * S, 2 * S), (2 * S, 2 * S), (0, 0))):
        prev, cur, _ = synth.make_pair(w, h, R, seed + q, shift=shift)
        out.append((f"shift{shift}", prev, cur, dict(kind="shift2", shift=shift)))
    if c["eq"]:
        for q, step in enumerate((90, -90)):
            prev, cur, _ = synth.make_pair(w, h, R, seed + 10 + q, shift=(2, -2), brightness=step)
            out.append((f"step{step:+d}", prev, cur, dict(kind="step", step=step)))
    # A whole-frame translation is absorbed by level 1 (reach 2S at level 0): level 0 then only confirms the predictor.  The
    # residual pairs move ONE level-0 block on top of the frame's translation A: its tile is pasted into cur at A + r, r a
    # corner of level 0's scan, and its match at A is inverted -- under the predictor A the winner is the scan's corner and
    # |dx|, |dy| reach the two-level reach of 3S.  (Match and paste are a quarter of a level-1 block each: level 1 still votes A.)
    B, g = c["tile"], grid_of(c)
    origins = block_origins(g)
    for q, (A, r) in enumerate((((2 * S, -2 * S), (S, -S)), ((-2 * S, 2 * S), (-S, S)), ((2 * S, 2 * S), (-S, -S)), ((-2 * S, -2 * S), (S, S)))):
        prev, cur, _ = synth.make_pair(w, h, R, seed + 20 + q, shift=A)
        live = np.flatnonzero(inside(c, g, *A))
        blk = int(live[live.size // 2])
        i, j = origins[blk]
        cur[j + A[1]:j + A[1] + B, i + A[0]:i + A[0] + B] ^= 0xFF        # (at S = B the paste does not touch the match at A: invert it)
        cur[j + A[1] + r[1]:j + A[1] + r[1] + B, i + A[0] + r[0]:i + A[0] + r[0] + B] = prev[j:j + B, i:i + B]
        out.append((f"residual{r}-under{A}", prev, cur, dict(kind="residual", pred=A, res=r, block=blk)))
    if c["sub"]:
        # half a pixel short of (2S, -2S) in both axes: level 1 sees (S - 1/4, -S + 1/4), level 0 refines under its predictor
        canvas = textured(h + 2 * R, w + 2 * R, seed + 30)
        prev, cur = half_pair(canvas, half_images(canvas), h, w, 2 * S, 3, 2 * S, -2 * S)
        out.append(("half3-under-a-predictor", prev, cur, dict(kind="half-predicted")))
    return out


_designs = {}


def design(c, group, w, synth):
    """(names, prevs, curs, metas) of a configuration's group at width w, built once and left unchanged."""
    key = (c["id"], group, w)
    if key not in _designs:
        g = grid_of(c, w)
        if c["levels"] == 2:
            pairs = two_level_pairs(c, synth)
        else:
            pairs = dict(std=lambda: std_pairs(c, w, synth), open=lambda: open_pairs(c, w, g), **{"gate-off": lambda: equality_pair(c, w, g)})[group]()
        prevs, curs = np.stack([q[1] for q in pairs]), np.stack([q[2] for q in pairs])
        prevs.setflags(write=False), curs.setflags(write=False)
        _designs[key] = ([q[0] for q in pairs], prevs, curs, [q[3] for q in pairs])
    return _designs[key]


_oracle = {}


def oracle_of(aof, orc, synth, c, group, w=None):
    """(params, names, prevs, curs, metas, the oracle's records per pair with level 1 and its flow record), computed once."""
    w = c["w"] if w is None else w
    key = (c["id"], group, w)
    if key not in _oracle:
        names, prevs, curs, metas = design(c, group, w, synth)
        p = aof.default_params(**params_kw(c, group, w))
        assert aof.check_params(p) == 0 and tuple(aof.grid(p, 0)) == grid_of(c, w), (c["id"], tuple(aof.grid(p, 0)), grid_of(c, w))
        po = orc.params_from(p)
        refs = []
        for a, b in zip(prevs, curs):
            r = orc.flow_pair(po, a, b, want_l1=True)
            if c["levels"] == 2:
                f1, px, py = orc.reduce(po, r["blocks_l1"], r["subdirs_l1"] if c["sub"] else None, c["search"])
                rec = np.zeros(1, dtype=orc.FLOW_DTYPE)
                rec[0] = f1
                rec["pred_x"], rec["pred_y"] = px, py       # (the level-1 record carries the predictor it emits)
                assert (int(r["flow"]["pred_x"]), int(r["flow"]["pred_y"])) == (px, py)
                r["flow_l1"] = rec[0]
            refs.append(r)
        _oracle[key] = (p, names, prevs, curs, metas, refs)
    return _oracle[key]


# ---- the census -----------------------------------------------------------------------------------------------------------

def sad_table(prev, cur, i, j, B, S):
    """[dy + S, dx + S] SADs of the block at (i, j), in numpy."""
    ref = prev[j:j + B, i:i + B].astype(np.int64)
    win = sliding_window_view(cur[j - S:j + S + B, i - S:i + S + B].astype(np.int64), (B, B))
    return np.abs(win - ref).sum(axis=(2, 3))


def winner_index(b, S):
    return (b["dy"].astype(int) + S) * (2 * S + 1) + b["dx"].astype(int) + S


def block_origins(g):
    x0, y0, sx, sy, nx, ny = g
    return [(x0 + bx * sx, y0 + by * sy) for by in range(ny) for bx in range(nx)]


def census(c, group, w, p, names, prevs, curs, metas, refs, orc):
    """Every pair does what it is in the batch for, on the oracle's records; returns the situations met."""
    S, B, sub = c["search"], c["tile"], c["sub"]
    side, g = 2 * S + 1, grid_of(c, w)
    ncand, met, winners, dirs = side * side, set(), set(), set()
    for name, prev, cur, meta, r in zip(names, prevs, curs, metas, refs):
        b, sd, kind = r["blocks"], r["subdirs"], meta["kind"]
        key = (c["id"], group, w, name)
        live = b["sad"] != SKIPPED
        assert sub or (sd == 8).all(), key
        if sub:
            dirs |= set(sd[live].tolist())
        if kind == "shift":
            assert live.all() and (b["sad"] == 0).all() and (b["dx"] == meta["shift"][0]).all() and (b["dy"] == meta["shift"][1]).all(), (key, b)
            winners |= set(winner_index(b, S).tolist())
        elif kind == "unrelated":
            assert live.all() and (b["sad"] >= p.value_threshold).all() and (sd == 8).all(), (key, b)
            met.add("rejected")
        elif kind == "flat":
            assert not live.any() and (sd == 8).all(), key
            met.add("gated")
        elif kind == "tie":
            trips = set()
            for (i, j), rec in zip(block_origins(g), b):
                zeros = np.flatnonzero(sad_table(prev, cur, i, j, B, S).ravel() == 0)
                assert zeros.size >= 2 and rec["sad"] == 0 and int(winner_index(rec, S)) == int(zeros[0]), (key, i, j, rec, zeros[:4])
                if meta["axis"] == "x":
                    assert set((zeros // side).tolist()) == {S} and rec["dy"] == 0 and rec["dx"] in (-S, 1 - S), (key, rec)
                else:
                    assert rec["dy"] in (-S, 1 - S) and rec["dx"] == (0 if meta["axis"] == "y" else rec["dy"]), (key, rec)
                trips |= set((zeros // 64).tolist())
            assert S < 4 or meta["axis"] == "x" or len(trips) >= 2, (key, trips)
            if len(trips) >= 2:
                met.add("ties-across-trips")
            met.add("ties")
        elif kind == "contrast":
            rec = b[meta["block"]]
            assert rec["sad"] == B * B * 255 != SKIPPED and (rec["dx"], rec["dy"]) == (-S, -S) and live.all(), (key, rec)
            if sub:
                i, j = block_origins(g)[meta["block"]]
                acc = orc.subpixel(prev, i, j, cur, i - S, j - S, B)
                assert (acc == B * B * 255).all() and sd[meta["block"]] == 8, (key, acc)
                met.add("direction-equals-the-match")
            met.add("full-contrast")
        elif kind == "searched":
            assert live.all(), key
        elif kind == "half-edge":
            # (a block may still prefer a neighbour along the edge; the designed match and direction must be among the blocks.
            # These textures make their direction likely, and the set 0 .. 8 asserted below could be met by other blocks: only
            # the blocks of "equalities" carry a direction that is designed byte by byte, the window's edge bytes included.)
            k, (ox, oy) = meta["k"], meta["match"]
            assert live.all() and ((b["dx"] == ox) & (b["dy"] == oy) & (sd == k)).any(), (key, b, sd)
            assert (b["sad"] > 0).all() and (b["sad"] < p.value_threshold).all(), (key, b)
        elif kind == "half-centre":
            # the true displacement is half of DIRS[k]: direction k from (0, 0), or the one that points there from a neighbour
            hx, hy = DIRS[meta["k"]]
            designed = {(ix, iy, DIRS.index((hx - 2 * ix, hy - 2 * iy))) for ix in {0, hx} for iy in {0, hy}}
            assert live.all() and any((int(r_["dx"]), int(r_["dy"]), int(d)) in designed for r_, d in zip(b, sd)), (key, b, sd)
            assert (b["sad"] > 0).all() and (b["sad"] < p.value_threshold).all(), (key, b)
        elif kind == "equalities":
            origins = block_origins(g)
            for blk, ((dx, dy), sad, d) in meta["blocks"].items():
                rec = b[blk]
                assert (int(rec["dx"]), int(rec["dy"]), int(rec["sad"]), int(sd[blk])) == (dx, dy, sad, d), (key, blk, rec, sd[blk])
                i, j = origins[blk]
                acc = orc.subpixel(prev, i, j, cur, i + dx, j + dy, B).astype(int)
                if blk == meta["tie"]:
                    assert acc[0] == acc[2] < sad and (np.delete(acc, (0, 2)) > acc[0]).all(), (key, acc)
                    met.add("two-directions-tie")
                elif blk == meta["equal"]:
                    assert (acc == sad).all(), (key, acc)
                    met.add("direction-equals-the-match")
                else:
                    assert acc[d] == 0 and (np.delete(acc, d) >= sad).all(), (key, acc)
            if (w, c["h"]) == (2 * (S + 1) + 3 * B, 2 * (S + 1) + 2 * B):   # the smallest frame: the ring's first and last byte are the frame's
                assert origins[0][0] - S - 1 == 0 == origins[0][1] - S - 1 and meta["last_byte"] == (c["h"] - 1, w - 1), (key, meta)
                met.add("ring-on-the-frame-edge")
        else:
            raise KeyError(kind)
    if group == "std":
        assert winners >= {0, side - 1, ncand - side, ncand - 1, ncand // 2}, (c["id"], w, sorted(winners))
        assert {"rejected", "gated", "ties"} <= met and (S < 4 or "ties-across-trips" in met), (c["id"], w, met)
        met.add("corners")
        if sub:
            assert dirs >= set(range(9)), (c["id"], w, sorted(dirs))
            met.add("every-direction")
    return met


def wanted_sweep(c, w):
    """The situations the groups of a sweep configuration must meet between them at width w."""
    want = {"corners", "ties", "rejected", "gated", "full-contrast"} | ({"ties-across-trips"} if c["search"] >= 4 else set())
    if c["sub"]:
        want |= {"every-direction", "direction-equals-the-match", "two-directions-tie"} | ({"ring-on-the-frame-edge"} if w == c["w"] else set())
    return want


def wanted_two_levels(c):
    return ({"predictor-range", "out-of-frame", "residual-at-the-scan-corners"} | ({"delta-both-signs"} if c["eq"] else set())
            | ({"direction-under-a-predictor"} if c["sub"] else set()))


def inside(c, g, px, py, w=None):
    """The kernel's window test per level-0 block under predictor (px, py)."""
    w, h, B, S, m = c["w"] if w is None else w, c["h"], c["tile"], c["search"], 1 if c["sub"] else 0
    return np.array([i + px - S - m >= 0 and j + py - S - m >= 0 and i + px + S + m + B <= w and j + py + S + m + B <= h for i, j in block_origins(g)])


def census_two_levels(c, p, names, prevs, curs, metas, refs, orc):
    S, g = c["search"], grid_of(c)
    pl = plan_ref.plan(plan_call(c, len(names)))
    assert pl["valid"] and pl["kind"] == ["generic", "generic"] and pl["coarse"] == "k1" and not pl["small"], (c["id"], pl["kind"], pl["coarse"])
    met, preds, deltas, reach, residuals = set(), [], [], [], set()
    for name, prev, cur, meta, r in zip(names, prevs, curs, metas, refs):
        b, key = r["blocks"], (c["id"], name)
        px, py = int(r["flow"]["pred_x"]), int(r["flow"]["pred_y"])
        live = b["sad"] != SKIPPED
        assert np.array_equal(live, inside(c, g, px, py)), (key, px, py, live)      # (every tile of these textures passes the gate)
        if meta["kind"] == "shift2":
            sx, sy = meta["shift"]
            # (an equalised cur may sit one level off: the crops' means differ)
            assert (px, py) == (sx, sy) and (b["dx"][live] == sx).all() and (b["dy"][live] == sy).all() and (c["eq"] or (b["sad"][live] == 0).all()), (key, px, py, b)
            preds.append((px, py))
            assert live.any(), key
            if (sx, sy) != (0, 0):
                if not live.all():
                    met.add("out-of-frame")
                reach += [int(v) for v in (b["dx"][live].max(), b["dx"][live].min(), b["dy"][live].max(), b["dy"][live].min())]
        elif meta["kind"] == "residual":
            (ax, ay), (rx, ry), rec = meta["pred"], meta["res"], b[meta["block"]]
            assert (px, py) == (ax, ay) != (0, 0) and live[meta["block"]], (key, px, py)
            assert (int(rec["dx"]) - px, int(rec["dy"]) - py) == (rx, ry) and (c["eq"] or rec["sad"] == 0) and rec["sad"] < p.value_threshold, (key, rec)
            assert abs(rx) == abs(ry) == S and max(abs(int(rec["dx"])), abs(int(rec["dy"]))) in (S, 3 * S), key
            residuals.add((rx, ry))
            reach += [int(rec["dx"]), int(rec["dy"])]
            if not live.all():
                met.add("out-of-frame")
        elif meta["kind"] == "half-predicted":
            moved = live & (r["subdirs"] != 8)
            assert (px, py) != (0, 0) and px * py != 0 and moved.any() and (b["sad"][moved] < p.value_threshold).all(), (key, px, py, b, r["subdirs"])
            met.add("direction-under-a-predictor")
        else:
            d0 = orc.frame_mean(prev) - orc.frame_mean(cur)
            d1 = orc.frame_mean(orc.pyramid_down(prev)) - orc.frame_mean(orc.pyramid_down(cur))
            assert d0 * meta["step"] < 0 and d1 * meta["step"] < 0 and (cur == (255 if meta["step"] > 0 else 0)).any() and live.any(), (key, d0, d1)
            deltas.append(d0)
    assert max(reach) > S and min(reach) < -S and {np.sign(v) for q in preds for v in q} == {-1, 0, 1}, (c["id"], reach, preds)
    # the residual pairs: level 0 picks each corner of its scan under a non-zero predictor, out to the two-level reach
    assert residuals == {(S, -S), (-S, S), (-S, -S), (S, S)} and max(reach) == 3 * S and min(reach) == -3 * S, (c["id"], residuals, reach)
    assert "out-of-frame" in met and (not c["sub"] or "direction-under-a-predictor" in met), (c["id"], met)
    met |= {"predictor-range", "residual-at-the-scan-corners"}
    if c["eq"]:
        assert min(deltas) < 0 < max(deltas), deltas
        met.add("delta-both-signs")
    return met


def census_handover(c, layout, reason, n_pairs):
    """The plan model sends the case to the generic kernel, for the named reason."""
    pl = plan_ref.plan(plan_call(c, n_pairs, **layout))
    assert pl["valid"] and pl["kind"][0] == "generic" and not pl["small"] and pl["coarse"] == "none", (c["id"], pl["kind"])
    if reason is not None:
        assert plan_ref.tile16_verdict(pl["a0"]) == reason, (c["id"], plan_ref.tile16_verdict(pl["a0"]), reason)
        assert c["num_blocks"] != 8 or grid_of(c)[2] < 16, "at 8 blocks the tiles overlap"
    return pl
