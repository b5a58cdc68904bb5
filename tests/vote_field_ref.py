"""Motion fields by construction (tests/test_vote_field_ref.py, tests/test_gpu_vote_fields.py): frame pairs whose every
tile votes as a DESIGN says, so that a test chooses the histogram the reduce gets -- and with it the branch of
peak_window, the tie, the window's bins, the quad patterns of K3, the key changes of a column walk, the predictor's
halves -- instead of taking what an image happens to give.  Only `prev`'s tiles are written; `cur` stays one texture.

Here: the grid and histogram rules restated from DESIGN.md section 2, the generator (integer-only: box sums, integer
stretches, the spec's half-pixel averages), the named designs as pure functions of (ny, nx, R), reduce_model -- the
Reduce paragraph restated independently of the oracle's code and of the kernels' --, and census, which names the
branches a field reaches.  Pure numpy; a parameter set is any object or dict with the 13 fields of aof_params.  Nothing
here touches the GPU, the product or the oracle."""
import hashlib
from collections import namedtuple

import numpy as np

VOTE, GATED, REJECTED, SAD_BELOW, SAD_AT, GATED_PATCH = range(6)
#  VOTE         the tile is `cur` at its vote: SAD 0
#  GATED        flat tile: skipped by the 4x4 gate, SAD 0xFFFF
#  REJECTED     unrelated noise: searched, SAD >= value_threshold
#  SAD_BELOW    the tile at its (integer) vote plus T - 1 in total: accepted with SAD T - 1
#  SAD_AT       the same plus T: rejected with SAD T
#  GATED_PATCH  only the gate's 4x4 patch is flat: skipped at level 0 while level 1 still sees the texture around it
KIND_NAMES = ("VOTE", "GATED", "REJECTED", "SAD(T-1)", "SAD(T)", "GATED_PATCH")
FLOW_DTYPE = np.dtype([("flow_x", "<f4"), ("flow_y", "<f4"), ("count", "<u4"), ("quality", "u1"), ("flags", "u1"),
                       ("pred_x", "i1"), ("pred_y", "i1")])
FLAG_FLOW_VALID, FLAG_PRED_VALID = 1, 2
SKIPPED = 0xFFFF
REDUCE_CHUNK = 4096          # K3 in two steps beyond 2 * REDUCE_CHUNK records (reduce_chunks, aof_params.cpp)

Grid = namedtuple("Grid", "x0 y0 step_x step_y nx ny")


def par(p, name):
    return int(p[name] if isinstance(p, dict) else getattr(p, name))


# ---- Grid, histogram range, bins ------------------------------------------------------------------
def grid_of(p, level=0):
    w, h, B, S = par(p, "width") >> level, par(p, "height") >> level, par(p, "tile"), par(p, "search")
    if par(p, "grid_mode") == 0:
        M = S + (1 if par(p, "subpixel") else 0)
        return Grid(M, M, B, B, (w - 2 * M) // B, (h - 2 * M) // B)
    lo, hix, hiy = S + 1, w - (S + 1) - B, h - (S + 1) - B
    sx, sy = (hix - lo) // par(p, "num_blocks") + 1, (hiy - lo) // par(p, "num_blocks") + 1
    return Grid(lo, lo, sx, sy, -(-(hix - lo) // sx), -(-(hiy - lo) // sy))


def level_range(p, level=0):
    S = par(p, "search")
    return 3 * S + 1 if par(p, "pyramid_levels") == 2 and level == 0 else S


def bins_of(p, level=0):
    return 2 * (2 * level_range(p, level) + 1) + 1


def threshold_of(p):
    return min(par(p, "value_threshold"), 0xFFFF)


def reduce_chunks(nblocks):
    """Chunks of K3's first step (0: one step), and the records per chunk."""
    if nblocks <= 2 * REDUCE_CHUNK:
        return 0, nblocks
    chunks = -(-nblocks // REDUCE_CHUNK)
    return chunks, -(-nblocks // chunks)


def searchable(p, pred=(0, 0), level=0):
    """[ny, nx] bool: the displaced window (plus the half-pixel ring) of the tile stays inside the frame."""
    g, B, S, m = grid_of(p, level), par(p, "tile"), par(p, "search"), 1 if par(p, "subpixel") else 0
    w, h = par(p, "width") >> level, par(p, "height") >> level
    i = g.x0 + g.step_x * np.arange(g.nx) + pred[0]
    j = g.y0 + g.step_y * np.arange(g.ny) + pred[1]
    okx, oky = (i - S - m >= 0) & (i + S + m + B <= w), (j - S - m >= 0) & (j + S + m + B <= h)
    return oky[:, None] & okx[None, :]


# ---- designs -----------------------------------------------------------------------------------------------------------
class Design:
    """One entry per tile: kind [ny, nx] and vote [ny, nx, 2] = (2 dx + hx, 2 dy + hy), half-pixel units."""

    def __init__(self, kind, vote):
        self.kind = np.ascontiguousarray(kind, np.uint8)
        self.vote = np.ascontiguousarray(vote, np.int32)
        assert self.kind.ndim == 2 and self.vote.shape == self.kind.shape + (2,)

    @classmethod
    def uniform(cls, ny, nx, vote=(0, 0)):
        d = cls(np.zeros((ny, nx), np.uint8), np.zeros((ny, nx, 2), np.int32))
        d.vote[:] = vote
        return d

    @property
    def shape(self):
        return self.kind.shape

    def voters(self):
        return (self.kind == VOTE) | (self.kind == SAD_BELOW)

    def flat(self):
        """(kind [nb], vote [nb, 2]) in record order."""
        return self.kind.reshape(-1), self.vote.reshape(-1, 2)

    def set_flat(self, idx, kind=None, vote=None):
        k, v = self.flat()
        if kind is not None:
            k[idx] = kind
        if vote is not None:
            v[idx] = vote

    def offset(self, vote):
        """The same design around another motion (two levels: residuals around the predictor, 2 P)."""
        return Design(self.kind.copy(), self.vote + np.asarray(vote, np.int32))

    def digest(self):
        return hashlib.sha256(self.kind.tobytes() + self.vote.tobytes()).hexdigest()


def motion(R, k, half=False):
    """The k-th of a fixed sequence of motions in +-R px; consecutive ones differ on both axes."""
    dx, dy = (5 * k + 2) % (2 * R + 1) - R, (3 * k + 1) % (2 * R + 1) - R
    if not half:
        return 2 * dx, 2 * dy
    hx = k % 3 - 1           # a half step on one axis only: a diagonal half-pixel match is the weakest to construct
    return 2 * dx + hx, 2 * dy + (0 if hx else (k // 3) % 3 - 1)


def other(R, base, k, half=False):
    """A motion of the sequence that differs from `base` on both axes."""
    while True:
        m = motion(R, k, half)
        if m[0] != base[0] and m[1] != base[1]:
            return m
        k += 1


def _base(R, variant, half, base):
    return tuple(base) if base is not None else motion(R, variant, half)


def d_one(ny, nx, R, variant=0, half=False, base=None):
    return Design.uniform(ny, nx, _base(R, variant, half, base))


def d_rows(ny, nx, R, variant=0, half=False, base=None, sparse=False):
    """The motion changes at every block row.  sparse: every other row keeps the base (A, B, A, C, A ...)."""
    a = _base(R, variant, half, base)
    d = Design.uniform(ny, nx, a)
    prev = a
    for r in range(ny):
        if sparse and r % 2 == 0:
            prev = a
            continue
        k = r + variant + 1
        m = motion(R, k, half)
        while m[0] == prev[0] or m[1] == prev[1] or m == a:
            k += 1
            m = motion(R, k, half)
        d.vote[r] = prev = m
    return d


def d_row_once(ny, nx, R, variant=0, half=False, base=None):
    a = _base(R, variant, half, base)
    d = Design.uniform(ny, nx, a)
    d.vote[1 + variant % (ny - 1):] = other(R, a, variant + 1, half)
    return d


def d_aba_rows(ny, nx, R, variant=0, half=False, base=None):
    """Rows of A, B, A: thirds of the grid (variant 0), or bands of `variant` rows in turn -- A, B, A inside every walk
    of three steps and more."""
    a = _base(R, variant, half, base)
    d = Design.uniform(ny, nx, a)
    b = other(R, a, variant + 1, half)
    if variant == 0:
        d.vote[max(1, ny // 3):min(ny - 1, max(ny // 3 + 1, 2 * ny // 3))] = b
    else:
        band = 1 + (variant - 1) % 3
        d.vote[(np.arange(ny) // band) % 2 == 1] = b
    return d


def d_cols(ny, nx, R, variant=0, half=False, base=None):
    d = Design.uniform(ny, nx)
    for c in range(nx):
        d.vote[:, c] = motion(R, c + variant, half)
    return d


def d_checker(ny, nx, R, variant=0, half=False, base=None):
    a = _base(R, variant, half, base)
    d = Design.uniform(ny, nx, a)
    rr, cc = np.mgrid[0:ny, 0:nx]
    d.vote[(rr + cc + variant) % 2 == 1] = other(R, a, variant + 1, half)
    return d


ODD_POSITIONS = (0, 1, 31, 32, 63, 64, 65, 127, 255, 256)      # lanes of a wave, and the first of the next waves


def d_odd_one_out(ny, nx, R, variant=0, half=False, base=None):
    """One tile differs: record ODD_POSITIONS[variant] (the last record behind the grid's end)."""
    a = _base(R, variant, half, base)
    d = Design.uniform(ny, nx, a)
    pos = ODD_POSITIONS[variant % len(ODD_POSITIONS)]
    d.set_flat(pos if pos < ny * nx else ny * nx - 1, vote=other(R, a, variant + 1, half))
    return d


def d_silent_rows(ny, nx, R, variant=0, half=False, base=None):
    """All-gated rows between voting rows; the voting rows alternate between two motions."""
    a = _base(R, variant, half, base)
    b = other(R, a, variant + 1, half)
    d = Design.uniform(ny, nx, a)
    period = 2 + variant % 2
    voting = 0
    for r in range(ny):
        if r % period == period - 1 and r != ny - 1:
            d.kind[r] = GATED
        else:
            d.vote[r] = a if voting % 2 == 0 else b
            voting += 1
    return d


# the four slots of a quad, each A (agrees with the quad's motion), B (another motion), R (rejected) or S (skipped)
QUAD_STATES = "ABRS"
QUAD_PATTERNS = tuple(tuple(QUAD_STATES[(q * 37 % 256) >> (2 * j) & 3] for j in range(4)) for q in range(256))


def d_quads(ny, nx, R, variant=0, half=False, base=None):
    """Record order: quad q of the pair takes pattern QUAD_PATTERNS[(q + 27 variant) % 256] -- every pattern of agree,
    disagree, rejected and skipped over the four slots within 256 quads.  B is another motion in even quads and, with
    half-pixel votes, the same integer shift under another direction in odd ones (the `subdirs` word differs inside the
    quad).  The records behind the last whole quad are B, R, A."""
    a = _base(R, variant, half, base)
    d = Design.uniform(ny, nx, a)
    nb = ny * nx
    b_far = other(R, a, variant + 1, half)
    ax, ay = a
    b_near = (ax + 1 if ax % 2 == 0 else ax - (1 if ax > 0 else -1), ay) if half else b_far
    for q in range(nb // 4):
        for j, s in enumerate(QUAD_PATTERNS[(q + 27 * variant) % 256]):
            i = 4 * q + j
            if s == "B":
                d.set_flat(i, vote=b_near if q % 2 else b_far)
            elif s != "A":
                d.set_flat(i, kind=REJECTED if s == "R" else GATED)
    for j, s in enumerate("BRA"[:nb % 4]):
        i = nb - nb % 4 + j
        if s == "B":
            d.set_flat(i, vote=b_far)
        elif s == "R":
            d.set_flat(i, kind=REJECTED)
    return d


def _fill_groups(ny, nx, groups, variant, first=0):
    """groups: [(vote, count)], the first one takes what is left; the small groups are spread over the records (stride
    7, from record `first`), so that quads, waves and rows all see them."""
    nb = ny * nx
    d = Design.uniform(ny, nx, groups[0][0])
    free = list(range(nb))
    at = first % nb
    for vote, count in groups[1:]:
        for _ in range(count):
            at = (at + 7) % len(free)
            d.set_flat(free.pop(at), vote=vote)
    return d


def d_tie(ny, nx, R, variant=0, half=False, base=None):
    """Two bins with equal counts k, four bins apart, and three votes on the bin between them: the first maximum (the
    lower bin) takes {lower, between}, the last would take {between, higher}.  variant & 1: the higher motion comes first
    in record order; variant & 2: the tie is on the y axis.  What is left over is gated."""
    nb, c = ny * nx, 3
    k = (nb - 2 * c) // 2
    axis = (variant >> 1) & 1
    a = list(_base(R, variant, half, base))
    if a[axis] + 4 > 2 * R:
        a[axis] -= 4
    b, m = list(a), list(a)
    b[axis] += 4
    m[axis] += 2
    d = Design.uniform(ny, nx, tuple(a))
    kind, vote = d.flat()
    lo, hi = (tuple(b), tuple(a)) if variant & 1 else (tuple(a), tuple(b))
    vote[:k] = lo
    vote[k:2 * k] = hi
    vote[2 * k:2 * k + c] = tuple(m)
    kind[2 * k + c:] = GATED_PATCH
    # interleave the two halves in record order past the first quarter, so that waves and quads see both
    swap = np.arange(k // 2, k, 2)
    vote[swap], vote[swap + k] = vote[swap + k].copy(), vote[swap].copy()
    return d


def _end_bins(e, n, half):
    """The peak's bin, the other bins of its clipped window, and the first bin outside it."""
    near = e if e < n // 2 else n - 1 - e
    offs = ({0: (1, 2, 3), 1: (-1, 1, 2, 3)}[near] if half else (2, 4))
    sign = 1 if e < n // 2 else -1
    return [e] + [e + sign * o for o in offs]


def d_ends(ny, nx, R, variant=0, half=False, base=None):
    """Peaks at the clipped ends: with half-pixel votes variant 0..3 puts the x peak at bin 0, 1, n-2, n-1 and the y peak
    at bin n-2, n-1, 0, 1 (never both at a half-pixel end: that diagonal match has only one integer neighbour inside the
    search); integer votes reach bins 1 and n-2 only.  Each peak has neighbours on every other bin of its clipped window
    and more votes on the first bin outside it."""
    n = 2 * (2 * R + 1) + 1
    centre = 2 * R + 1
    if half:
        xs, ys = _end_bins((0, 1, n - 2, n - 1)[variant % 4], n, True), _end_bins((n - 2, n - 1, 0, 1)[variant % 4], n, True)
    else:
        xs, ys = _end_bins((1, n - 2)[variant % 2], n, False), _end_bins((n - 2, 1)[variant % 2], n, False)
    m = max(len(xs), len(ys))
    xs, ys = xs + [xs[0]] * (m - len(xs)), ys + [ys[0]] * (m - len(ys))
    counts = (0, 3, 2, 5, 4)
    return _fill_groups(ny, nx, [((x - centre, y - centre), c) for x, y, c in zip(xs, ys, counts)], variant, first=variant)


def d_spread(ny, nx, R, variant=0, half=False, base=None):
    """A window of 3 (integer votes), 4 or 5 non-empty bins around the peak with an odd total, and votes outside it."""
    a = list(_base(R, variant, half, base))
    for ax in (0, 1):
        a[ax] = max(-2 * R + 6, min(2 * R - 6, a[ax]))
    offs = ((-2, 2), (-2, -1, 2), (-2, -1, 1, 2))[variant % 3 if half else 0]
    counts = (3, 5, 2, 1)
    groups = [(tuple(a), 0)] + [((a[0] + o, a[1] - o), c) for o, c in zip(offs, counts)]
    groups += [((a[0] + 6, a[1] - 6), 4), ((a[0] - 4, a[1] + 4), 3)]
    d = _fill_groups(ny, nx, groups, variant, first=3 * variant)
    inside = sum(c for _, c in groups[1:-2])
    main = ny * nx - sum(c for _, c in groups[1:])
    if (inside + main) % 2 == 0:      # an odd total inside the window: one of the peak's tiles goes silent
        kind, vote = d.flat()
        kind[np.flatnonzero((vote == a).all(1))[0]] = GATED_PATCH
    return d


def d_min_valid(ny, nx, R, variant=0, half=False, base=None, min_valid=10):
    """Exactly min_valid (even variants) or min_valid + 1 voters of two motions, spread over the grid; the other tiles
    are gated or rejected in turn."""
    a = _base(R, variant, half, base)
    b = other(R, a, variant + 1, half)
    nb = ny * nx
    want = min_valid + variant % 2
    d = Design.uniform(ny, nx, a)
    kind, vote = d.flat()
    kind[:] = np.where(np.arange(nb) % 2 == 0, GATED_PATCH, REJECTED)
    at = np.linspace(0, nb - 1, want).round().astype(int)
    assert len(set(at.tolist())) == want
    kind[at] = VOTE
    vote[at[1::3]] = b
    return d


def d_threshold(ny, nx, R, variant=0, half=False, base=None):
    """SAD(T - 1) next to SAD(T): records 3k vote A with SAD 0, 3k + 1 vote C with SAD T - 1, 3k + 2 would vote B with
    SAD T.  Integer votes (the half-pixel walk would find something below T - 1)."""
    a = motion(R, variant)
    b, c = other(R, a, variant + 1), other(R, a, variant + 4)
    d = Design.uniform(ny, nx, a)
    kind, vote = d.flat()
    i = np.arange(ny * nx)
    kind[i % 3 == 1], kind[i % 3 == 2] = SAD_BELOW, SAD_AT
    vote[i % 3 == 1], vote[i % 3 == 2] = c, b
    return d


def d_chunks(ny, nx, R, variant=0, half=False, base=None):
    """One motion per chunk of K3's first step, chunk `variant` silent (flat).  Grids that are not chunked are cut the
    same way, as if they were."""
    nb = ny * nx
    chunks = max(2, -(-nb // REDUCE_CHUNK))
    per = -(-nb // chunks)
    d = Design.uniform(ny, nx)
    kind, vote = d.flat()
    for c in range(chunks):
        vote[c * per:(c + 1) * per] = motion(R, c + variant, half)
        if c == variant % chunks:
            kind[c * per:(c + 1) * per] = GATED
    return d


def d_uniform_random(ny, nx, R, variant=0, half=False, base=None):
    rng = np.random.default_rng([ny, nx, R, variant, int(half)])
    top = 2 * R + 1 if half else R
    v = rng.integers(-top, top + 1, (ny, nx, 2))
    return Design(np.zeros((ny, nx), np.uint8), v if half else 2 * v)


DESIGNS = {"one": d_one, "rows": d_rows, "row-once": d_row_once, "aba-rows": d_aba_rows, "cols": d_cols,
           "checker": d_checker, "odd-one-out": d_odd_one_out, "silent-rows": d_silent_rows, "quads": d_quads,
           "tie": d_tie, "ends": d_ends, "spread": d_spread, "min-valid": d_min_valid, "threshold": d_threshold,
           "chunks": d_chunks, "uniform-random": d_uniform_random}


def design(name, ny, nx, R, variant=0, half=False, **kw):
    return DESIGNS[name](ny, nx, R, variant, half, **kw)


def level1_split(ny, nx, a, b, n_b):
    """A level-1 field: the last n_b tiles (record order) vote b, the others a -- integer level-1 shifts (dx, dy)."""
    d = Design.uniform(ny, nx, (2 * a[0], 2 * a[1]))
    if n_b:
        d.set_flat(np.arange(ny * nx - n_b, ny * nx), vote=(2 * b[0], 2 * b[1]))
    return d


def under_predictor(p, residuals, P):
    """Level-0 design of a two-level pair: `residuals` (a design around (0, 0), in +-S) carried to 2 P, tiles the search
    cannot reach under P skipped.  Returns (design, rewritten [ny, nx]: tiles that differ from the plain shift by P)."""
    S = par(p, "search")
    assert np.abs(residuals.vote).max() <= 2 * S + (1 if par(p, "subpixel") else 0)
    d = residuals.offset((2 * P[0], 2 * P[1]))
    out = ~searchable(p, P, 0)
    rewritten = ((residuals.vote != 0).any(2) | (residuals.kind != VOTE)) & ~out
    d.kind[out] = GATED
    return d, rewritten


# ---- the generator -----------------------------------------------------------------------------------------------------
BOX = 3


def texture(h, w, seed, smooth):
    """Uniform noise; smooth: its BOX x BOX box sum stretched to 0..255 (half-pixel votes need neighbours that resemble)."""
    rng = np.random.default_rng([seed, 0])
    if not smooth:
        return rng.integers(0, 256, (h, w)).astype(np.int32)
    noise = rng.integers(0, 256, (h + BOX - 1, w + BOX - 1)).astype(np.int64)
    s = sum(noise[a:a + h, b:b + w] for a in range(BOX) for b in range(BOX))
    return ((s - s.min()) * 255 // (s.max() - s.min())).astype(np.int32)


def towards(t, k):
    """The texture interpolated half a pixel towards direction k (0 = +x, 2 = +y, 4 = -x, 6 = -y, odd = the diagonals
    between; 8 = none): (a + b) >> 1, diagonals ((a + b) >> 1 + (c + d) >> 1) >> 1 of the two pixel pairs beside it."""
    def at(dy, dx):
        return np.roll(t, (-dy, -dx), (0, 1))

    def h(a, b):
        return (a + b) >> 1
    if k == 8:
        return t
    s0, s2, s4, s6 = h(t, at(0, 1)), h(t, at(1, 0)), h(t, at(0, -1)), h(t, at(-1, 0))
    s1, s3 = h(at(1, 0), at(1, 1)), h(at(1, 0), at(1, -1))
    s5, s7 = h(at(-1, 0), at(-1, -1)), h(at(-1, 0), at(-1, 1))
    return (s0, h(s0, s1), s2, h(s3, s4), s4, h(s4, s5), s6, h(s7, s0))[k]


DIRECTION = np.array([[5, 6, 7], [4, 8, 0], [3, 2, 1]])      # [hy + 1, hx + 1]


def split(v):
    """vote -> (integer shift, half step): truncation towards zero, so that |shift| stays within the search."""
    d = np.sign(v) * (np.abs(v) // 2)
    return d, v - 2 * d


def _axis(n_pix, origin, step, n, B):
    c = np.arange(n_pix) - origin
    t = c // step
    inside = (c >= 0) & (t < n) & (c - t * step < B)
    return np.where(inside, t, -1), np.where(inside, c - t * step, 0)


def paint(prev, stack, pad, g, B, d, noise, T, patch_at, only=None):
    """Writes the tiles of grid g (tile size B) into prev as design d says.  stack [9 or 1, H + 2 pad, W + 2 pad]: the
    texture towards each direction; noise [H, W]: what a REJECTED tile holds."""
    H, W = prev.shape
    ty, ry = _axis(H, g.y0, g.step_y, g.ny, B)
    tx, rx = _axis(W, g.x0, g.step_x, g.nx, B)
    inside = (ty[:, None] >= 0) & (tx[None, :] >= 0)
    if only is not None:
        inside &= only[np.maximum(ty, 0)[:, None], np.maximum(tx, 0)[None, :]]
    yy, xx = np.nonzero(inside)
    TY, TX, RY, RX = ty[yy], tx[xx], ry[yy], rx[xx]
    kind = d.kind[TY, TX]
    dx, hx = split(d.vote[TY, TX, 0])
    dy, hy = split(d.vote[TY, TX, 1])
    k = DIRECTION[hy + 1, hx + 1] if stack.shape[0] == 9 else np.zeros_like(dx)
    vals = stack[k, yy + dy + pad, xx + dx + pad]
    for kd, total in ((SAD_BELOW, T - 1), (SAD_AT, T)):
        sel = kind == kd
        amount = total // (B * B) + ((RY * B + RX) < total % (B * B))
        vals = np.where(sel, np.where(vals < 128, vals + amount, vals - amount), vals)
    vals = np.where(kind == GATED, 128, vals)
    in_patch = (RY >= patch_at) & (RY < patch_at + 4) & (RX >= patch_at) & (RX < patch_at + 4)
    vals = np.where((kind == GATED_PATCH) & in_patch, 128, vals)
    vals = np.where(kind == REJECTED, noise[yy, xx], vals)
    assert vals.min() >= 0 and vals.max() <= 255
    prev[yy, xx] = vals


def make_pair(p, seed, d0=None, level1=None, P=None):
    """(prev, cur) uint8 [H, W].  One level: d0, the level-0 design.  Two levels: either level1, a design on the level-1
    grid with integer level-1 votes -- the 2B x 2B level-0 region under each of its tiles is `cur` at twice the shift
    (even shifts commute with the 2 x 2 box) --, or P with d0 = under_predictor(...)[0]: `prev` is `cur` at P, and
    the tiles of d0 that differ from it are rewritten (no more than half of them).  Refuses what cannot come out as
    designed: overlapping tiles, votes out of range, half-pixel votes without `subpixel`, gated tiles without a gate."""
    W, H, B, S = par(p, "width"), par(p, "height"), par(p, "tile"), par(p, "search")
    two, sub = par(p, "pyramid_levels") == 2, bool(par(p, "subpixel"))
    g0 = grid_of(p, 0)
    if g0.step_x < B or g0.step_y < B:
        raise ValueError("the grid's tiles overlap")
    if two != (level1 is not None or P is not None) or (level1 is not None and P is not None):
        raise ValueError("two levels take a level-1 field or a predictor, one level takes neither")
    for d, level in ((d0, 0), (level1, 1)):
        if d is None:
            continue
        g = grid_of(p, level)
        if d.shape != (g.ny, g.nx):
            raise ValueError(f"design {d.shape} on a grid of {(g.ny, g.nx)}")
        R = level_range(p, level)
        v = d.vote[d.kind != GATED]
        if v.size and np.abs(v).max() > 2 * R + (1 if sub and level == 0 else 0):
            raise ValueError("vote out of range")
        if v.size and (v % 2).any() and not (sub and level == 0):
            raise ValueError("half-pixel vote without half-pixel refinement")
        if ((d.kind == GATED) | (d.kind == GATED_PATCH)).any() and par(p, "feature_threshold") <= 0:
            raise ValueError("gated tiles need a gate")
        if ((d.kind == SAD_BELOW) | (d.kind == SAD_AT)).any() and (d.vote[(d.kind == SAD_BELOW) | (d.kind == SAD_AT)] % 2).any():
            raise ValueError("SAD(T) tiles take integer votes")
    pad = level_range(p, 0) + 3
    smooth = any(d is not None and bool((d.vote % 2).any()) for d in (d0, level1))      # (only half-pixel votes need it)
    tex = texture(H + 2 * pad, W + 2 * pad, seed, smooth)
    stack = np.stack([towards(tex, k) for k in range(9)]) if smooth else tex[None]
    cur = tex[pad:pad + H, pad:pad + W].astype(np.uint8)
    noise = 255 * np.random.default_rng([seed, 1]).integers(0, 2, (H, W))      # black and white: far from every texture
    T = threshold_of(p)
    prev = cur.astype(np.int32)
    if level1 is not None:
        g1 = grid_of(p, 1)
        g = Grid(2 * g1.x0, 2 * g1.y0, 2 * g1.step_x, 2 * g1.step_y, g1.nx, g1.ny)
        paint(prev, stack, pad, g, 2 * B, Design(level1.kind, 2 * level1.vote), noise, T, B - 2)
    elif P is not None:
        prev = stack[-1][pad + P[1]:pad + P[1] + H, pad + P[0]:pad + P[0] + W].copy()
        plain = (d0.kind == VOTE) & (d0.vote == (2 * P[0], 2 * P[1])).all(2)
        rewritten = ~plain & (d0.kind != GATED)
        carriers = rewritten & (d0.kind != GATED_PATCH)
        if 2 * int(carriers.sum()) > d0.kind.size:
            raise ValueError("more than half of the tiles carry residuals")
        paint(prev, stack, pad, g0, B, d0, noise, T, B // 2 - 2, only=rewritten)
    else:
        paint(prev, stack, pad, g0, B, d0, noise, T, B // 2 - 2)
    return prev.astype(np.uint8), cur


# ---- records <-> designs -----------------------------------------------------------------------------------------------
SUBDIR_HALF = np.array([(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (0, 0)])


def design_of_records(p, blocks, subdirs, level=0):
    """The field a level's block records hold: skipped -> GATED, SAD >= T -> REJECTED, else the vote."""
    g = grid_of(p, level)
    blocks = np.asarray(blocks).reshape(g.ny, g.nx)
    vote = np.stack([2 * blocks["dx"].astype(np.int32), 2 * blocks["dy"].astype(np.int32)], -1)
    if subdirs is not None and par(p, "subpixel"):
        vote += SUBDIR_HALF[np.minimum(np.asarray(subdirs).reshape(g.ny, g.nx), 8)]
    sad = blocks["sad"].astype(np.int64)
    kind = np.where(sad == SKIPPED, GATED, np.where(sad >= threshold_of(p), REJECTED, VOTE))
    return Design(kind, vote)


def same_field(p, want, got):
    """The conditions of a designed pair on the records' field `got`: every tile meant to vote votes as designed, every
    gated tile is skipped, every rejected tile rejected.  Returns the list of offending records (empty: as designed)."""
    wk, wv = want.flat()
    gk, gv = got.flat()
    w_votes, g_votes = (wk == VOTE) | (wk == SAD_BELOW), gk == VOTE
    bad = (w_votes != g_votes) | (w_votes & (wv != gv).any(1))
    bad |= ((wk == GATED) | (wk == GATED_PATCH)) != (gk == GATED)
    bad |= ((wk == REJECTED) | (wk == SAD_AT)) != (gk == REJECTED)
    return np.flatnonzero(bad).tolist()


# ---- DESIGN.md section 2, Reduce: restated ------------------------------------------------------------------------------
def window_of(pos, n):
    """The published +-2-bin window around the peak, clipped at the ends: (lo, hi, name of the case)."""
    if pos == 0:
        return 0, 2, "bin0"
    if pos == 1:
        return 0, 3, "bin1"
    if pos == n - 2:
        return n - 4, n - 1, "bin n-2"
    if pos == n - 1:
        return n - 3, n - 1, "bin n-1"
    return pos - 2, pos + 2, "inside"


def histograms(d, p, level=0):
    centre = 2 * level_range(p, level) + 1
    n = 2 * centre + 1
    v = d.vote[d.voters()]
    return np.bincount(v[:, 0] + centre, minlength=n), np.bincount(v[:, 1] + centre, minlength=n), len(v)


def reduce_model(d, p, level=0, pred=None):
    """The flow record of a field, from the field alone: integer histograms, float32 operands and ONE float32 division,
    quality = count * 255 // blocks, the predictor by floor division.  pred: None (one level, or level 1, whose record
    carries the predictor it emits), or (px, py, valid) of the level above."""
    centre = 2 * level_range(p, level) + 1
    n = 2 * centre + 1
    hx, hy, count = histograms(d, p, level)
    out = np.zeros((), FLOW_DTYPE)
    out["count"] = count
    px = py = 0
    if count > par(p, "min_valid") and count > 0:
        res = []
        for h, axis in ((hx, 0), (hy, 1)):
            if par(p, "hist_filter"):
                pos = int(np.argmax(h))            # (the first maximum)
                lo, hi, _ = window_of(pos, n)
                v, w = int(sum(k * int(h[k]) for k in range(lo, hi + 1))), int(h[lo:hi + 1].sum())
                flow = (np.float32(v) / np.float32(w) - np.float32(centre)) / np.float32(2)
                pr = (2 * v + w) // (2 * w) - centre
            else:
                s = int(d.vote[d.voters()][:, axis].sum())
                flow = (np.float32(s) * np.float32(0.5)) / np.float32(count)
                pr = (2 * s + count) // (2 * count)
            res.append((flow, pr))
        out["flow_x"], out["flow_y"] = res[0][0], res[1][0]
        px, py = res[0][1], res[1][1]
        out["quality"] = count * 255 // d.kind.size
        out["flags"] = FLAG_FLOW_VALID
    if pred is not None:
        out["pred_x"], out["pred_y"] = pred[0], pred[1]
        if pred[2]:
            out["flags"] |= FLAG_PRED_VALID
    elif level == 1:
        out["pred_x"], out["pred_y"] = px, py
    return out


def pair_model(p, d0, d1=None, P=None):
    """The final record of a pair: level 0 under the predictor that level 1's field (d1) emits, or under a given P."""
    if par(p, "pyramid_levels") == 1:
        return reduce_model(d0, p, 0)
    if d1 is not None:
        r1 = reduce_model(d1, p, 1)
        return reduce_model(d0, p, 0, (int(r1["pred_x"]), int(r1["pred_y"]), bool(r1["flags"] & FLAG_FLOW_VALID)))
    return reduce_model(d0, p, 0, (P[0], P[1], True))


# ---- the census --------------------------------------------------------------------------------------------------------
def quad_class(kinds, votes):
    """The classes one quad of records belongs to (K3's vote_quad)."""
    ok = [k in (VOTE, SAD_BELOW) for k in kinds]
    valid = [tuple(v) for v, o in zip(votes, ok) if o]
    out = set()
    if not valid:
        return {"empty"}
    out.add("agree" if len(set(valid)) == 1 else "messy")
    if not ok[0]:
        out.add("late-first")
    first, last = ok.index(True), 3 - ok[::-1].index(True)
    if not all(ok[first:last + 1]):
        out.add("gap")
    if len(valid) == 4:
        out.add("full")
    return out


def census(d, p, level=0):
    """Which branches of the reduce a field reaches.  d: a design, or design_of_records(...) of the oracle's records."""
    n = bins_of(p, level)
    hx, hy, count = histograms(d, p, level)
    kind, vote = d.flat()
    nb = kind.size
    ok = (kind == VOTE) | (kind == SAD_BELOW)
    out = dict(bins=n, serial=n > 64, voters=count, blocks=nb, tail=nb % 4, valid=count > par(p, "min_valid") and count > 0)
    for h, axis in ((hx, "x"), (hy, "y")):
        pos = int(np.argmax(h))
        lo, hi, name = window_of(pos, n)
        v, w = int(sum(k * int(h[k]) for k in range(lo, hi + 1))), int(h[lo:hi + 1].sum())
        out["peak_" + axis] = pos
        out["window_" + axis] = name
        out["tie_" + axis] = count > 0 and int((h == h[pos]).sum()) > 1
        out["window_bins_" + axis] = int((h[lo:hi + 1] > 0).sum())
        out["window_total_" + axis] = w
        out["outside_" + axis] = count - w                  # votes the window leaves out
        out["dyadic_" + axis] = w > 0 and (w & (w - 1)) == 0 or (w > 0 and v % w == 0)
        out["pred_half_" + axis] = w > 0 and (2 * v + w) % (2 * w) == 0      # the predictor sits at exactly x.5
        out["pred_negative_" + axis] = w > 0 and (2 * v + w) // (2 * w) - (2 * level_range(p, level) + 1) < 0
    # K3's quads, in record order
    classes, differ = set(), False
    for q in range(nb // 4):
        s = slice(4 * q, 4 * q + 4)
        classes |= quad_class(kind[s].tolist(), vote[s].tolist())
        va = vote[s][ok[s]]
        if len(va) > 1 and (va // 2 == va[0] // 2).all() and (va != va[0]).any():
            differ = True
    out["quad_classes"] = classes
    out["quad_directions_differ"] = differ
    out["tail_voters"] = int(ok[nb - nb % 4:].sum()) if nb % 4 else 0
    # the column walk: a wave's step is a block row; its key the (x, y) bins of the row's voters
    rows = []
    for r in range(d.kind.shape[0]):
        v = {tuple(x) for x in d.vote[r][d.voters()[r]].tolist()}
        rows.append(None if not v else (next(iter(v)) if len(v) == 1 else "mixed"))
    voting = [k for k in rows if k is not None]
    keys = [k for k in voting if k != "mixed"]
    runs = [k for i, k in enumerate(keys) if i == 0 or k != keys[i - 1]]
    out["key_changes"] = max(0, len(runs) - 1)
    out["key_returns"] = sum(1 for a, c in zip(runs, runs[2:]) if a == c)      # A, B, A
    out["mixed_rows"] = sum(1 for k in rows if k == "mixed")
    out["voting_rows"] = len(voting)
    first = next((i for i, k in enumerate(rows) if k is not None), len(rows))
    last = len(rows) - next((i for i, k in enumerate(rows[::-1]) if k is not None), len(rows))
    out["silent_rows_between"] = sum(1 for k in rows[first:last] if k is None)
    out["motions"] = len({tuple(x) for x in vote[ok].tolist()})
    # K3's first step
    chunks, per = reduce_chunks(nb)
    out["chunks"] = chunks
    if chunks:
        per_chunk = [{tuple(x) for x in vote[c * per:(c + 1) * per][ok[c * per:(c + 1) * per]].tolist()} for c in range(chunks)]
        out["chunk_motions"] = [len(m) for m in per_chunk]
        out["chunk_sizes"] = [len(kind[c * per:(c + 1) * per]) for c in range(chunks)]
        out["chunks_differ"] = len({frozenset(m) for m in per_chunk if m}) > 1
    return out


# ---- the cases: shapes, pairs and designs of tests/test_gpu_vote_fields.py ---------------------------------------------
# The CPU test holds the oracle to every designed pair of this table; the GPU test holds the device to the oracle and
# to reduce_model on the same pairs.  size: {subpixel: (width, height)} -- the dense grid's margin grows by the
# half-pixel ring, so a block count is kept by another frame size.  Pair k of a case is variant k of its design.
BUT_CHUNKS = tuple(n for n in DESIGNS if n != "chunks")
WIDE = ("quads", "rows", "tie", "spread", "uniform-random")
T16 = dict(tile=16, search=8, value_threshold=12000)

ONE_LEVEL = {
    # <= 256 blocks, nblocks % 4 = 0, 1, 2, 3
    "b108": dict(size={0: (106, 82), 1: (106, 82)}, kw={}, pairs=5, designs=BUT_CHUNKS, blocks=108),
    "b81": dict(size={0: (84, 84), 1: (84, 84)}, kw={}, pairs=5, designs=BUT_CHUNKS, blocks=81),
    "b90": dict(size={0: (92, 84), 1: (92, 84)}, kw={}, pairs=5, designs=BUT_CHUNKS, blocks=90),
    "b99": dict(size={0: (100, 84), 1: (100, 84)}, kw={}, pairs=5, designs=BUT_CHUNKS, blocks=99),
    "b432": dict(size={0: (200, 152), 1: (202, 154)}, kw={}, pairs=3, designs=BUT_CHUNKS, blocks=432),
    "b2048": dict(size={0: (520, 264)}, kw={}, pairs=4, designs=WIDE, blocks=2048),
    "b2016": dict(size={0: (512, 264)}, kw={}, pairs=4, designs=WIDE, blocks=2016),
    "b8320": dict(size={0: (1048, 520), 1: (1050, 522)}, kw={}, pairs=2, designs=("chunks", "tie", "ends", "uniform-random"),
                  blocks=8320),
    "b8192": dict(size={0: (1032, 520), 1: (1034, 522)}, kw={}, pairs=2, designs=("chunks", "tie", "ends", "uniform-random"),
                  blocks=8192),
    "vga": dict(size={0: (640, 480)}, kw={}, pairs=2, blocks=4661,
                designs=("one", "checker", "odd-one-out", "silent-rows", "uniform-random", "min-valid", "rows", "row-once",
                         "aba-rows", "cols")),
    "px4": dict(size={1: (64, 64)}, kw=dict(grid_mode=1, num_blocks=5, subpixel=1), pairs=4, blocks=25,
                designs=("ends", "tie", "spread", "min-valid", "quads")),
    "small99": dict(size={0: (96, 80)}, kw={}, pairs=4, designs=("ends", "tie", "spread", "min-valid", "quads"), blocks=99),
    "t16": dict(size={0: (160, 128), 1: (162, 130)}, kw=T16, pairs=3, designs=("ends", "quads", "uniform-random"), blocks=63),
}


def designs_of(case, sub):
    """threshold only without half-pixel refinement: the walk over the eight directions averages the tile's T - 1 away
    and accepts a half step, which no construction can forbid."""
    return tuple(n for n in ONE_LEVEL[case]["designs"] if not (sub and n == "threshold"))


def one_level_params(make, case, sub):
    """make: default_params of the product or of the oracle."""
    w, h = ONE_LEVEL[case]["size"][sub]
    return make(w, h, **dict(ONE_LEVEL[case]["kw"], subpixel=sub))


def one_level_pairs(p, case, name, seed=0):
    """[(design, prev, cur)] of one case and design: the distinct pairs, variant k with seed + k."""
    g = grid_of(p, 0)
    half = bool(par(p, "subpixel"))
    out = []
    for k in range(ONE_LEVEL[case]["pairs"]):
        kw = dict(min_valid=par(p, "min_valid")) if name == "min-valid" else {}
        d = design(name, g.ny, g.nx, par(p, "search"), k, half and name != "threshold", **kw)
        out.append((d,) + make_pair(p, seed + k, d))
    return out


TWO_LEVEL = {
    # coarse: the fused coarse kernel (or, where the whole pair fits one workgroup, the small path) and the split form
    "c96": dict(size=(96, 80), kw={}, pairs=3),
    "c208": dict(size=(208, 152), kw={}, pairs=3),
    # more than 64 bins at level 0: the one-thread walk over the bins
    "s112": dict(size=(112, 96), kw=dict(search=5), pairs=3, bins=67),
    "s192": dict(size=(192, 160), kw=T16, pairs=3, bins=103),
}
LEVEL1_FIELDS = {            # name: (a, b, share of b): the level-1 votes and the predictor they give
    "pred-2.5": ((-1, 1), (-2, 2), 4),          # three quarters a: (-2.5, +2.5) -> (-2, 3), half up
    "pred-3.5": ((-2, 2), (-1, 1), 4),          # (-3.5, +3.5) -> (-3, 4)
    "pred-3.0": ((-1, 1), (-2, 2), 2),          # halves: (-3, 3); the plain average's 2 s + c is negative and inexact
}
RESIDUALS = ("tie", "spread", "rows", "lowest", "highest", "min-valid")


def two_level_params(make, case, **kw):
    w, h = TWO_LEVEL[case]["size"]
    return make(w, h, **dict(TWO_LEVEL[case]["kw"], pyramid_levels=2, **kw))


def level1_pairs(p, case, field, seed=0):
    """[(level-1 design, prev, cur)]: the field with its b tiles at the end, negated and rolled by a third, and rolled by
    two thirds."""
    g = grid_of(p, 1)
    a, b, share = LEVEL1_FIELDS[field]
    nb = g.ny * g.nx
    out = []
    for k in range(TWO_LEVEL[case]["pairs"]):
        d = level1_split(g.ny, g.nx, a, b, nb // share)
        kind, vote = d.flat()
        vote[:] = np.roll(vote, k * (nb // 3), 0)
        if k == 1:
            vote[:] = -vote                     # the halves on the other side of zero: +x.5 and -x.5 both round up
        out.append((d,) + make_pair(p, seed + k, level1=d))
    return out


P_OF_VARIANT = ((-2, 2), (4, -2), (-6, -4))


def residual_design(p, name, variant):
    """(level-0 design, P) of a two-level pair: residuals around P on the tiles the search reaches under P, no more than
    half of them carrying one.
      tie        a sixth of the tiles at P - 2 px, a sixth at P + 2 px (variant & 2: on the y axis; variant & 1: the
                 higher one first in record order), three at P - 1 px, the others at P but silent at level 0 (their
                 gate patch is flat): level 1 sees a field that is symmetric about P
      min-valid  exactly min_valid (even variants) or min_valid + 1 voters, the others silent at level 0
      lowest, highest   the ends of what the two searches reach together without a half-pixel step at level 1, +-3S:
                 half of the voters at P - S tie with P and, being the lower bin, win; P + S needs two more than P"""
    g, S = grid_of(p, 0), par(p, "search")
    scale = S // 4
    P = tuple(scale * c for c in P_OF_VARIANT[variant % 3])
    if name == "lowest":
        P = (-2 * S, 2 * S)
    elif name == "highest":
        P = (2 * S, -2 * S)
    idx = np.flatnonzero(searchable(p, P, 0).reshape(-1))
    r = Design.uniform(g.ny, g.nx, (0, 0))
    if name == "spread":
        r = design(name, g.ny, g.nx, S, variant, False, base=(0, 0))
    elif name == "rows":
        r = d_rows(g.ny, g.nx, S, variant, False, base=(0, 0), sparse=True)
    elif name == "tie":
        k, axis = len(idx) // 6, (variant >> 1) & 1
        lo, hi, mid = [0, 0], [0, 0], [0, 0]
        lo[axis], hi[axis], mid[axis] = -4, 4, -2
        first, second = (hi, lo) if variant & 1 else (lo, hi)
        r.set_flat(idx, kind=GATED_PATCH)
        r.set_flat(idx[0:4 * k:4], kind=VOTE, vote=first)
        r.set_flat(idx[2:4 * k:4], kind=VOTE, vote=second)
        r.set_flat(idx[1:12:4], kind=VOTE, vote=mid)
    elif name == "min-valid":
        want = par(p, "min_valid") + variant % 2
        at = idx[np.linspace(0, len(idx) - 1, want).round().astype(int)]
        assert len(set(at.tolist())) == want
        r.set_flat(idx, kind=GATED_PATCH)
        r.set_flat(at, kind=VOTE)
        r.set_flat(at[1::3], vote=other(S, (0, 0), variant + 1))
    elif name in ("lowest", "highest"):
        lo = name == "lowest"
        half = len(idx) // 2
        r.set_flat(idx[1:2 * half:2], vote=(-2 * S, 2 * S) if lo else (2 * S, -2 * S))
        if len(idx) % 2:
            r.set_flat(idx[-1], kind=GATED_PATCH)
        if not lo:
            r.set_flat(idx[0:4:2], kind=GATED_PATCH)
    else:
        raise KeyError(name)
    d, _ = under_predictor(p, r, P)
    if name == "spread" and census(d, p)["window_total_x"] % 2 == 0:      # (tiles out of reach took their votes along)
        kind, vote = d.flat()
        kind[np.flatnonzero((kind == VOTE) & (vote == (2 * P[0], 2 * P[1])).all(1))[0]] = GATED_PATCH
    return d, P


def residual_pairs(p, case, name, seed=0):
    out = []
    for k in range(TWO_LEVEL[case]["pairs"]):
        d, P = residual_design(p, name, k)
        out.append((d, P) + make_pair(p, seed + k, d0=d, P=P))
    return out


# ---- what a design is there for ----------------------------------------------------------------------------------------
BLOCK_DTYPE = np.dtype([("dx", "i1"), ("dy", "i1"), ("sad", "<u2")])
HALF_SUBDIR = {tuple(h): k for k, h in enumerate(SUBDIR_HALF.tolist())}


def records_of_design(p, d):
    """(blocks [nb], subdirs [nb] or None): records that hold the design, for the oracle's reduce on its own."""
    kind, vote = d.flat()
    dx, hx = split(vote[:, 0])
    dy, hy = split(vote[:, 1])
    T = threshold_of(p)
    sad = np.select([kind == VOTE, kind == SAD_BELOW, (kind == SAD_AT) | (kind == REJECTED)], [0, T - 1, T], SKIPPED)
    blocks = np.zeros(kind.size, BLOCK_DTYPE)
    blocks["dx"], blocks["dy"], blocks["sad"] = dx, dy, sad
    if not par(p, "subpixel"):
        return blocks, None
    ok = (kind == VOTE) | (kind == SAD_BELOW)
    return blocks, np.array([HALF_SUBDIR[(int(a), int(b))] if o else 8 for a, b, o in zip(hx, hy, ok)], np.uint8)


def check_reaches(name, p, cs, level=0):
    """The conditions on ONE case's fields: cs, the census of every pair of the case (pair k = variant k), taken from
    the ORACLE's records.  Each design must reach what it is there for."""
    g = grid_of(p, level)
    n, half = bins_of(p, level), bool(par(p, "subpixel"))
    what = (name, [(c["window_x"], c["window_y"]) for c in cs])
    every = lambda f: all(f(c) for c in cs)
    some = lambda f: any(f(c) for c in cs)
    if name == "one":
        assert every(lambda c: c["motions"] == 1 and c["key_changes"] == 0), what
    elif name == "rows":
        assert every(lambda c: c["key_changes"] == c["voting_rows"] - 1 >= 2 and c["mixed_rows"] == 0), what
    elif name == "row-once":
        assert every(lambda c: c["key_changes"] == 1 and c["mixed_rows"] == 0), what
    elif name == "aba-rows":
        assert every(lambda c: c["key_changes"] >= 2 and c["key_returns"] >= 1 and c["mixed_rows"] == 0), what
        assert cs[0]["key_changes"] == 2 and (len(cs) < 2 or cs[1]["key_changes"] >= 4), what
    elif name == "cols":
        assert every(lambda c: c["mixed_rows"] == g.ny and c["motions"] >= min(g.nx, 9)), what
    elif name == "checker":
        assert every(lambda c: c["mixed_rows"] == g.ny and c["motions"] == 2), what
    elif name == "odd-one-out":
        assert every(lambda c: c["mixed_rows"] == 1 and c["motions"] == 2), what
    elif name == "silent-rows":
        assert every(lambda c: c["silent_rows_between"] >= 1 and c["key_changes"] >= 1), what
    elif name == "quads":
        seen = set().union(*(c["quad_classes"] for c in cs))
        assert seen >= {"agree", "messy", "late-first", "gap", "empty", "full"}, (what, seen)
        assert every(lambda c: c["tail_voters"] >= min(c["tail"], 1)), what
        assert not half or some(lambda c: c["quad_directions_differ"]), what
    elif name == "tie":
        assert every(lambda c: c["tie_x"] or c["tie_y"]), what
        assert some(lambda c: c["tie_x"]) and (len(cs) < 3 or some(lambda c: c["tie_y"])), what
    elif name == "ends":
        assert every(lambda c: c["window_x"] != "inside" and c["window_y"] != "inside" and c["outside_x"] > 0 and
                     c["outside_y"] > 0 and c["window_bins_x"] >= 2 and c["window_bins_y"] >= 2), what
        seen = {c["window_x"] for c in cs} | {c["window_y"] for c in cs}
        want = {"bin0", "bin1", "bin n-2", "bin n-1"} if half else {"bin1", "bin n-2"}
        assert seen >= want, (what, seen)
    elif name == "spread":
        assert every(lambda c: c["window_bins_x"] >= 3 and c["window_bins_y"] >= 3 and not c["dyadic_x"] and
                     not c["dyadic_y"] and c["window_total_x"] % 2 == 1 and c["outside_x"] > 0), what
        assert not half or len(cs) < 3 or {c["window_bins_x"] for c in cs} >= {3, 4, 5}, what
    elif name == "min-valid":
        mv = par(p, "min_valid")
        assert [c["voters"] for c in cs] == [mv + k % 2 for k in range(len(cs))], what
        assert [c["valid"] for c in cs] == [k % 2 == 1 for k in range(len(cs))], what
    elif name == "chunks":
        assert every(lambda c: c["motions"] >= 1), what
        if cs[0]["chunks"]:
            assert every(lambda c: c["chunks_differ"] and 0 in c["chunk_motions"] and
                         c["chunk_sizes"][-1] < c["chunk_sizes"][0]), (what, cs[0]["chunk_sizes"], cs[0]["chunk_motions"])
    elif name == "uniform-random":
        assert every(lambda c: c["motions"] >= min(20, c["voters"] // 2)), what
    elif name == "lowest":
        assert every(lambda c: c["peak_x"] == 3 and c["tie_x"] and c["tie_y"]), what
    elif name == "highest":
        assert every(lambda c: c["peak_x"] == n - 4 and c["peak_y"] == 3 and c["tie_y"] is False), what
    elif name == "threshold":
        pass        # (the SADs T - 1 and T are conditions on the records themselves: the tests look at them)
    else:
        raise KeyError(name)
