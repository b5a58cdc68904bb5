"""The motion-field fit (include/aof.h, "the motion FIELD of a batch"; DESIGN.md "The motion field") as a numpy model: exact
int64 sums, the model in float64 with one rounding per operation in the contract's order -- what aof_field_host and
k_field.hip must both give byte for byte --, builders of designed block records, and the geometries the tests walk.
Nothing here imports the product: parameters come as any object or dict with aof_params' field names."""
import numpy as np

import vote_field_ref as vf

BLOCK_DTYPE = vf.BLOCK_DTYPE
FLOW_DTYPE = vf.FLOW_DTYPE
FIELD_DTYPE = np.dtype([("det", "<i8"), ("num_zoom", "<i8"), ("num_rot", "<i8"), ("accepted", "<u4"), ("at_reach", "<u4"),
                        ("fitted", "<u4"), ("used", "<u4"), ("zoom", "<f4"), ("rotation", "<f4"), ("centre_x", "<f4"),
                        ("centre_y", "<f4"), ("flags", "<u4"), ("reserved", "<u4")])
VALID, REFIT = 1, 2
SKIPPED = 0xFFFF
DEFAULTS = dict(min_blocks=8, passes=2, exclude_reach=1, gate_px=1.0)
# sub-direction k -> (hx, hy), Reduce's table; 8 and everything above: none
HALF = np.zeros((256, 2), np.int64)
HALF[:8] = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
SUBDIR_OF = {tuple(h): k for k, h in enumerate(HALF[:9].tolist())}


def fparams(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


# ---- geometry ----------------------------------------------------------------------------------------------------------
def coordinates(p):
    """(X [nb], Y [nb]) int64: half-pixels from the frame centre to every block's centre, record order."""
    g, B = vf.grid_of(p, 0), vf.par(p, "tile")
    X = 2 * (g.x0 + g.step_x * np.arange(g.nx, dtype=np.int64)) + B - vf.par(p, "width")
    Y = 2 * (g.y0 + g.step_y * np.arange(g.ny, dtype=np.int64)) + B - vf.par(p, "height")
    return np.tile(X, g.ny), np.repeat(Y, g.nx)


def range_product(p):
    """nb^2 (Xmax^2 + Ymax^2) as a Python integer: aof_field_supported accepts iff it is below 2^62."""
    X, Y = coordinates(p)
    return int(X.size) ** 2 * (int(np.abs(X).max()) ** 2 + int(np.abs(Y).max()) ** 2)


# ---- the model ---------------------------------------------------------------------------------------------------------
def _solve(sel, X, Y, U, V, min_blocks):
    """(fits, D, Na, Nb, a, b, tU, tV, n) of the blocks `sel`."""
    x, y, u, v = X[sel], Y[sel], U[sel], V[sel]
    n, SX, SY, SU, SV = int(sel.sum()), int(x.sum()), int(y.sum()), int(u.sum()), int(v.sum())
    Q, A, C = int((x * x + y * y).sum()), int((x * u + y * v).sum()), int((x * v - y * u).sum())
    D, Na, Nb = n * Q - SX * SX - SY * SY, n * A - SX * SU - SY * SV, n * C - SX * SV + SY * SU
    assert max(abs(D), abs(Na), abs(Nb), n * Q, abs(n * A), abs(n * C)) < 2 ** 63
    if n < min_blocks or D <= 0:
        return (False, D, Na, Nb, 0.0, 0.0, 0.0, 0.0, n)
    f = np.float64
    a, b = f(Na) / f(D), f(Nb) / f(D)
    tU = ((f(SU) - a * f(SX)) + b * f(SY)) / f(n)
    tV = ((f(SV) - b * f(SX)) - a * f(SY)) / f(n)
    return (True, D, Na, Nb, a, b, tU, tV, n)


def model(p, blocks, subdirs, flow, fp=None):
    """One pair: blocks BLOCK_DTYPE [nb], subdirs uint8 [nb] or None, flow one FLOW_DTYPE record -> one FIELD_DTYPE record."""
    fp = fp or DEFAULTS
    X, Y = coordinates(p)
    S, vthr = vf.par(p, "search"), vf.threshold_of(p)
    dx, dy, sad = blocks["dx"].astype(np.int64), blocks["dy"].astype(np.int64), blocks["sad"].astype(np.int64)
    h = HALF[subdirs] if subdirs is not None else np.zeros((dx.size, 2), np.int64)
    U, V = 2 * dx + h[:, 0], 2 * dy + h[:, 1]
    accepted = (sad != SKIPPED) & (sad < vthr)
    at_reach = accepted & ((np.abs(dx - int(flow["pred_x"])) == S) | (np.abs(dy - int(flow["pred_y"])) == S))
    m1 = accepted & ~at_reach if fp["exclude_reach"] else accepted
    out = np.zeros((), FIELD_DTYPE)
    out["accepted"], out["at_reach"] = accepted.sum(), at_reach.sum()
    s1 = _solve(m1, X, Y, U, V, fp["min_blocks"])
    if not s1[0]:
        return out
    pub, flags = s1, VALID
    if fp["passes"] == 2:
        _, _, _, _, a, b, tU, tV, _ = s1
        g = np.float64(2.0) * np.float64(np.float32(fp["gate_px"]))
        x, y = X.astype(np.float64), Y.astype(np.float64)
        ru = U.astype(np.float64) - ((tU + a * x) - b * y)
        rv = V.astype(np.float64) - ((tV + b * x) + a * y)
        s2 = _solve(m1 & (np.abs(ru) <= g) & (np.abs(rv) <= g), X, Y, U, V, fp["min_blocks"])
        if s2[0]:
            pub, flags = s2, VALID | REFIT
    _, D, Na, Nb, a, b, tU, tV, n = pub
    out["det"], out["num_zoom"], out["num_rot"] = D, Na, Nb
    out["fitted"], out["used"] = s1[8], n
    out["zoom"], out["rotation"] = np.float32(a), np.float32(b)
    out["centre_x"], out["centre_y"] = np.float32(tU * np.float64(0.5)), np.float32(tV * np.float64(0.5))
    out["flags"] = flags
    return out


def model_batch(p, blocks, subdirs, flows, fp=None):
    """blocks [n, nb], subdirs [n, nb] or None, flows [n] -> FIELD_DTYPE [n]."""
    return np.array([model(p, blocks[i], None if subdirs is None else subdirs[i], flows[i], fp) for i in range(len(blocks))], FIELD_DTYPE)


# ---- designed records --------------------------------------------------------------------------------------------------
def records_of(U, V, sad):
    """(blocks, subdirs) that hold the half-pixel field (U, V): dx = floor(U / 2), hx = U mod 2."""
    U, V = np.asarray(U, np.int64), np.asarray(V, np.int64)
    b = np.zeros(U.size, BLOCK_DTYPE)
    b["dx"], b["dy"], b["sad"] = U >> 1, V >> 1, sad
    sd = np.array([SUBDIR_OF[(int(hx), int(hy))] for hx, hy in zip(U & 1, V & 1)], np.uint8)
    return b, sd


def d_similarity(p, rng, a=None, b=None, t=None):
    """The field of a zoom and a rotation about a point, rounded to half-pixels and kept inside the reach."""
    X, Y = coordinates(p)
    S = vf.par(p, "search")
    r = max(int(np.abs(X).max()), int(np.abs(Y).max()), 1)
    a = rng.uniform(-1, 1) * S / r if a is None else a
    b = rng.uniform(-1, 1) * S / r if b is None else b
    t = rng.integers(-S, S + 1, 2) if t is None else t
    U = np.clip(np.rint(t[0] + a * X - b * Y), -2 * S, 2 * S - 1).astype(np.int64)
    V = np.clip(np.rint(t[1] + b * X + a * Y), -2 * S, 2 * S - 1).astype(np.int64)
    return records_of(U, V, rng.integers(0, max(vf.threshold_of(p), 1), X.size))


def d_random(p, rng):
    """Every record on its own: any shift of the reach, any sub-direction, SADs at and around both gates."""
    nb, S, T = coordinates(p)[0].size, vf.par(p, "search"), vf.threshold_of(p)
    b = np.zeros(nb, BLOCK_DTYPE)
    b["dx"], b["dy"] = rng.integers(-S, S + 1, nb), rng.integers(-S, S + 1, nb)
    edges = np.array([0, max(T - 1, 0), T, 0xFFFE, 0xFFFF])
    b["sad"] = np.where(rng.random(nb) < 0.3, edges[rng.integers(0, 5, nb)], rng.integers(0, max(T, 1), nb))
    return b, rng.integers(0, 9, nb).astype(np.uint8)


def d_all_skipped(p, rng):
    b, sd = d_random(p, rng)
    b["sad"] = SKIPPED
    return b, sd


def d_few(p, rng, keep=5):
    """Fewer accepted blocks than min_blocks."""
    b, sd = d_similarity(p, rng)
    skip = np.ones(b.size, bool)
    skip[rng.permutation(b.size)[:keep]] = False
    b["sad"][skip] = SKIPPED
    return b, sd


def d_all_at_reach(p, rng):
    b, sd = d_random(p, rng)
    S = vf.par(p, "search")
    b["dx"], b["sad"] = np.where(rng.random(b.size) < 0.5, S, -S), 0
    return b, sd


def d_outliers(p, rng):
    """A similarity with wild blocks at the lanes where a wave or a quad begins or ends, and in the pair's last record."""
    b, sd = d_similarity(p, rng, t=(0, 0))
    S = vf.par(p, "search")
    at = [k for k in vf.ODD_POSITIONS if k < b.size - 1] + [b.size - 1]
    b["dx"][at], b["dy"][at], b["sad"][at] = S - 1, 1 - S, 0
    sd[at] = 8
    return b, sd


def d_extreme(p, rng):
    """Shifts at the ends of int8, far outside any reach and away from the centre everywhere: the largest sums the integer
    ranges must hold (D and Na beyond 2^53 on the largest grid)."""
    X, Y = coordinates(p)
    nb = X.size
    b = np.zeros(nb, BLOCK_DTYPE)
    b["dx"], b["dy"] = np.where(X > 0, 127, -128), np.where(Y > 0, 127, -128)
    b["sad"] = np.where(rng.random(nb) < 0.1, SKIPPED, 0)        # (a full symmetric grid gives sums with many trailing zero bits)
    return b, rng.integers(0, 9, nb).astype(np.uint8)


DESIGNS = dict(similarity=d_similarity, random=d_random, outliers=d_outliers, skipped=d_all_skipped, few=d_few, reach=d_all_at_reach)
PREDICTORS = ((0, 0), (1, -2), (-3, 0), (0, 4))


def batch(p, n_pairs, seed=0, designs=None):
    """(blocks [n, nb], subdirs [n, nb], flows [n]): pair i holds design i mod len(designs), predictor i mod 4."""
    names = list(designs or DESIGNS)
    every = dict(DESIGNS, extreme=d_extreme)
    nb = coordinates(p)[0].size
    blocks, subdirs, flows = np.zeros((n_pairs, nb), BLOCK_DTYPE), np.zeros((n_pairs, nb), np.uint8), np.zeros(n_pairs, FLOW_DTYPE)
    for i in range(n_pairs):
        rng = np.random.default_rng([nb, seed, i])
        blocks[i], subdirs[i] = every[names[i % len(names)]](p, rng)
        flows[i]["pred_x"], flows[i]["pred_y"] = PREDICTORS[i % len(PREDICTORS)]
        flows[i]["flow_x"], flows[i]["count"] = rng.uniform(-4, 4), i   # (never read by the fit)
    return blocks, subdirs, flows


# ---- the geometries the kernel is held to: (name, constructor, width, height, overrides), and why -----------------------
GEOMETRIES = (
    ("px4-9", "px4", 64, 64, dict(num_blocks=3)),                      # 9: below a wave
    ("dense-49", "dense", 64, 64, {}),
    ("dense-64", "dense", 72, 72, {}),                                 # one wave exactly
    ("dense-72", "dense", 80, 72, {}),
    ("dense-225", "dense", 128, 128, {}),
    ("dense-256", "dense", 136, 136, {}),                              # the wave / workgroup switch
    ("dense-272", "dense", 144, 136, {}),
    ("vga-4661", "dense", 640, 480, {}),                               # odd: misaligned pair bases
    ("c3-18644", "dense", 1280, 960, dict(subpixel=1)),
    ("c5-4661", "dense", 1280, 960, dict(tile=16, search=8, value_threshold=12000)),
)
NBLOCKS = dict(zip((g[0] for g in GEOMETRIES), (9, 49, 64, 72, 225, 256, 272, 4661, 18644, 4661)))
# the largest grid aof_params_check and aof_field_supported both accept: 4096 x 4096 pixels, 261 121 blocks
LARGEST = ("dense-261121", "dense", 4096, 4096, {})
# On a dense grid of 8 x 8 tiles X and Y are multiples of 16 and D of 256: D beyond 2^53 still converts exactly.  A sparse grid
# of step 9 has X and Y of every even value: 206 116 blocks whose D and Na beyond 2^53 have to be ROUNDED to double
LARGEST_ODD = ("px4-206116", "px4", 4096, 4096, dict(num_blocks=500))


def make_params(aof, geom):
    _, kind, w, h, kw = geom
    return aof.px4flow_params(w, h, **kw) if kind == "px4" else aof.default_params(w, h, **kw)
