"""The launch plans of a two-level pair's coarse passes in plain Python -- k_coarse's sweep plan and K1's strip plan
(csrc/aof_coarse_plan.hpp: coarse_plan_make, pyramid_plan_make) --, what the kernels make of them lane by lane (k_coarse's
phase 1, k_pyramid_vec, k_pyramid_scalar), which kernel a batch's coarse pass is made by (batch_plan_ref.py, the model of aof_batch_plan.hpp: plan_batch), the
names of the paths a launch can take through all of it, and the case lists of tests/test_coarse_plan_ref.py,
tests/test_host_asan.py (the same plans from the C++ functions) and tests/test_gpu_coarse_plan.py (every case of
GPU_CASES on the device, against the oracle).

Written from DESIGN.md ("Kernels": K1, K1C) and the kernels' comments:

  k_coarse   one workgroup of 512 lanes per pair.  A lane owns one 16-byte chunk of a level-0 row pair: lane t sits at
             row t / chunks of the sweep and chunk t % chunks; a sweep covers `rpi` level-1 rows, lanes beyond rpi rows
             idle.  A frame takes nkf = ceil(h1 / rpi) sweeps, a pair nk = 2 nkf (prev first), loaded in rounds of two
             batches of four: nk_pad sweeps.  Rows beyond a frame's end re-read its last row pair and are dropped.  The
             loads run one round ahead, so the last round of a pair already requests the first eight sweeps of the
             workgroup's next pair (pair + workgroups), or of the same pair again behind the last one.
  K1 vec     frames cut into strips of 1024 / chunks level-1 rows (at least one), a workgroup of 256 lanes per strip,
             item i of a strip = row i / chunks, chunk i % chunks.
  K1 scalar  one 2x2 cell per lane and trip, cells of the odd last column / row summed but not written; a frame's
             ceil(cells / 1024) workgroups stride over its cells together.
"""
import numpy as np

import selftest_rig as rig
from cols_plan_ref import fast_div, fastdiv_make

# csrc/aof_coarse_plan.hpp
THREADS, UNROLL, MAX_BINS, SCRATCH, LDS_LIMIT = 512, 4, 64, 8, 160 * 1024
STAGGER_GROUPS, STAGGER_BYTES_PER_US = 3, 75000
K1_THREADS, K1_ITEMS = 256, 1024
# the verdict of coarse_fused_supported: the first condition that fails (enum CoarseVerdict, in this order)
VERDICTS = ("ok", "tile", "search", "subpixel", "width", "height", "stride", "chunks", "prev", "cur", "grid", "bins", "pairs", "lds")
CENSUS_CUS = 256   # the CU-relative pair counts of the case lists are evaluated here on the host
BASE = 0x7F0000000000   # a frame address for the plans: 16-byte aligned


def dense_grid(w, h, level=0, tile=8, search=4, subpixel=0):
    """(x0, y0, step_x, step_y, nx, ny) of the dense grid of a level (aof_params.cpp)."""
    w, h, m = w >> level, h >> level, search + (1 if subpixel else 0)
    return m, m, tile, tile, (w - 2 * m) // tile, (h - 2 * m) // tile


# ---- the two plans -----------------------------------------------------------------------------------------------------

def coarse_lds(w, h, nb):
    """Both level-1 frames, a key per block, two sets of (two histograms and eight words of sums)."""
    return 2 * (w // 2) * (h // 2) + 4 * nb + 2 * (2 * MAX_BINS + SCRATCH) * 4


def coarse_verdict(w, h, pair_stride, prev, cur, grid, rng, tile, search, subpixel, n_pairs):
    x0, y0, sx, sy, nx, ny = grid
    tests = (("tile", tile != 8), ("search", search != 4), ("subpixel", bool(subpixel)), ("width", w < 16 or w % 16 != 0),
             ("height", h < 2 or h % 2 != 0), ("stride", pair_stride % 16 != 0), ("chunks", w // 16 > THREADS),
             ("prev", prev % 16 != 0), ("cur", cur % 16 != 0), ("grid", (x0, y0, sx, sy) != (4, 4, 8, 8) or nx < 1 or ny < 1),
             ("bins", 2 * (2 * rng + 1) + 1 > MAX_BINS), ("pairs", n_pairs > 0x7FFFFFFF))
    for name, fails in tests:
        if fails:
            return name
    return "ok" if coarse_lds(w, h, nx * ny) <= LDS_LIMIT else "lds"


def sweeps(h1, rpi):
    """(nkf, nk, nk_pad) of a frame of h1 level-1 rows swept rpi rows at a time."""
    nkf = -(-h1 // rpi)
    return nkf, 2 * nkf, -(-2 * nkf // (2 * UNROLL)) * (2 * UNROLL)


def coarse_plan(w, h, pair_stride, prev, cur, grid, rng, tile, search, subpixel, n_pairs, cus):
    """coarse_plan_make.  Everything behind the verdict is zero where k_coarse does not serve the configuration."""
    verdict = coarse_verdict(w, h, pair_stride, prev, cur, grid, rng, tile, search, subpixel, n_pairs)
    pl = dict(verdict=verdict, supported=verdict == "ok", w=w, h=h, rows_per_sweep=0, nkf=0, nk=0, nk_pad=0, div_nb=(0, 0), div_nx=(0, 0),
              div_chunks=(0, 0), lds=0, stagger_groups=0, stagger_ticks=0, wgs=0, rmax=0, n_pairs=n_pairs)
    if verdict != "ok":
        return pl
    chunks, h1 = w // 16, h // 2
    rmax = THREADS // chunks
    # as many rows per sweep as the lanes allow, down to half of that: the fewest rows loaded, padding sweeps included;
    # among equals the most rows
    rpi = min(range(max(1, rmax // 2), rmax + 1), key=lambda r: (sweeps(h1, r)[2] * r, -r))
    nkf, nk, nk_pad = sweeps(h1, rpi)
    nb = grid[4] * grid[5]
    pl.update(rows_per_sweep=rpi, nkf=nkf, nk=nk, nk_pad=nk_pad, div_nb=fastdiv_make(nb), div_nx=fastdiv_make(grid[4]),
              div_chunks=fastdiv_make(chunks), lds=coarse_lds(w, h, nb), rmax=rmax, nb=nb,
              stagger_groups=STAGGER_GROUPS if cus > 0 and n_pairs >= 2 * cus else 1,
              stagger_ticks=2 * w * h * 100 // STAGGER_BYTES_PER_US, wgs=0 if cus <= 0 else min(n_pairs, cus))
    return pl


COARSE_FIELDS = ("verdict", "rows_per_sweep", "nkf", "nk", "nk_pad", "nb.mul", "nb.shift", "nx.mul", "nx.shift", "chunks.mul",
                 "chunks.shift", "lds", "stagger_groups", "stagger_ticks", "wgs")


def _coarse_fields(pl):
    """The plan as the flat list of numbers the host self-test prints for coarse_plan_make (COARSE_FIELDS)."""
    return [VERDICTS.index(pl["verdict"]), pl["rows_per_sweep"], pl["nkf"], pl["nk"], pl["nk_pad"], *pl["div_nb"], *pl["div_nx"],
            *pl["div_chunks"], pl["lds"], pl["stagger_groups"], pl["stagger_ticks"], pl["wgs"]]


def pyramid_plan(w, h, pair_stride, prev, cur, sequence, n_pairs, sums=True):
    """pyramid_plan_make.  n_pairs as K1 is given it: the FRAMES of a sequence, else the pairs."""
    scalar_by = dict(width=w < 16 or w % 16 != 0, height=h % 2 != 0, stride=pair_stride % 16 != 0, prev=prev % 16 != 0,
                     cur=not sequence and cur % 16 != 0)
    vec = not any(scalar_by.values())
    units = n_pairs if sequence else 2 * n_pairs
    zero_words = max(0, 4 * (n_pairs - 1 if sequence else n_pairs)) if sums else 0
    if vec:
        rows = max(1, K1_ITEMS // (w // 16))
        nstrips = -(-(h // 2) // rows)
    else:
        rows = 0
        nstrips = max(1, -(-(((w + 1) // 2) * ((h + 1) // 2)) // K1_ITEMS))
    return dict(vec=int(vec), rows_per_strip=rows, nstrips=nstrips, units=units, total=units * nstrips, zero_words=zero_words, w=w, h=h,
                scalar_by=scalar_by, sequence=int(bool(sequence)), n_pairs=n_pairs)


PYRAMID_FIELDS = ("vec", "rows_per_strip", "nstrips", "units", "total", "zero_words")


# ---- k_coarse, phase 1: lanes, sweeps, loads ---------------------------------------------------------------------------

def coarse_lanes(pl):
    """lane -> (yoff, col, active): the row of the sweep and the 16-byte chunk a lane owns; idle lanes sit on (0, 0)."""
    chunks = pl["w"] // 16
    tid = np.arange(THREADS, dtype=np.uint64)
    yoff = fast_div(tid, pl["div_chunks"]).astype(np.int64)
    col = tid.astype(np.int64) - yoff * chunks
    active = yoff < pl["rows_per_sweep"]
    return np.where(active, yoff, 0), np.where(active, col, 0), active


def coarse_sweep(pl, k, lanes=None):
    """Sweep k (0 .. nk_pad - 1) of a pair: the frame it reads (0 prev, 1 cur), per lane the level-1 row, the byte offset
    of the first of its two 16-byte loads (the second is one row, w bytes, behind), and whether the lane keeps it."""
    w, h, rpi, nkf = pl["w"], pl["h"], pl["rows_per_sweep"], pl["nkf"]
    yoff, col, active = coarse_lanes(pl) if lanes is None else lanes
    frame = int(k >= nkf)
    kk = k - nkf * frame
    y1 = yoff + kk * rpi
    wanted = 2 * y1 * w + 16 * col
    assert int(wanted.max()) < 2 ** 32, "the kernel's 32-bit offset"
    off = np.minimum(wanted, (h - 2) * w + 16 * col)       # rows past the frame's end: its last row pair again
    kept = active & (y1 < h // 2) & (k < pl["nk"])
    return dict(frame=frame, y1=y1, col=col, off=off, kept=kept)


def coarse_coverage(pl):
    """Runs every sweep of a pair.  Returns how often each level-1 pixel of (prev, cur) is written to LDS ([2, h1, w1]),
    how often each level-0 byte enters the sums ([2, h, w]) and the lowest / highest byte any load touches; raises where a
    load leaves the frame or a kept load is not the one its level-1 row needs."""
    w, h = pl["w"], pl["h"]
    w1, h1 = w // 2, h // 2
    lds = np.zeros(2 * h1 * w1, dtype=np.int64)
    summed = np.zeros((2, h * w), dtype=np.int64)
    lanes = coarse_lanes(pl)
    lo, hi = w * h, 0
    for k in range(pl["nk_pad"]):
        s = coarse_sweep(pl, k, lanes)
        lo, hi = min(lo, int(s["off"].min())), max(hi, int(s["off"].max()) + w + 16)
        assert 0 <= lo and hi <= w * h, ("a load outside the frame", k, lo, hi)
        kept = s["kept"]
        y1, col, off = s["y1"][kept], s["col"][kept], s["off"][kept]
        assert (off == 2 * y1 * w + 16 * col).all(), ("a kept load was clamped", k)
        row = (s["frame"] * h1 + y1) * w1 + 8 * col           # the (prev, cur) image in LDS: cur behind prev
        for b in range(8):
            np.add.at(lds, row + b, 1)
        for r in (0, w):
            for b in range(16):
                np.add.at(summed[s["frame"]], off + r + b, 1)
    return dict(lds=lds.reshape(2, h1, w1), summed=summed.reshape(2, h, w), lo=lo, hi=hi)


def coarse_walk(pl, n_pairs, block):
    """The pair loop of workgroup `block` with its two register batches as tags: returns (filtered, ahead) -- filtered:
    (pair, k0, tags, set) of every batch handed to the filter, tags = the (pair, sweep) its four loads were issued for,
    set = which of the two histogram sets the pair votes into; ahead: (pair, next, loads) of every batch requested at or
    beyond nk_pad."""
    wgs, nk_pad = pl["wgs"], pl["nk_pad"]
    filtered, ahead = [], []

    def load(pair, nxt, k0):
        if k0 >= nk_pad:
            tags = [(nxt, k0 - nk_pad + u) for u in range(UNROLL)]
            ahead.append((pair, nxt, tags))
            return tags
        return [(pair, k0 + u) for u in range(UNROLL)]

    follower = lambda p: p + wgs if p + wgs < n_pairs else p
    a, b = load(block, follower(block), 0), load(block, follower(block), UNROLL)
    pair, which = block, 0
    while pair < n_pairs:
        nxt = follower(pair)
        for k0 in range(0, nk_pad, 2 * UNROLL):
            filtered.append((pair, k0, a, which))
            a = load(pair, nxt, k0 + 2 * UNROLL)
            filtered.append((pair, k0 + UNROLL, b, which))
            b = load(pair, nxt, k0 + 3 * UNROLL)
        pair, which = pair + wgs, which ^ 1
    return filtered, ahead


# ---- K1: strips, items, cells ----------------------------------------------------------------------------------------------

def k1_vec_items(pl, strip):
    """k_pyramid_vec: the items of a strip in the order (trip, lane) -> (y1, chunk)."""
    chunks, h1, rows = pl["w"] // 16, pl["h"] // 2, pl["rows_per_strip"]
    y_begin = strip * rows
    items = (min(h1, y_begin + rows) - y_begin) * chunks
    lane, trip = np.meshgrid(np.arange(K1_THREADS), np.arange(-(-items // K1_THREADS)))
    it = (trip * K1_THREADS + lane).ravel()
    it = it[it < items]
    return y_begin + it // chunks, it % chunks


def k1_scalar_cells(pl, strip):
    """k_pyramid_scalar: the cells workgroup `strip` of a frame visits, (y, x) of the 2x2 cell."""
    w1c, h1c = (pl["w"] + 1) // 2, (pl["h"] + 1) // 2
    cells, stride = w1c * h1c, pl["nstrips"] * K1_THREADS
    first = strip * K1_THREADS + np.arange(K1_THREADS)
    trips = -(-cells // stride)
    cell = (first[None, :] + stride * np.arange(trips)[:, None]).ravel()
    cell = cell[cell < cells]
    return cell // w1c, cell % w1c


def k1_coverage(pl):
    """One frame through K1: how often each level-1 pixel is written ([h1, w1]) and each level-0 byte summed ([h, w]);
    raises where a read leaves the frame."""
    w, h = pl["w"], pl["h"]
    w1, h1 = w // 2, h // 2
    out, summed = np.zeros(h1 * w1, dtype=np.int64), np.zeros(h * w, dtype=np.int64)
    for strip in range(pl["nstrips"]):
        if pl["vec"]:
            y1, c = k1_vec_items(pl, strip)
            assert y1.size == 0 or (0 <= y1.min() and y1.max() < h1 and c.max() < w // 16)
            for b in range(8):
                np.add.at(out, y1 * w1 + 8 * c + b, 1)
            for r in (0, 1):
                at = (2 * y1 + r) * w + 16 * c
                assert at.size == 0 or at.max() + 16 <= w * h, "a load outside the frame"
                for b in range(16):
                    np.add.at(summed, at + b, 1)
        else:
            y, x = k1_scalar_cells(pl, strip)
            xin, yin = 2 * x + 1 < w, 2 * y + 1 < h
            for dy, dx, ok in ((0, 0, np.ones_like(xin)), (0, 1, xin), (1, 0, yin), (1, 1, xin & yin)):
                at = (2 * y[ok] + dy) * w + 2 * x[ok] + dx
                assert at.size == 0 or (at.max() < w * h and (2 * x[ok] + dx < w).all()), "a read outside the frame"
                np.add.at(summed, at, 1)
            both = xin & yin
            np.add.at(out, y[both] * w1 + x[both], 1)
    return dict(out=out.reshape(h1, w1), summed=summed.reshape(h, w))


def sums_targets(pl, unit):
    """The pixel-sum records a unit's byte sums go to: [(pair, 0 prev | 1 cur)]."""
    if not pl["sequence"]:
        return [(unit >> 1, unit & 1)]
    frames = pl["n_pairs"]
    return ([(unit, 0)] if unit < frames - 1 else []) + ([(unit - 1, 1)] if unit > 0 else [])


# ---- which kernels make a batch's coarse pass (plan_batch) ------------------------------------------------------------------

def n_pairs_of(c, cus=CENSUS_CUS):
    n = c["n_pairs"]
    return n[1] * cus + n[2] if isinstance(n, tuple) else n


def frame_layout(c):
    """(pair_stride, prev, cur) of a case: the byte distance of consecutive pairs and the two frame arrays' addresses
    relative to a 16-byte boundary.  A sequence views one array of frames twice, one frame apart."""
    frame = c["w"] * c["h"]
    if c["sequence"]:
        return frame, BASE + c["prev_off"], BASE + c["prev_off"] + frame
    return frame + c["stride_extra"], BASE + c["prev_off"], BASE + (1 << 32) + c["cur_off"]


def coarse_kind(c, cus=CENSUS_CUS):
    """'small' (k_flow_small does the whole batch), 'fused' (k_coarse), 'k1' (K1, then the level-1 search where there are
    two levels), 'none' (one level without equalisation): batch_plan_ref owns the rule."""
    import batch_plan_ref as bp
    pl = bp.plan(bp.of_coarse(c, cus))
    return "small" if pl["small"] else pl["coarse"]


def case_coarse_plan(c, cus=CENSUS_CUS):
    stride, prev, cur = frame_layout(c)
    return coarse_plan(c["w"], c["h"], stride, prev, cur, dense_grid(c["w"], c["h"], 1, c["tile"], c["search"], c["subpixel"]), c["search"],
                       c["tile"], c["search"], c["subpixel"], n_pairs_of(c, cus), cus)


def case_pyramid_plan(c, cus=CENSUS_CUS):
    stride, prev, cur = frame_layout(c)
    n = n_pairs_of(c, cus)
    return pyramid_plan(c["w"], c["h"], stride, prev, cur, c["sequence"], n + 1 if c["sequence"] else n, bool(c["mean_subtract"]))


def counters(c, cus=CENSUS_CUS):
    """The launches of one call by profiling counter: K_PYRAMID, K_SEARCH_L1, K_REDUCE_L1 (a flat level-1 search: K3 behind
    it, the in-launch reduction is the caller's switch)."""
    import batch_plan_ref as bp
    got = bp.plan(bp.of_coarse(c, cus))["counters"]
    return {k: 1 if got[k] is None else got[k] for k in ("K_PYRAMID", "K_SEARCH_L1", "K_REDUCE_L1")}


# ---- cases and what they reach -----------------------------------------------------------------------------------------------

def case(id, w, h, n_pairs, *paths, levels=2, mean_subtract=1, split=False, subpixel=0, search=4, tile=8, stride_extra=0, prev_off=0,
         cur_off=0, sequence=False, distinct=None, edge=False):
    """w x h frames, n_pairs pairs (a number, or ("cus", a, b) = a CUs + b).  split: the caller asks for the split coarse
    pass (set_split_coarse).  stride_extra: bytes between consecutive pairs beyond a frame; prev_off / cur_off: bytes the
    frame arrays start behind a 16-byte boundary; sequence: one array of n_pairs + 1 frames viewed twice.  distinct:
    distinct pairs the launch replicates (default: all pairs, at most 64).  edge: the last column and row of every frame
    are set so that leaving them out of the sums changes the rounded mean (one level, odd sizes)."""
    return dict(id=id, w=w, h=h, n_pairs=n_pairs, paths=paths, levels=levels, mean_subtract=mean_subtract, split=split, subpixel=subpixel,
                search=search, tile=tile, stride_extra=stride_extra, prev_off=prev_off, cur_off=cur_off, sequence=sequence,
                distinct=distinct, edge=edge)


def params_kw(c):
    # (min_valid 0: a level-1 grid of one or six blocks still yields a predictor, so the level-1 winner shows in level 0)
    kw = dict(pyramid_levels=c["levels"], mean_subtract=c["mean_subtract"], min_valid=0)
    if c["subpixel"]:
        kw["subpixel"] = 1
    if c["search"] != 4:
        kw["search"] = c["search"]
    if c["tile"] != 8:
        kw["tile"] = c["tile"]
    return kw


def distinct_pairs(c, cus=CENSUS_CUS):
    n = n_pairs_of(c, cus)
    return min(n, c["distinct"] or 64)


def device_bytes(c, cus=CENSUS_CUS):
    return 2 * c["w"] * c["h"] * n_pairs_of(c, cus)


def reach_coarse(c, cus=CENSUS_CUS):
    pl = case_coarse_plan(c, cus)
    n, rpi, rmax, chunks, h1 = n_pairs_of(c, cus), pl["rows_per_sweep"], pl["rmax"], c["w"] // 16, c["h"] // 2
    got = {"fused", "rpi_eq_rmax" if rpi == rmax else "rpi_lt_rmax"}
    if rpi == 1:
        got.add("rpi_1")
    idle = int((~coarse_lanes(pl)[2]).sum())
    got.add("idle_lanes_0" if idle == 0 else "idle_lanes_some")
    if chunks in (2, 256, 257, 512):
        got.add(f"chunks_{chunks}")
    if h1 < rpi:
        got.add("h1_lt_rpi")
    got.add("last_sweep_full" if h1 % rpi == 0 else "last_sweep_partial")
    pad = pl["nk_pad"] - pl["nk"]
    got.add(f"pad_{pad}" if pl["nkf"] > 1 else f"pad_{pad}_nkf_1")
    nb = pl["nb"]
    got |= {name for name, hit in (("nb_1", nb == 1), ("nb_under_64", nb < 64), ("nb_512", nb == 512), ("nb_513", nb == 513),
                                   ("nb_over_1024", nb > 1024), ("rounds_2", 512 < nb <= 1024)) if hit}
    got |= {name for name, hit in (("one_generation", n < cus), ("pairs_cus_minus_1", n == cus - 1), ("pairs_cus", n == cus),
                                   ("pairs_cus_plus_1", n == cus + 1), ("pairs_2cus_minus_1", n == 2 * cus - 1),
                                   ("pairs_2cus", n == 2 * cus), ("pairs_2cus_plus_1", n == 2 * cus + 1),
                                   ("three_pairs_per_workgroup", n >= 3 * cus), ("ragged_last_generation", n > cus and n % cus != 0),
                                   ) if hit}
    got.add("stagger_on" if pl["stagger_groups"] > 1 else "stagger_off")
    assert (pl["stagger_groups"] > 1) == (n >= 2 * cus)
    if LDS_LIMIT - 256 <= pl["lds"] <= LDS_LIMIT:
        got.add("lds_within_256_of_limit")
    return got


def reach_k1(c, cus=CENSUS_CUS):
    pl = case_pyramid_plan(c, cus)
    w, h = c["w"], c["h"]
    got = {"k1", "two_levels_k1" if c["levels"] == 2 else "sums_only"}
    if pl["vec"]:
        chunks, h1, rows = w // 16, h // 2, pl["rows_per_strip"]
        got.add("vec")
        if chunks in (2, 3, 1024):
            got.add(f"vec_chunks_{chunks}")
        if chunks < K1_ITEMS and K1_ITEMS % chunks:
            got.add("vec_chunks_non_divisor")
        if chunks > K1_ITEMS:
            got.add("vec_rows_clamped_to_1")
        if pl["nstrips"] == 1 and h1 * chunks < K1_THREADS:
            got.add("vec_single_strip_under_256_items")
        if h1 % rows:
            got.add("vec_partial_last_strip")
            if h1 % rows == 1 and pl["nstrips"] > 1:
                got.add("vec_one_leftover_row")
        elif pl["nstrips"] > 1:
            got.add("vec_h1_multiple_of_rows")
        if c["sequence"]:
            got.add("sequence_vec")
    else:
        got.add("scalar")
        why = [k for k, v in pl["scalar_by"].items() if v]
        if len(why) == 1:
            got.add("scalar_by_" + why[0] + "_alone")
        if w % 2 or h % 2:
            got.add({(1, 0): "odd_w", (0, 1): "odd_h", (1, 1): "odd_both"}[(w % 2, h % 2)])
        cells = ((w + 1) // 2) * ((h + 1) // 2)
        if cells % K1_ITEMS == 0:
            got.add("cells_multiple_of_1024")
        if cells % K1_ITEMS == 1:
            got.add("cells_multiple_of_1024_plus_1")
        if c["sequence"]:
            got.add("sequence_scalar")
    return got


def reach(c, cus=CENSUS_CUS):
    """The names of the paths the case takes (VOCABULARY)."""
    kind = coarse_kind(c, cus)
    if kind == "small":
        return {"small_class"}
    if kind == "fused":
        return reach_coarse(c, cus)
    assert kind == "k1", (c["id"], kind)
    got = reach_k1(c, cus)
    if c["levels"] == 2 and not c["split"]:
        got.add("fallback_" + case_coarse_plan(c, cus)["verdict"])
    return got


VOCABULARY = (
    ["fused", "rpi_eq_rmax", "rpi_lt_rmax", "rpi_1", "idle_lanes_0", "idle_lanes_some", "chunks_2", "chunks_256", "chunks_257", "chunks_512",
     "h1_lt_rpi", "last_sweep_full", "last_sweep_partial", "pad_0", "pad_2", "pad_4", "pad_6", "pad_6_nkf_1", "nb_1", "nb_under_64",
     "nb_512", "nb_513", "nb_over_1024", "rounds_2", "one_generation", "pairs_cus_minus_1", "pairs_cus", "pairs_cus_plus_1",
     "pairs_2cus_minus_1", "pairs_2cus", "pairs_2cus_plus_1", "three_pairs_per_workgroup", "ragged_last_generation", "stagger_on",
     "stagger_off", "lds_within_256_of_limit", "small_class"]
    + ["fallback_" + v for v in ("lds", "chunks", "width", "stride", "prev", "cur", "subpixel", "search", "tile")]
    + ["k1", "two_levels_k1", "sums_only", "vec", "vec_chunks_2", "vec_chunks_3", "vec_chunks_non_divisor", "vec_chunks_1024",
       "vec_rows_clamped_to_1", "vec_single_strip_under_256_items", "vec_partial_last_strip", "vec_one_leftover_row",
       "vec_h1_multiple_of_rows", "scalar", "scalar_by_width_alone", "scalar_by_height_alone", "scalar_by_stride_alone",
       "scalar_by_prev_alone", "scalar_by_cur_alone", "odd_w", "odd_h", "odd_both", "cells_multiple_of_1024",
       "cells_multiple_of_1024_plus_1", "sequence_vec", "sequence_scalar"])

# paths a first-failing verdict has that no device launch can take: the parameter check or the grid refuses them first
UNREACHABLE_VERDICTS = {"height": "two levels need an even height (aof_params_check)", "grid": "the dense level-1 grid of tile 8, search 4 IS (4, 4) step 8",
                        "bins": "search 4 votes into 19 bins", "pairs": "more pairs than any device holds frames for"}

CUS = lambda a, b: ("cus", a, b)

# 64 x 48 (35 blocks at level 0, 6 at level 1: the level-1 grid keeps it out of the small class at any pair count): the pair
# count against the CU count, about 50 distinct pairs
GENERATIONS = [
    case("64x48-cus-minus-1", 64, 48, CUS(1, -1), "one_generation", "pairs_cus_minus_1", "stagger_off", distinct=50),
    case("64x48-cus", 64, 48, CUS(1, 0), "pairs_cus", distinct=50),
    case("64x48-cus-plus-1", 64, 48, CUS(1, 1), "pairs_cus_plus_1", "ragged_last_generation", distinct=50),
    case("64x48-2cus-minus-1", 64, 48, CUS(2, -1), "pairs_2cus_minus_1", "stagger_off", "ragged_last_generation", distinct=50),
    case("64x48-2cus", 64, 48, CUS(2, 0), "pairs_2cus", "stagger_on", distinct=50),
    case("64x48-2cus-plus-1", 64, 48, CUS(2, 1), "pairs_2cus_plus_1", "stagger_on", distinct=50),
    case("64x48-3cus-plus-1", 64, 48, CUS(3, 1), "three_pairs_per_workgroup", "stagger_on", distinct=50),
]

FUSED = [
    case("32x32", 32, 32, 130, "chunks_2", "nb_1", "pad_6_nkf_1", "h1_lt_rpi", "rpi_lt_rmax", distinct=7),
    case("48x32", 48, 32, 130, "fused", "nb_under_64", distinct=7),
    case("96x96", 96, 96, 130, "fused", "nb_under_64", distinct=7),
    case("8192x32", 8192, 32, 3, "chunks_512", "rpi_1", "idle_lanes_0", "rpi_eq_rmax"),
    case("8192x38", 8192, 38, 2, "chunks_512", "rpi_1", "pad_2"),
    case("4112x32", 4112, 32, 3, "chunks_257", "idle_lanes_some", "rpi_1"),
    case("4096x32", 4096, 32, 3, "chunks_256", "rpi_eq_rmax", "idle_lanes_0"),
    case("4096x38", 4096, 38, 3, "chunks_256", "rpi_1", "rpi_lt_rmax"),
    case("32x10014", 32, 10014, 3, "lds_within_256_of_limit", "chunks_2", "rounds_2"),
    case("528x272", 528, 272, 3, "nb_512"),
    case("448x320", 448, 320, 3, "nb_513", "rounds_2"),
    case("1040x290", 1040, 290, 3, "pad_6"),
    case("1040x294", 1040, 294, 3, "pad_6"),
    case("1184x98", 1184, 98, 3, "pad_4"),
    case("112x168", 112, 168, 130, "pad_2", distinct=7),
    case("256x256", 256, 256, 3, "rpi_eq_rmax", "idle_lanes_0", "last_sweep_full"),
    case("640x480", 640, 480, 3, "nb_over_1024", "pad_0", "last_sweep_full"),
    case("96x96-7-small-class", 96, 96, 7, "small_class"),
]

FALLBACKS = [
    case("32x10016-over-lds", 32, 10016, 3, "fallback_lds"),
    case("8192x40-over-lds", 8192, 40, 2, "fallback_lds"),
    case("8208x32-513-chunks", 8208, 32, 3, "fallback_chunks", "vec_chunks_non_divisor"),
    case("72x48-width-8-mod-16", 72, 48, 130, "fallback_width", "scalar_by_width_alone", distinct=7),
    case("64x48-stride-plus-8", 64, 48, 130, "fallback_stride", "scalar_by_stride_alone", stride_extra=8, distinct=7),
    case("64x48-prev-off-8", 64, 48, 130, "fallback_prev", "scalar_by_prev_alone", prev_off=8, distinct=7),
    case("64x48-cur-off-4", 64, 48, 130, "fallback_cur", "scalar_by_cur_alone", cur_off=4, distinct=7),
    case("64x48-subpixel", 64, 48, 130, "fallback_subpixel", subpixel=1, distinct=7),
    case("64x48-search-3", 64, 48, 130, "fallback_search", search=3, distinct=7),
    case("128x96-tile-16", 128, 96, 130, "fallback_tile", tile=16, search=8, distinct=7),
]

K1 = [
    case("k1-32x32", 32, 32, 130, "vec_chunks_2", "vec_single_strip_under_256_items", "two_levels_k1", split=True, distinct=7),
    case("k1-32x32-sums", 32, 32, 130, "vec_chunks_2", "sums_only", levels=1, split=True, distinct=7),
    case("k1-48x1040", 48, 1040, 5, "vec_chunks_3", "vec_chunks_non_divisor", "vec_partial_last_strip", split=True),
    case("k1-48x1040-sums", 48, 1040, 5, "vec_chunks_3", "sums_only", levels=1, split=True),
    case("k1-16384x32", 16384, 32, 2, "vec_chunks_1024", "vec_h1_multiple_of_rows", split=True),
    case("k1-16384x32-sums", 16384, 32, 2, "vec_chunks_1024", "sums_only", levels=1, split=True),
    case("k1-16400x32", 16400, 32, 2, "vec_rows_clamped_to_1", split=True),
    case("k1-16400x32-sums", 16400, 32, 2, "vec_rows_clamped_to_1", "sums_only", levels=1, split=True),
    case("k1-64x1024-exact-strips", 64, 1024, 5, "vec_h1_multiple_of_rows", split=True),        # 512 rows: two strips of 256
    case("k1-64x514-one-leftover-row", 64, 514, 5, "vec_one_leftover_row", "vec_partial_last_strip", split=True),
    case("k1-50x46", 50, 46, 130, "scalar", "two_levels_k1", split=True, distinct=7),
    case("k1-51x46-sums", 51, 46, 130, "odd_w", "sums_only", levels=1, split=True, distinct=7, edge=True),
    case("k1-50x47-sums", 50, 47, 130, "odd_h", "sums_only", levels=1, split=True, distinct=7, edge=True),
    case("k1-51x47-sums", 51, 47, 130, "odd_both", "sums_only", levels=1, split=True, distinct=7, edge=True),
    case("k1-48x47-height-alone-sums", 48, 47, 130, "scalar_by_height_alone", "odd_h", levels=1, split=True, distinct=7, edge=True),
    case("k1-40x512-cells-5120", 40, 512, 130, "cells_multiple_of_1024", split=True, distinct=7),  # 20 x 256 = 5 x 1 024
    case("k1-63x64-cells-1024-sums", 63, 64, 130, "cells_multiple_of_1024", "odd_w", levels=1, split=True, distinct=7),
    case("k1-cells-1025", 82, 50, 130, "cells_multiple_of_1024_plus_1", split=True, distinct=7),  # 41 x 25 = 1 025
    case("k1-64x48-scalar-by-base", 64, 48, 130, "scalar_by_prev_alone", split=True, prev_off=4, distinct=7),
] + [case(f"k1-sequence-vec-{n}", 64, 48, n, "sequence_vec", split=True, sequence=True) for n in (1, 2, 5)] \
  + [case(f"k1-sequence-scalar-{n}", 72, 48, n, "sequence_scalar", split=True, sequence=True) for n in (1, 2, 5)]

GPU_CASES = GENERATIONS + FUSED + FALLBACKS + K1


def plan_case(id, w, h, n_pairs, **kw):
    """A launch for the plans and the decode alone."""
    return case(id, w, h, n_pairs, **kw)


CPU_CASES = [
    plan_case("16x32-one-chunk", 16, 32, 1),
    plan_case("vga-1024", 640, 480, 1024),
    plan_case("672x464", 672, 464, 7),
    plan_case("160x128", 160, 128, 7),
    plan_case("320x66", 320, 66, 7),
    plan_case("96x64-1100", 96, 64, 1100),
    plan_case("8176x34-511-chunks", 8176, 34, 1),
    plan_case("4080x36-255-chunks", 4080, 36, 1),
    plan_case("k1-1023-chunks", 16368, 34, 1, split=True),
    plan_case("k1-odd-3x3", 3, 3, 2, levels=1, split=True),
    plan_case("k1-1x1", 1, 1, 2, levels=1, split=True),
    plan_case("k1-2047-cells", 89, 46, 3, levels=1, split=True),     # 45 x 23 = 1 035
    plan_case("k1-sequence-3-odd", 51, 47, 3, levels=1, split=True, sequence=True),
]

# the plans alone, against the C++ functions: up to the ABI's 2^24 pixels and pair counts near 2^31.  (w, h, pair_stride,
# prev, cur, tile, search, subpixel, n_pairs, cus, sequence, sums)
PLAN_ONLY = [
    dict(id="4096x4096", w=4096, h=4096, n_pairs=3, cus=256),
    dict(id="16x1048576", w=16, h=1 << 20, n_pairs=3, cus=256),
    dict(id="16777216x1", w=1 << 24, h=1, n_pairs=2, cus=256),
    dict(id="1048576x16", w=1 << 20, h=16, n_pairs=2, cus=256),
    dict(id="2^31-1-pairs", w=64, h=48, n_pairs=0x7FFFFFFF, cus=256),
    dict(id="2^31-pairs", w=64, h=48, n_pairs=0x80000000, cus=256),
    dict(id="2^30-pairs-total-2^31", w=64, h=48, n_pairs=1 << 30, cus=256),
    dict(id="2^30-minus-1-pairs", w=64, h=48, n_pairs=(1 << 30) - 1, cus=256),
    dict(id="sequence-2^31-frames", w=64, h=48, n_pairs=0x80000000, cus=256, sequence=1),
    dict(id="sequence-one-frame", w=64, h=48, n_pairs=1, cus=256, sequence=1),
    dict(id="no-sums", w=64, h=48, n_pairs=9, cus=256, sums=0),
    dict(id="one-cu", w=64, h=48, n_pairs=9, cus=1),
    dict(id="304-cus", w=640, h=480, n_pairs=608, cus=304),
    dict(id="303-pairs-304-cus", w=640, h=480, n_pairs=607, cus=304),
    dict(id="odd-height-two-levels", w=64, h=47, n_pairs=9, cus=256),
    dict(id="stride-huge", w=64, h=48, n_pairs=9, cus=256, pair_stride=(1 << 40) + 16),
    dict(id="range-16-bins", w=640, h=480, n_pairs=9, cus=256, rng=16),
    dict(id="tile-16", w=640, h=480, n_pairs=9, cus=256, tile=16, search=8),
    dict(id="plan-32x10014", w=32, h=10014, n_pairs=9, cus=256),
    dict(id="plan-32x10016", w=32, h=10016, n_pairs=9, cus=256),
]


def plan_args(c, cus=CENSUS_CUS):
    """A case of any list as the arguments of both plans: dict(w, h, pair_stride, prev, cur, tile, search, subpixel, rng,
    grid (level 1), n_pairs, cus, sequence, k1_n (what K1 is given), sums)."""
    if "paths" in c:
        stride, prev, cur = frame_layout(c)
        n = n_pairs_of(c, cus)
        return dict(w=c["w"], h=c["h"], pair_stride=stride, prev=prev, cur=cur, tile=c["tile"], search=c["search"], subpixel=c["subpixel"],
                    rng=c["search"], grid=dense_grid(c["w"], c["h"], 1, c["tile"], c["search"], c["subpixel"]), n_pairs=n, cus=cus,
                    sequence=int(c["sequence"]), k1_n=n + 1 if c["sequence"] else n, sums=int(bool(c["mean_subtract"])))
    tile, search, sub = c.get("tile", 8), c.get("search", 4), c.get("subpixel", 0)
    return dict(w=c["w"], h=c["h"], pair_stride=c.get("pair_stride", c["w"] * c["h"]), prev=c.get("prev", BASE), cur=c.get("cur", BASE + (1 << 40)),
                tile=tile, search=search, subpixel=sub, rng=c.get("rng", search), grid=dense_grid(c["w"], c["h"], 1, tile, search, sub),
                n_pairs=c["n_pairs"], cus=c["cus"], sequence=c.get("sequence", 0), k1_n=c["n_pairs"], sums=c.get("sums", 1))


def plans_of(c, cus=CENSUS_CUS):
    a = plan_args(c, cus)
    return (coarse_plan(a["w"], a["h"], a["pair_stride"], a["prev"], a["cur"], a["grid"], a["rng"], a["tile"], a["search"], a["subpixel"],
                        a["n_pairs"], a["cus"]),
            pyramid_plan(a["w"], a["h"], a["pair_stride"], a["prev"], a["cur"], a["sequence"], a["k1_n"], bool(a["sums"])))


def selftest_families():
    """coarse_plan_make == coarse_plan() and pyramid_plan_make == pyramid_plan(), on every case of every list.  The cases as
    tests/native/host_selftest.cpp reads them:
    coarse: w h pair_stride prev cur x0 y0 step_x step_y nx ny range tile search subpixel n_pairs cus
    pyramid: w h pair_stride prev cur sequence n_pairs sums"""
    def coarse_line(c):
        a = plan_args(c)
        return rig.joined([a["w"], a["h"], a["pair_stride"], a["prev"], a["cur"], *a["grid"], a["rng"], a["tile"], a["search"], a["subpixel"],
                           a["n_pairs"], a["cus"]])

    def pyramid_line(c):
        a = plan_args(c)
        return rig.joined([a["w"], a["h"], a["pair_stride"], a["prev"], a["cur"], a["sequence"], a["k1_n"], a["sums"]])

    cases = CPU_CASES + GPU_CASES + PLAN_ONLY
    return [rig.family("coarse-plan", "coarse plan: ", cases, coarse_line, lambda c: _coarse_fields(plans_of(c)[0]), COARSE_FIELDS),
            rig.family("pyramid-plan", "pyramid plan: ", cases, pyramid_line, lambda c: [plans_of(c)[1][k] for k in PYRAMID_FIELDS], PYRAMID_FIELDS)]


# ---- the frames of a device case ---------------------------------------------------------------------------------------

SHIFT_REACH, NOISE = 9, 3
# what distinct pair j holds, by j % len: textured pairs at their own shift and brightness, and the suite's hard cases
KINDS = ("tex", "tex", "flat-half", "tex", "saturated", "black-prev", "tex", "inverted", "tex", "identical", "tex", "tex", "level", "tex",
         "tex", "saturated", "tex")
CHAIN_STEP = 11   # consecutive pairs of a workgroup hold contents CHAIN_STEP apart (see pair_contents)
# level-1 blocks whose tile is flattened in prev (gated), by content: none, each of six, each two of six -- contents
# CHAIN_STEP apart never share a mask
MASKS = [()] + [(b,) for b in range(6)] + [(a, b) for a in range(6) for b in range(a + 1, 6)]
assert len(MASKS) == 2 * CHAIN_STEP


def distinct_frames(c, synth, cus=CENSUS_CUS):
    """The case's distinct pairs (prevs, curs: uint8 [k, h, w]) and their kinds.  Every pair has its own shift of up to
    +-9 pixels, noise of +-3 and its own brightness offset; 'flat-half': the upper half flat in both frames (gated
    blocks); 'saturated': cur doubled and clamped; 'black-prev': everything gated; 'inverted'; 'identical' (and with it
    delta == 0); 'level': no brightness offset (delta == 0 behind pairs that have one).  Where the case says `edge`, the
    last column and row are raised in prev and lowered in cur, far enough to move both rounded means."""
    k, w, h = distinct_pairs(c, cus), c["w"], c["h"]
    prevs, curs, kinds = np.empty((k, h, w), np.uint8), np.empty((k, h, w), np.uint8), []
    for j in range(k):
        kind = KINDS[j % len(KINDS)] if k > 1 else "tex"
        bright = 0 if kind in ("level", "identical") or not c["mean_subtract"] else (4 + 2 * (j % 13)) * (1 if j % 2 else -1)
        shift = ((5 * j + 3) % 19 - 9, (7 * j + 5) % 19 - 9)      # contents CHAIN_STEP apart: 2 or 17 pixels apart on both axes
        a, b, _ = synth.make_pair(w, h, SHIFT_REACH, 7700 + 31 * j + w, shift=shift, noise=NOISE, brightness=bright)
        a, b = a.copy(), b.copy()
        if c["distinct"] == 50:   # (the generation cases: 3 x 2 level-1 blocks, a tile of 16 x 16 level-0 pixels each)
            for blk in MASKS[j % len(MASKS)]:
                y0, x0 = 8 + 16 * (blk // 3), 8 + 16 * (blk % 3)
                a[y0:y0 + 16, x0:x0 + 16] = 90
        if kind == "flat-half":
            a[: h // 2], b[: h // 2] = 7, 7
        elif kind == "saturated":
            b = np.minimum(b.astype(np.int32) * 2, 255).astype(np.uint8)
        elif kind == "black-prev":
            a[:] = 0
        elif kind == "inverted":
            a, b = 255 - a, 255 - b
        elif kind == "identical":
            b = a.copy()
        if c["edge"]:
            a[:, w - 1], a[h - 1, :] = 255, 255
            b[:, w - 1], b[h - 1, :] = 0, 0
        prevs[j], curs[j] = a, b
        kinds.append(kind)
    return prevs, curs, kinds


def pair_contents(n, k, wgs):
    """Which distinct pair each pair of the launch holds: workgroup s walks pairs s, s + wgs, ...; its g-th pair holds
    content (s + CHAIN_STEP g) % k, so that consecutive pairs of a workgroup always differ and, with k >= 50, every
    (content, content + CHAIN_STEP) ordering occurs.  One generation: content i % k."""
    i = np.arange(n)
    return (i % wgs + CHAIN_STEP * (i // wgs)) % k


def sequence_frames(c, synth):
    """n_pairs + 1 frames of a panning camera with a brightness ramp (every pair has a delta)."""
    n = n_pairs_of(c) + 1
    frames = synth.make_sequence(c["w"], c["h"], n, SHIFT_REACH, seed=11, max_step=6)[0].astype(np.int32)
    frames += (7 * np.arange(n))[:, None, None]
    frames += np.random.default_rng(4242).integers(-NOISE, NOISE + 1, size=frames.shape)
    return np.clip(frames, 0, 255).astype(np.uint8)


def rounded_mean(img, cols=None, rows=None):
    """(sum + n / 2) / n over the first `cols` columns and `rows` rows (default: all)."""
    part = img[:rows, :cols]
    return (int(part.sum(dtype=np.uint64)) + part.size // 2) // part.size


def check_edge_moves_delta(c, prevs, curs):
    """One level, odd sizes: without the last column, the last row, or both, every pair's delta would be another."""
    w, h = c["w"], c["h"]
    cuts = {(w - w % 2, h - h % 2), (w - w % 2, h), (w, h - h % 2)} - {(w, h)}
    assert cuts, c["id"]
    for a, b in zip(prevs, curs):
        whole = rounded_mean(a) - rounded_mean(b)
        for cols, rows in cuts:
            assert rounded_mean(a, cols, rows) - rounded_mean(b, cols, rows) != whole, (c["id"], cols, rows)


def oracle_facts(aof, orc, synth, c, cus=CENSUS_CUS):
    """Per distinct pair of a two-level case, from the oracle: pixel sums, delta, gated level-1 blocks, level-1 records,
    predictor, votes."""
    p = orc.params_from(aof.default_params(c["w"], c["h"], **params_kw(c)))
    prevs, curs, kinds = distinct_frames(c, synth, cus)
    facts = []
    for a, b, kind in zip(prevs, curs, kinds):
        out = orc.flow_pair(p, a, b, want_l1=True)
        b1 = out["blocks_l1"]
        a1, c1 = orc.pyramid_down(a), orc.pyramid_down(b)
        sums = tuple(int(x.sum(dtype=np.uint64)) for x in (a, a1, b, c1))
        f1, px, py = orc.reduce(p, b1, None, p.search)
        facts.append(dict(kind=kind, sums=sums, delta=rounded_mean(a1) - rounded_mean(c1), gated=tuple(b1["sad"] == 0xFFFF), b1=b1.tobytes(),
                          pred=(int(out["flow"]["pred_x"]), int(out["flow"]["pred_y"])), votes=int(f1["count"])))
    return facts


def check_chains(facts, contents, wgs, orderings):
    seen = set()
    for first in range(min(wgs, len(contents))):
        chain = contents[first::wgs]
        for a, b in zip(chain[:-1], chain[1:]):
            x, y = facts[a], facts[b]
            assert x["sums"] != y["sums"] and x["delta"] != y["delta"] and x["gated"] != y["gated"] and x["b1"] != y["b1"], (a, b)
            if x["kind"] == y["kind"] == "tex":
                assert x["pred"] != y["pred"], (a, b)
            voted = lambda f: f["votes"] >= 3 and not all(f["gated"])
            if voted(x) and all(y["gated"]):
                seen.add("gated behind voted")
            if all(x["gated"]) and voted(y):
                seen.add("voted behind gated")
            if x["delta"] != 0 and y["delta"] == 0 and voted(x):
                seen.add("level behind stepped")
    if orderings:
        assert seen == {"gated behind voted", "voted behind gated", "level behind stepped"}, seen
