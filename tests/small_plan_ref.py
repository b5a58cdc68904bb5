"""The launch plans of the small-pair kernels in plain Python -- the one-workgroup class that runs flow_small_pair
(csrc/aof_small_plan.hpp: small_plan_make) and the grouped lane-per-block search k_flow_lane8 (lane8_group_plan) --, what
the kernels make of them lane by lane (passes A, B, C and D1 of csrc/aof_flow_small.hpp, the (workgroup, lane) -> (pair,
block) map of k_flow_lane8), which kernels serve a batch (batch_plan_ref.py, the model of aof_batch_plan.hpp: plan_batch), the names of the paths a launch
can take through all of it, and the case lists of tests/test_small_plan_ref.py, tests/test_host_asan.py (the same plans
from the C++ functions) and tests/test_gpu_small_plan.py (every case of GPU_CASES on the device, against the oracle).

Written from DESIGN.md ("Kernels": KS, K2) and the kernels' comments:

  A   both level-0 frames as 16-byte chunks in ONE item space (buffer `first`, then the other), rounds of 8 x 256 chunks:
      item (trip * 8 + k) * 256 + lane.  `load` 1 or 2 fetches one buffer only (the resident kernel).
  B   two levels: one 8-byte piece of a level-1 row per lane and trip, both buffers in one item space again.
  C   per level one lane per (block, dy): item = block * 9 + dy, 256 items per trip.  A lane reads its 8 tile rows with
      three aligned dwords each and its 8 window rows with five: up to three bytes in front of the first and seven behind
      the last byte it needs.  Behind a frame lie 16 bytes of padding for that.
  D1  half-pixel refinement: four lanes per block, padded to whole waves; window rows with four aligned dwords.
  K2  k_flow_lane8: a workgroup of 256 lanes owns ppw = 256 / nb whole pairs, lane t is block t % nb of pair t / nb.

No device case's shape is typed in here: a case names a width (or the widths to choose among) and the property it is
there for, and the height comes from the grid rule (grid_for_level).  Only the workload's own shapes among CPU_CASES and the
extreme shapes of PLAN_ONLY are written out."""
import numpy as np

import selftest_rig as rig

# csrc/aof_small_plan.hpp
THREADS, MAX_BINS, LOADS, PAD = 256, 64, 8, 16
STATIC_LDS, LDS_LIMIT, ATTR_ABOVE = 4096, 160 * 1024, 48 * 1024
TRIP_A = LOADS * THREADS
ZERO_COPY_MAX = 64 * 1024   # aof_percall.cpp: the per-call paths read frames up to here from pinned host memory (tagged, resident)
# the verdict of flow_small_supported: the first condition that fails (enum SmallVerdict, in this order)
VERDICTS = ("ok", "levels", "tile", "pairs", "grid0", "bins0", "width", "stride", "prev", "cur", "subdirs0", "height", "grid1", "bins1",
            "subdirs1", "lds")
# verdicts no device launch can end on: something in front of flow_small_supported refuses the configuration first
UNREACHABLE_VERDICTS = {
    "levels": "aof_params_check knows one and two levels only",
    "tile": "plan_batch asks only where level 0 runs the grouped 8x8 / +-4 search",
    "pairs": "2^23 pairs of at least 1 152 bytes per frame: more than the cases' device bytes",
    "grid0": "plan_batch asks only where level 0's grid has 8 .. 256 blocks (lane8_group)",
    "bins0": "a search range of 4 votes into 19 or 55 bins",
    "subdirs0": "the C entry points refuse half-pixel refinement without an array of directions",
    "height": "aof_params_check refuses two levels at an odd height",
    "grid1": "plan_batch asks only where level 1's grid has 8 .. 256 blocks",
    "bins1": "a search range of 4 votes into 19 bins",
    "subdirs1": "the workspace always holds level 1's directions",
}
BASE = 0x7F0000000000   # a frame address for the plans: 16-byte aligned


def grid_for_level(w, h, level=0, px4=False, subpixel=0, tile=8, search=4, num_blocks=5):
    """(x0, y0, step_x, step_y, nx, ny) of a level's grid (aof_params.cpp), or None where there is none."""
    w, h = w >> level, h >> level
    if not px4:
        m = search + (1 if subpixel else 0)
        g = (m, m, tile, tile, (w - 2 * m) // tile, (h - 2 * m) // tile)
    else:
        lo, hix, hiy = search + 1, w - (search + 1) - tile, h - (search + 1) - tile
        if hix <= lo or hiy <= lo:
            return None
        sx, sy = (hix - lo) // num_blocks + 1, (hiy - lo) // num_blocks + 1
        g = (lo, lo, sx, sy, (hix - lo + sx - 1) // sx, (hiy - lo + sy - 1) // sy)
    return g if g[4] >= 1 and g[5] >= 1 else None


def blocks(g):
    return 0 if g is None else g[4] * g[5]


def level_range(levels, level, search=4):
    return 3 * search + 1 if levels == 2 and level == 0 else search


# ---- the two plans -----------------------------------------------------------------------------------------------------

def trips(items, per):
    return 0 if items <= 0 else -(-items // per)


def small_lds(w, h, levels):
    frame0, frame1 = w * h, (w // 2) * (h // 2)
    return 2 * (frame0 + PAD) + (2 * ((frame1 + PAD + 15) & ~15) if levels == 2 else 0)


def small_plan(w, h, levels, g0, g1, n_pairs, pair_stride, prev, cur, subpixel=0, tile=8, search=4, rng0=None, rng1=None, subdirs0=1,
               subdirs1=1, l1_w=None, l1_h=None):
    """small_plan_make.  g0, g1: the levels' grids as tuples (None: no block).  subdirs0 / subdirs1: a place for the
    directions is given.  l1_w, l1_h: level 1's size as the caller states it (default: half of level 0)."""
    two = levels == 2
    rng0 = level_range(levels, 0, search) if rng0 is None else rng0
    rng1 = level_range(levels, 1, search) if rng1 is None else rng1
    l1_w, l1_h = w // 2 if l1_w is None else l1_w, h // 2 if l1_h is None else l1_h
    nb0, nb1 = blocks(g0), blocks(g1)
    frame0, frame1 = w * h, (w // 2) * (h // 2)
    lds = small_lds(w, h, levels)
    f1_0 = 2 * (frame0 + PAD)
    pl = dict(w=w, h=h, levels=levels, g0=g0, g1=g1, nb=(nb0, nb1), subpixel=int(bool(subpixel)), lds=lds, f0=(0, frame0 + PAD),
              f1=(f1_0, f1_0 + ((frame1 + PAD + 15) & ~15)) if two else (0, 0), attr=int(lds > ATTR_ABOVE),
              trips_a=(trips(frame0 // 16, TRIP_A), trips(frame0 // 16, TRIP_A), trips(2 * (frame0 // 16), TRIP_A)),
              trips_b=(trips((h // 2) * (w // 16), THREADS), trips(2 * (h // 2) * (w // 16), THREADS)) if two else (0, 0))
    ok_nb = [1 <= nb <= THREADS for nb in (nb0, nb1)]
    live = [ok_nb[0], two and ok_nb[1]]
    pl["trips_c"] = tuple(trips(nb * 9, THREADS) if on else 0 for nb, on in zip((nb0, nb1), live))
    pl["trips_d1"] = tuple(trips((4 * nb + 63) // 64 * 64, THREADS) if on and subpixel else 0 for nb, on in zip((nb0, nb1), live))
    tests = [("levels", levels not in (1, 2)), ("tile", tile != 8 or search != 4), ("pairs", n_pairs < 1 or n_pairs > 0x7FFFFFFF // THREADS),
             ("grid0", not ok_nb[0]), ("bins0", 2 * (2 * rng0 + 1) + 1 > MAX_BINS), ("width", w % 16 != 0),
             ("stride", n_pairs > 1 and pair_stride % 16 != 0), ("prev", prev % 16 != 0), ("cur", cur % 16 != 0),
             ("subdirs0", bool(subpixel) and not subdirs0)]
    if two:
        tests += [("height", h % 2 != 0 or l1_w != w // 2 or l1_h != h // 2), ("grid1", not ok_nb[1]),
                  ("bins1", 2 * (2 * rng1 + 1) + 1 > MAX_BINS), ("subdirs1", bool(subpixel) and not subdirs1)]
    tests.append(("lds", lds + STATIC_LDS > LDS_LIMIT))
    pl["verdict"] = next((name for name, fails in tests if fails), "ok")
    return pl


PLAN_FIELDS = ("verdict", "lds", "f0[0]", "f0[1]", "f1[0]", "f1[1]", "attr", "a[1]", "a[2]", "a[3]", "b[1]", "b[2]", "c[0]", "c[1]", "d1[0]", "d1[1]")


def _plan_fields(pl):
    """The plan as the flat list of numbers the host self-test prints for small_plan_make (PLAN_FIELDS)."""
    return [VERDICTS.index(pl["verdict"]), pl["lds"], *pl["f0"], *pl["f1"], pl["attr"], *pl["trips_a"], *pl["trips_b"], *pl["trips_c"],
            *pl["trips_d1"]]


def lane8_supported(w, h, nb, n_pairs, pair_stride, tile=8, search=4):
    if tile != 8 or search != 4:
        return False
    frame = w * h
    if frame > 1 << 24 or nb < 1 or nb >= 1 << 24:
        return False
    return not (n_pairs > 1 and (pair_stride < 0 or (64 // nb + 2) * pair_stride + frame > 0xFFFFFFFF))


def group_plan(w, h, g, n_pairs, pair_stride, rng, tile=8, search=4):
    """lane8_group_plan: ppw (0: the grid does not qualify), workgroups, live lanes of the last one, LDS bytes."""
    nb = blocks(g)
    pl = dict(nb=nb, n_pairs=n_pairs, ppw=0, wgs=0, last_live=0, lds=0)
    if not lane8_supported(w, h, nb, n_pairs, pair_stride, tile, search) or nb < 8 or nb > THREADS:
        return pl
    ppw = THREADS // nb
    pl.update(ppw=ppw, lds=ppw * 2 * max(0, 2 * (2 * rng + 1) + 1) * 4)
    if n_pairs >= 1:
        wgs = -(-n_pairs // ppw)
        pl.update(wgs=wgs, last_live=(n_pairs - (wgs - 1) * ppw) * nb)
    return pl


GROUP_FIELDS = ("ppw", "wgs", "last_live", "lds")


# ---- the decodes ---------------------------------------------------------------------------------------------------------

def first_count(load):
    """The buffers `load` names: (first, count)."""
    return (0 if load & 1 else 1), (2 if load == 3 else 1 if load else 0)


def pass_a(pl, load):
    """Every (trip, k, lane) of pass A that fetches: arrays trip, k, lane, buffer, chunk."""
    per_frame = pl["w"] * pl["h"] // 16
    first, count = first_count(load)
    items = count * per_frame
    t, k, lane = np.meshgrid(np.arange(trips(items, TRIP_A)), np.arange(LOADS), np.arange(THREADS), indexing="ij")
    it = (t * TRIP_A + k * THREADS + lane).ravel()
    keep = it < items
    it = it[keep]
    second = (it >= per_frame).astype(np.int64)
    return dict(trip=t.ravel()[keep], k=k.ravel()[keep], lane=lane.ravel()[keep], buf=first + second, chunk=it - second * per_frame, items=items,
                per_frame=per_frame)


def pass_b(pl, load):
    """Every (trip, lane) of pass B that filters: arrays trip, lane, buffer, level-1 row, 8-byte piece."""
    chunks, h1 = pl["w"] // 16, pl["h"] // 2
    per_frame = h1 * chunks
    first, count = first_count(load)
    items = count * per_frame
    t, lane = np.meshgrid(np.arange(trips(items, THREADS)), np.arange(THREADS), indexing="ij")
    it = (t * THREADS + lane).ravel()
    keep = it < items
    it = it[keep]
    second = (it >= per_frame).astype(np.int64)
    rest = it - second * per_frame
    return dict(trip=t.ravel()[keep], lane=lane.ravel()[keep], buf=first + second, y1=rest // chunks, piece=rest % chunks, items=items,
                per_frame=per_frame)


def level_frame(pl, level):
    return (pl["w"] >> level, pl["h"] >> level)


def dword_span(off, n_dwords):
    """The bytes an unaligned LDS read of n_dwords aligned dwords touches: [begin, end) relative to the frame."""
    begin = off & ~3
    return begin, begin + 4 * n_dwords


def pass_c(pl, level, pred=(0, 0)):
    """Every item of pass C: arrays trip, lane, block, dy, searched (the window with its ring lies in the frame), and for
    the searched ones the bytes read relative to the frames: tile rows of the older frame (three dwords each), window rows
    of the newer one (five dwords: the q[4] of lds_bytes16)."""
    W, H = level_frame(pl, level)
    x0, y0, sx, sy, nx, ny = pl["g1" if level else "g0"]
    nb, ring = nx * ny, pl["subpixel"]
    it = np.arange(nb * 9)
    blk, d = it // 9, it % 9
    by, bx = blk // nx, blk % nx
    i, j = x0 + bx * sx, y0 + by * sy
    wx0, wy0 = i + pred[0] - 4, j + pred[1] - 4
    searched = ~((wx0 - ring < 0) | (wy0 - ring < 0) | (wx0 + 16 + ring > W) | (wy0 + 16 + ring > H))
    r = np.arange(8)[:, None]
    tile_lo, tile_hi = dword_span((j[None, :] + r) * W + i[None, :], 3)
    win_lo, win_hi = dword_span((wy0[None, :] + d[None, :] + r) * W + wx0[None, :], 5)
    need_hi = (wy0[None, :] + d[None, :] + r) * W + wx0[None, :] + 16
    return dict(trip=it // THREADS, lane=it % THREADS, block=blk, dy=d, searched=searched, i=i, j=j, wx0=wx0, wy0=wy0,
                tile=(tile_lo[:, searched], tile_hi[:, searched]), window=(win_lo[:, searched], win_hi[:, searched]),
                needed_end=need_hi[:, searched])


def pass_d1(pl, level, pred=(0, 0)):
    """Every lane of D1: arrays q, trip, lane, wave (of the workgroup), block (>= nb: padding), part; and the widest bytes
    a refining quad can read over all 81 best matches: (lo, hi) relative to the newer frame, for the blocks pass C searched."""
    W, H = level_frame(pl, level)
    x0, y0, sx, sy, nx, ny = pl["g1" if level else "g0"]
    nb = nx * ny
    q = np.arange((4 * nb + 63) // 64 * 64)
    blk, part = q // 4, q % 4
    c = pass_c(pl, level, pred)
    ok = np.zeros(nb, dtype=bool)
    ok[c["block"][c["searched"]]] = True
    live = blk < nb
    lo, hi = [], []
    b, p = blk[live & ok[np.minimum(blk, nb - 1)]], part[live & ok[np.minimum(blk, nb - 1)]]
    i, j = x0 + (b % nx) * sx, y0 + (b // nx) * sy + 2 * p
    for idx in (0, 8, 72, 80):       # the corners of the 9 x 9 candidates bound every other
        rx, ry = i + pred[0] - 4 + idx % 9 - 1, j + pred[1] - 4 + idx // 9 - 1
        for y in (-1, 2):
            s = dword_span((ry + y + 1) * W + rx, 4)
            lo.append(s[0])
            hi.append(s[1])
    return dict(q=q, trip=q // THREADS, lane=q % THREADS, wave=(q % THREADS) // 64, block=blk, part=part, live=live,
                span=(np.concatenate(lo), np.concatenate(hi)) if lo and b.size else (np.zeros(0, np.int64), np.zeros(0, np.int64)))


def grouped(pl, wg):
    """k_flow_lane8: lane -> (pair, block) of workgroup wg; pair -1: idle."""
    nb, ppw, n = pl["nb"], pl["ppw"], pl["n_pairs"]
    np_ = min(ppw, n - wg * ppw)
    lane = np.arange(THREADS)
    live = lane < np_ * nb
    return np.where(live, wg * ppw + lane // nb, -1), np.where(live, lane % nb, -1)


# ---- cases ---------------------------------------------------------------------------------------------------------------

def dense_height(w, nb, subpixel=0, level=0):
    """The smallest height at which the dense grid of a level of a w-wide frame has nb blocks (None: no such height)."""
    for h in range(16, 4200):
        g = grid_for_level(w, h, level, False, subpixel)
        if blocks(g) == nb:
            return h
        if blocks(g) > nb:
            return None
    return None


def dense_shape(nb, subpixel=0, widths=(16, 32, 48, 64, 80, 96, 112, 128, 144), nx=None):
    """The fewest bytes of a frame whose dense level-0 grid has nb blocks (nx: in that many columns)."""
    best = None
    for w in widths:
        if nx is not None and (grid_for_level(w, 4000, 0, False, subpixel) or (0,) * 6)[4] != nx:
            continue
        h = dense_height(w, nb, subpixel)
        if h is not None and (best is None or w * h < best[0] * best[1]):
            best = (w, h)
    assert best is not None, nb
    return best


def lds_edge_height(w, levels, over=False):
    """The last height whose frames fit the LDS limit (over: the first beyond it; two levels: even heights)."""
    step = 2 if levels == 2 else 1
    h = step
    while small_lds(w, h + step, levels) + STATIC_LDS <= LDS_LIMIT:
        h += step
    return h + step if over else h


def attr_edge_height(w, over=False):
    """The last height of a one-level frame at which the dynamic-LDS attribute is not set (over: the first where it is)."""
    h = 1
    while small_lds(w, h + 1, 1) <= ATTR_ABOVE:
        h += 1
    return h + 1 if over else h


def case(id, w, h, *tags, px4=False, levels=1, subpixel=None, mean_subtract=1, n_pairs=9, stride_extra=0, prev_off=0, cur_off=0,
         group=(), over_128=False, percall=False, threshold=None):
    """w x h frames on the dense grid (px4: the published sparse grid, with half-pixel refinement as it comes).  n_pairs:
    the pairs of the one launch (the eight distinct pairs and a replica of the first).  stride_extra / prev_off / cur_off: bytes between consecutive pairs beyond a frame, and
    the frame arrays' distance from a 16-byte boundary.  group: which pair counts the grouped search runs at, by name
    (ppw-1, ppw, ppw+1, kppw+1); over_128: also one launch of 129 pairs without the split switch.  percall: the per-call
    forms run too.  threshold: 'value' or 'feature' (the case takes that threshold from the oracle's records)."""
    subpixel = (1 if px4 else 0) if subpixel is None else subpixel
    return dict(id=id, w=w, h=h, tags=tags, px4=px4, levels=levels, subpixel=subpixel, mean_subtract=mean_subtract, n_pairs=n_pairs,
                stride_extra=stride_extra, prev_off=prev_off, cur_off=cur_off, group=tuple(group), over_128=over_128, percall=percall,
                threshold=threshold)


def grids(c):
    return tuple(grid_for_level(c["w"], c["h"], l, c["px4"], c["subpixel"]) if l < c["levels"] else None for l in (0, 1))


def frame_layout(c):
    """(pair_stride, prev, cur): as the device test places the frames."""
    return c["w"] * c["h"] + c["stride_extra"], BASE + c["prev_off"], BASE + (1 << 32) + c["cur_off"]


def case_plan(c, n_pairs=None):
    g0, g1 = grids(c)
    stride, prev, cur = frame_layout(c)
    return small_plan(c["w"], c["h"], c["levels"], g0, g1, c["n_pairs"] if n_pairs is None else n_pairs, stride, prev, cur, c["subpixel"])


def case_group_plan(c, n_pairs, level=0):
    g = grids(c)[level]
    w, h = c["w"] >> level, c["h"] >> level
    stride = (w * h) if level else frame_layout(c)[0]
    return group_plan(w, h, g, n_pairs, stride, level_range(c["levels"], level))


def kind(c, n_pairs=None, split=False):
    """'small' (one launch of the one-workgroup kernel) or 'separate' (plan_batch keeps the separate kernels):
    batch_plan_ref owns the rule."""
    import batch_plan_ref as bp
    return "small" if bp.plan(bp.of_small(c, n_pairs, split))["small"] else "separate"


def why_separate(c):
    """What keeps a case of `separate` kind out of the one launch: 'plan_grid0' / 'plan_grid1' (a level's search is not the
    grouped one), else the verdict of small_plan_make."""
    import batch_plan_ref as bp
    pl = bp.plan(bp.of_small(c))
    if pl["kind"][0] != "lane8_group":
        return "plan_grid0"
    if c["levels"] == 2 and pl["small_l1_kind"] != "lane8_group":
        return "plan_grid1"
    return pl["small_verdict"]


def counters(c, n_pairs=None, split=False):
    """The launches of one call by profiling counter [K_PYRAMID, K_SEARCH_L1, K_REDUCE_L1, K_SEARCH, K_REDUCE] (a flat
    search: K3 behind it, the in-launch reduction is the caller's switch)."""
    import batch_plan_ref as bp
    got = bp.plan(bp.of_small(c, n_pairs, split))["counters"]
    return [1 if got[k] is None else got[k] for k in bp.COUNTERS]


def group_counts(c):
    """The pair counts of the grouped launches of a case, from its plan: {name: n}."""
    ppw = case_group_plan(c, 1)["ppw"]
    k = 2 if ppw > 1 else 1
    table = {"ppw-1": ppw - 1, "ppw": ppw, "ppw+1": ppw + 1, "kppw+1": k * ppw + 1}
    return {name: table[name] for name in c["group"] if table[name] >= 1}


def params_kw(c):
    kw = dict(pyramid_levels=c["levels"], mean_subtract=c["mean_subtract"])
    if min(blocks(g) for g in grids(c) if g is not None) < 10:
        kw["min_valid"] = 0     # (a grid of fewer than ten blocks still yields a flow, and at level 1 a predictor)
    return kw


def resident_serves(c):
    """The per-call forms of a case run the tagged and the resident kernel: its frames are read from pinned host memory.
    Larger frames are copied to the device first and go through the batch plan."""
    return c["percall"] and c["w"] * c["h"] <= ZERO_COPY_MAX


def reach(c):
    """The names of the paths the case takes (VOCABULARY)."""
    pl = case_plan(c)
    g0, g1 = grids(c)
    nb0, nb1 = blocks(g0), blocks(g1)
    w, h, two, sub = c["w"], c["h"], c["levels"] == 2, c["subpixel"]
    got = set()
    if kind(c) == "separate":
        got.add("fallback_" + why_separate(c))
        if why_separate(c) == "lds":
            got.add("lds_one_step_over_two_levels" if c["levels"] == 2 else "lds_one_row_over_one_level")
        return got | group_reach(c)
    per_frame = w * h // 16
    items = 2 * per_frame
    resident = resident_serves(c)
    got.add("small")
    got |= {name for name, hit in (
        ("a_items_one_trip", items == TRIP_A), ("a_items_just_over_a_trip", items > TRIP_A and 0 < items % TRIP_A <= 8),
        ("a_border_inside_a_wave", per_frame % 64 != 0), ("a_border_inside_a_k_loop", per_frame % THREADS != 0),
        ("a_one_buffer", resident), ("a_one_buffer_over_a_trip", resident and per_frame > TRIP_A),
        ("b_border_inside_a_wave", two and ((h // 2) * (w // 16)) % 64 != 0), ("b_one_buffer", two and resident),
        ("f1_rounded_up", two and ((w // 2) * (h // 2) + PAD) % 16 != 0),
        ("c_nb_8", 8 in (nb0, nb1)), ("c_nb_28", nb0 == 28), ("c_nb_29", nb0 == 29), ("c_nb_255", nb0 == 255), ("c_nb_256", nb0 == 256),
        ("c_nb_256_nx_1", nb0 == 256 and g0[4] == 1),
        ("c_nx_1", g0[4] == 1), ("c_nx_1_level_1", two and g1[4] == 1),
        ("c_window_ends_on_the_last_byte", not c["px4"] and not sub and h % 8 == 0),
        ("c_window_ends_on_the_last_byte_of_level_1", two and not c["px4"] and not sub and (h // 2) % 8 == 0),
        ("d1_one_wave", sub and nb0 == 16), ("d1_one_trip", sub and nb0 == 64), ("d1_second_trip_partial_wave", sub and nb0 == 66),
        ("d1_nine_trips_of_c", sub and nb0 == 256), ("d1_under_a_predictor", two and sub and not c["px4"]),
        ("lds_limit_to_the_byte_one_level", not two and pl["lds"] + STATIC_LDS == LDS_LIMIT),
        ("lds_limit_to_the_byte_two_levels", two and pl["lds"] + STATIC_LDS == LDS_LIMIT),
        ("attr_not_set_at_48k", pl["lds"] == ATTR_ABOVE), ("attr_set", pl["attr"] == 1),
        ("attr_set_by_the_last_row", pl["attr"] == 1 and small_lds(w, h - 1, c["levels"]) <= ATTR_ABOVE),
        ("attr_set_per_call", pl["attr"] == 1 and resident), ("per_call_frames_copied", c["percall"] and not resident),
        ("stride_off_16_one_pair", c["stride_extra"] % 16 != 0 and c["n_pairs"] == 1),
        ("threshold_value", c["threshold"] == "value"), ("threshold_feature", c["threshold"] == "feature"),
        ("mean_subtract", bool(c["mean_subtract"])), ("two_levels", two),
        ("per_call", c["percall"]), ("per_call_half_pixel", c["percall"] and sub), ("per_call_integer", c["percall"] and not sub),
        ("per_call_integer_one_level", c["percall"] and not sub and not two),
        ("per_call_two_levels_border_inside_a_wave", c["percall"] and two and per_frame % 64 != 0),
    ) if hit}
    return got | group_reach(c)


def group_reach(c):
    got = set()
    if not c["group"] and not c["over_128"]:
        return got
    nb = blocks(grids(c)[0])
    ppw = THREADS // nb
    got |= {f"g_nb_{nb}"} if nb in (8, 9, 85, 86, 128, 129, 255, 256) else set()
    got |= {"g_" + name for name in group_counts(c)}
    if any(n % ppw for n in group_counts(c).values()):
        got.add("g_last_workgroup_short")
    if ppw > 1 and nb % 64:
        got.add("g_pairs_straddle_waves")
    if ppw * nb < THREADS:
        got.add("g_idle_lanes_behind_the_pairs")
    if c["over_128"]:
        got.add("g_over_128_pairs")
    if c["levels"] == 2 and c["group"]:
        got.add("g_two_levels")
    return got


VOCABULARY = [
    "small", "a_items_one_trip", "a_items_just_over_a_trip", "a_border_inside_a_wave", "a_border_inside_a_k_loop", "a_one_buffer",
    "a_one_buffer_over_a_trip", "b_border_inside_a_wave", "b_one_buffer", "f1_rounded_up", "c_nb_8", "c_nb_28", "c_nb_29", "c_nb_255",
    "c_nb_256", "c_nb_256_nx_1", "c_nx_1", "c_nx_1_level_1", "c_window_ends_on_the_last_byte", "c_window_ends_on_the_last_byte_of_level_1", "d1_one_wave",
    "d1_one_trip", "d1_second_trip_partial_wave", "d1_nine_trips_of_c", "d1_under_a_predictor", "lds_limit_to_the_byte_one_level", "lds_limit_to_the_byte_two_levels",
    "attr_not_set_at_48k", "attr_set", "attr_set_by_the_last_row", "attr_set_per_call", "per_call_frames_copied", "stride_off_16_one_pair", "threshold_value", "threshold_feature", "mean_subtract",
    "two_levels", "per_call", "per_call_half_pixel", "per_call_integer", "per_call_integer_one_level", "per_call_two_levels_border_inside_a_wave",
    "lds_one_row_over_one_level", "lds_one_step_over_two_levels",
    "fallback_plan_grid0", "fallback_plan_grid1"] + ["fallback_" + v for v in VERDICTS[1:] if v not in UNREACHABLE_VERDICTS] + [
    "g_nb_8", "g_nb_9", "g_nb_85", "g_nb_86", "g_nb_128", "g_nb_129", "g_nb_255", "g_nb_256", "g_ppw-1", "g_ppw", "g_ppw+1", "g_kppw+1",
    "g_last_workgroup_short", "g_pairs_straddle_waves", "g_idle_lanes_behind_the_pairs", "g_over_128_pairs", "g_two_levels"]

ALL_COUNTS = ("ppw-1", "ppw", "ppw+1", "kppw+1")


def _shape(nb, **kw):
    return dense_shape(nb, **kw)


def _two_level_shape(w, nb1, odd=False, subpixel=0):
    """The smallest w-wide frame whose dense level-1 grid has nb1 blocks (odd: in an odd number of level-1 rows)."""
    h1 = dense_height(w // 2, nb1, subpixel)
    assert h1 is not None, (w, nb1)
    if odd and h1 % 2 == 0:
        h1 += 1
        assert blocks(grid_for_level(w // 2, h1)) == nb1
    return w, 2 * h1


def _height_with(w, nb, pred):
    """The smallest height of a w-wide frame of nb dense blocks at which pred(h) holds."""
    h = dense_height(w, nb)
    while not pred(h):
        h += 1
    assert blocks(grid_for_level(w, h)) == nb
    return h


GPU_CASES = [
    # ---- pass C: the block counts, nx = 1, the window on the last byte
    case("nb-8-nx-1", *_shape(8, nx=1), "c_nb_8", "c_nx_1", "c_window_ends_on_the_last_byte", "g_nb_8", group=ALL_COUNTS, over_128=True),
    case("nb-9", *_shape(9, nx=1), "g_nb_9", "g_pairs_straddle_waves", "g_idle_lanes_behind_the_pairs", group=ALL_COUNTS),
    case("nb-28", *_shape(28), "c_nb_28", mean_subtract=0, group=("ppw+1",)),
    case("nb-29", *_shape(29), "c_nb_29", group=("ppw+1",)),
    case("nb-127-chunks-over-a-trip", 16, _height_with(16, 127, lambda h: 0 < (2 * h) % TRIP_A <= 8), "a_items_just_over_a_trip", "a_border_inside_a_wave",
         "a_border_inside_a_k_loop", "c_nx_1"),
    case("nb-256-nx-1", *_shape(256, nx=1), "c_nb_256_nx_1", "c_nx_1", "g_nb_256", group=("ppw", "kppw+1")),
    case("nb-257-nx-1", *_shape(257, nx=1), "fallback_plan_grid0", mean_subtract=1),
    case("nb-225-one-trip", *_shape(225, nx=15), "a_items_one_trip", "threshold_value", threshold="value"),
    case("nb-255", *_shape(255, nx=15), "c_nb_255", "g_nb_255", "c_window_ends_on_the_last_byte", "threshold_feature", group=("ppw", "kppw+1"),
         threshold="feature"),
    case("nb-256-half-pixel", *_shape(256, subpixel=1, nx=16), "c_nb_256", "d1_nine_trips_of_c", subpixel=1, group=("kppw+1",)),
    case("nb-85", *_shape(85), "g_nb_85", mean_subtract=0, group=ALL_COUNTS),
    case("nb-86", *_shape(86, subpixel=1), "g_nb_86", subpixel=1, group=ALL_COUNTS),
    case("nb-128", *_shape(128, subpixel=1), "g_nb_128", subpixel=1, group=ALL_COUNTS),
    case("nb-129", *_shape(129), "g_nb_129", mean_subtract=0, group=("ppw", "kppw+1")),
    # ---- D1
    case("d1-66", *_shape(66, subpixel=1, nx=6), "d1_second_trip_partial_wave", subpixel=1, percall=True),
    case("d1-64", *_shape(64, subpixel=1, nx=8), "d1_one_trip", subpixel=1, mean_subtract=1),
    case("d1-16", *_shape(16, subpixel=1, nx=4), "d1_one_wave", mean_subtract=0, subpixel=1, group=("ppw+1",)),
    # ---- two levels
    case("l1-1x8", *_two_level_shape(32, 8), "c_nx_1_level_1", "c_nb_8", "two_levels", "c_window_ends_on_the_last_byte_of_level_1", levels=2, mean_subtract=1, group=("ppw+1",)),
    case("l1-rounded-buffer", *_two_level_shape(48, 8, odd=True), "f1_rounded_up", "b_border_inside_a_wave", "per_call_two_levels_border_inside_a_wave",
         levels=2, mean_subtract=0, percall=True),
    case("l1-7-blocks", 32, _two_level_shape(32, 8)[1] - 2, "fallback_plan_grid1", levels=2),
    case("l1-half-pixel", *_two_level_shape(64, 18, subpixel=1), "d1_under_a_predictor", levels=2, subpixel=1),
    # ---- the LDS limit and the attribute
    case("lds-fit-one-level", 368, lds_edge_height(368, 1), "lds_limit_to_the_byte_one_level", "per_call_frames_copied", px4=True, n_pairs=2,
         percall=True),
    case("lds-over-one-level", 368, lds_edge_height(368, 1, over=True), "fallback_lds", "lds_one_row_over_one_level", px4=True, mean_subtract=1, n_pairs=2),
    case("lds-fit-two-levels", 64, lds_edge_height(64, 2), "lds_limit_to_the_byte_two_levels", "attr_set_per_call", "a_one_buffer_over_a_trip", "b_one_buffer",
         px4=True, levels=2, n_pairs=2, percall=True),
    case("lds-over-two-levels", 64, lds_edge_height(64, 2, over=True), "fallback_lds", "lds_one_step_over_two_levels", px4=True, levels=2, n_pairs=2),
    case("attr-48k-not-set", 80, attr_edge_height(80), "attr_not_set_at_48k", mean_subtract=0, px4=True),
    case("attr-set", 80, attr_edge_height(80, over=True), "attr_set_by_the_last_row", "per_call_half_pixel", px4=True, percall=True),
    case("per-call-integer", *_shape(35), "per_call_integer_one_level", mean_subtract=1, percall=True),
    # ---- placement
    case("stride-8-two-pairs", *_shape(35), "fallback_stride", mean_subtract=1, stride_extra=8, n_pairs=2),
    case("stride-8-one-pair", *_shape(35), "stride_off_16_one_pair", mean_subtract=1, stride_extra=8, n_pairs=1),
    case("prev-off-8", *_shape(35), "fallback_prev", mean_subtract=1, prev_off=8),
    case("cur-off-8", *_shape(35), "fallback_cur", mean_subtract=1, cur_off=8),
    case("width-8-mod-16", 72, dense_height(72, 40), "fallback_width", mean_subtract=1),
]

# plans and decodes alone
CPU_CASES = [
    case("workload-64x64-px4", 64, 64, px4=True, percall=True),
    case("workload-128x128-px4-two-levels", 128, 128, px4=True, levels=2, percall=True),
    case("workload-96x80", 96, 80, levels=2),
    case("workload-256x224-px4", 256, 224, px4=True),
    case("workload-320x240-px4", 320, 240, px4=True),
    case("nb-10", *_shape(10, nx=1), group=ALL_COUNTS),
    case("nb-64", *_shape(64), group=ALL_COUNTS),
    case("nb-65", *_shape(65), group=ALL_COUNTS),
]

# the plans alone, against the C++ functions: SmallArgs and SearchArgs field by field
PLAN_ONLY = [
    dict(id="4096x4096", w=4096, h=4096, nx=10, ny=10),
    dict(id="16x1048576", w=16, h=1 << 20, nx=1, ny=8),
    dict(id="16777216x1", w=1 << 24, h=1, nx=1, ny=8),
    dict(id="one-row", w=16, h=1, nx=1, ny=1),
    dict(id="levels-0", w=64, h=64, levels=0),
    dict(id="levels-3", w=64, h=64, levels=3),
    dict(id="tile-16", w=64, h=64, tile=16),
    dict(id="search-8", w=64, h=64, search=8),
    dict(id="no-pairs", w=64, h=64, n_pairs=0),
    dict(id="pairs-limit", w=64, h=64, n_pairs=0x7FFFFFFF // 256),
    dict(id="pairs-over", w=64, h=64, n_pairs=0x7FFFFFFF // 256 + 1),
    dict(id="grid0-none", w=64, h=64, nx=0, ny=5),
    dict(id="grid0-257", w=64, h=64, nx=257, ny=1),
    dict(id="bins0-15", w=64, h=64, rng0=15),
    dict(id="bins0-16", w=64, h=64, rng0=16),
    dict(id="width-24", w=24, h=64),
    dict(id="stride-one-pair", w=64, h=64, n_pairs=1, pair_stride=4100),
    dict(id="stride-two-pairs", w=64, h=64, n_pairs=2, pair_stride=4100),
    dict(id="prev-4", w=64, h=64, prev=BASE + 4),
    dict(id="cur-12", w=64, h=64, cur=BASE + 12),
    dict(id="no-subdirs0", w=64, h=64, subpixel=1, subdirs0=0),
    dict(id="odd-height-two-levels", w=64, h=63, levels=2),
    dict(id="l1-size-off", w=64, h=64, levels=2, l1_w=30),
    dict(id="grid1-none", w=64, h=64, levels=2, nx1=0, ny1=0),
    dict(id="grid1-257", w=64, h=64, levels=2, nx1=257, ny1=1),
    dict(id="bins1-16", w=64, h=64, levels=2, rng1=16),
    dict(id="no-subdirs1", w=64, h=64, levels=2, subpixel=1, subdirs1=0),
    dict(id="lds-over-by-16", w=16, h=4992),
    dict(id="group-stride-negative", w=64, h=64, pair_stride=-4096, n_pairs=5),
    dict(id="group-stride-2^32", w=64, h=64, pair_stride=1 << 32, n_pairs=5),
    dict(id="group-2^31-pairs", w=64, h=64, n_pairs=1 << 31),
    dict(id="group-frame-over-2^24", w=4112, h=4096, nx=10, ny=10),
]


def plan_args(c):
    """A case of any list as the arguments of both plans."""
    if "tags" in c:
        g0, g1 = grids(c)
        stride, prev, cur = frame_layout(c)
        return dict(w=c["w"], h=c["h"], levels=c["levels"], g0=g0 or (0,) * 6, g1=g1 or (0,) * 6, n_pairs=c["n_pairs"], pair_stride=stride,
                    prev=prev, cur=cur, subpixel=c["subpixel"], tile=8, search=4, rng0=level_range(c["levels"], 0),
                    rng1=level_range(c["levels"], 1), subdirs0=1, subdirs1=1, l1_w=c["w"] // 2, l1_h=c["h"] // 2)
    levels = c.get("levels", 1)
    return dict(w=c["w"], h=c["h"], levels=levels, g0=(4, 4, 8, 8, c.get("nx", 5), c.get("ny", 5)), g1=(4, 4, 8, 8, c.get("nx1", 2), c.get("ny1", 4)),
                n_pairs=c.get("n_pairs", 3), pair_stride=c.get("pair_stride", c["w"] * c["h"]), prev=c.get("prev", BASE), cur=c.get("cur", BASE + (1 << 40)),
                subpixel=c.get("subpixel", 0), tile=c.get("tile", 8), search=c.get("search", 4), rng0=c.get("rng0", 13 if levels == 2 else 4),
                rng1=c.get("rng1", 4), subdirs0=c.get("subdirs0", 1), subdirs1=c.get("subdirs1", 1), l1_w=c.get("l1_w", c["w"] // 2),
                l1_h=c.get("l1_h", c["h"] // 2))


def plans_of(c):
    a = plan_args(c)
    none = lambda g: g if blocks(g) else None
    small = small_plan(a["w"], a["h"], a["levels"], none(a["g0"]), none(a["g1"]), a["n_pairs"], a["pair_stride"], a["prev"], a["cur"], a["subpixel"],
                       a["tile"], a["search"], a["rng0"], a["rng1"], a["subdirs0"], a["subdirs1"], a["l1_w"], a["l1_h"])
    group = group_plan(a["w"], a["h"], none(a["g0"]), a["n_pairs"], a["pair_stride"], a["rng0"], a["tile"], a["search"])
    return small, group


def selftest_families():
    """small_plan_make == small_plan() and lane8_group_plan == group_plan(), on every case of every list: one listing, two
    lines a case.  The case as tests/native/host_selftest.cpp reads it: w h levels g0[6] g1[6] n_pairs pair_stride prev cur
    subpixel tile search rng0 rng1 subdirs0 subdirs1 l1_w l1_h"""
    def line(c):
        a = plan_args(c)
        return rig.joined([a["w"], a["h"], a["levels"], *a["g0"], *a["g1"], a["n_pairs"], a["pair_stride"], a["prev"], a["cur"], a["subpixel"], a["tile"],
                           a["search"], a["rng0"], a["rng1"], a["subdirs0"], a["subdirs1"], a["l1_w"], a["l1_h"]])

    cases = CPU_CASES + GPU_CASES + PLAN_ONLY
    return [rig.family("small-plan", "small plan: ", cases, line, lambda c: _plan_fields(plans_of(c)[0]), PLAN_FIELDS),
            rig.family("small-plan", "group plan: ", cases, line, lambda c: [plans_of(c)[1][k] for k in GROUP_FIELDS], GROUP_FIELDS, name="group-plan",
                       summary="small plan: {} cases")]


# ---- the frames of a device case -----------------------------------------------------------------------------------------

REACH = 16
# What the distinct pairs of a case hold, in launch order.  Neighbours (cyclically) differ in flow and in vote count:
# the kinds marked `row` have the first block row of prev flattened (gated), `flat` votes nowhere, `unrelated` is rejected
# by the value threshold.  (kind, shift one level, shift two levels, noise, row)
KINDS = (("corner", (4, 4), (8, -8), 0, False), ("flat", None, None, 0, False), ("corner", (-4, -4), (-6, 4), 2, True),
         ("identical", None, None, 0, False), ("corner", (4, -4), (12, 10), 0, True), ("unrelated", None, None, 0, False),
         ("period-x", None, None, 0, False), ("period-y", None, (-16, 16), 3, True))
BRIGHT = {0: 120, 4: -120}     # with mean_subtract: the brightness steps of pairs 0 and 4


def rounded_mean(img):
    return (int(img.sum(dtype=np.uint64)) + img.size // 2) // img.size


def gate(img, x, y):
    """The feature gate of the 8 x 8 tile at (x, y): the 12 + 12 absolute differences between vertical and horizontal
    neighbours inside its centre 4 x 4."""
    c = img[y + 2:y + 6, x + 2:x + 6].astype(np.int64)
    return int(np.abs(c[1:] - c[:-1]).sum() + np.abs(c[:, 1:] - c[:, :-1]).sum())


def hard_pairs(c, synth):
    """The case's eight distinct pairs: prevs, curs (uint8 [8, h, w]) and their kinds."""
    w, h, two = c["w"], c["h"], c["levels"] == 2
    g0 = grids(c)[0]
    prevs, curs, kinds = np.empty((8, h, w), np.uint8), np.empty((8, h, w), np.uint8), []
    seed = 9100 + 13 * w + h
    for j, (name, s1, s2, noise, row) in enumerate(KINDS):
        shift = s2 if two else s1
        bright = BRIGHT.get(j, 0) if c["mean_subtract"] else 0
        if name == "period-y" and two:
            name = "far"         # (two levels: beyond the reach of both levels together on both axes)
        if name in ("corner", "far"):
            a, b, _ = synth.make_pair(w, h, REACH, seed + j, shift=shift, noise=noise, brightness=bright)
            a, b = a.copy(), b.copy()
            if bright:           # hot and dead pixels: the equalised frame saturates at the end its brightness step leaves room at
                b.reshape(-1)[5::37] = 0 if bright > 0 else 255
        elif name == "flat":
            a, b = np.full((h, w), 90, np.uint8), np.full((h, w), 90, np.uint8)
        elif name == "identical":
            a = synth.make_pair(w, h, REACH, seed + j, shift=(0, 0))[0].copy()
            b = a.copy()
        elif name == "unrelated":
            a = synth.make_pair(w, h, REACH, seed + j, shift=(0, 0))[0].copy()
            b = np.random.default_rng(seed + j).integers(0, 256, size=(h, w), dtype=np.uint8)
        else:                    # period 2 along one axis, random along the other: every even shift along the axis ties at 0
            rng = np.random.default_rng(seed + j)
            if name == "period-x":
                a = np.where(np.arange(w)[None, :] % 2 == 0, rng.integers(0, 256, size=(h, 1)), rng.integers(0, 256, size=(h, 1)))
            else:
                a = np.where(np.arange(h)[:, None] % 2 == 0, rng.integers(0, 256, size=(1, w)), rng.integers(0, 256, size=(1, w)))
            a = a.astype(np.uint8)
            b = a.copy()
        if row:
            a[: g0[1] + 8] = 90          # down to the last row of the first block row's tiles
            if name == "period-y":       # (in both frames: their means stay equal, and with them a SAD of 0 under mean_subtract)
                b[: g0[1] + 8] = 90
        prevs[j], curs[j] = a, b
        kinds.append(name)
    return prevs, curs, kinds


def pick_value_threshold(sads):
    """A threshold t from the records: some block has sad == t (rejected) and another t - 1 (the last accepted).  The most
    frequent such pair."""
    vals, counts = np.unique(sads[(sads != 0xFFFF) & (sads > 1)], return_counts=True)
    have = dict(zip(vals.tolist(), counts.tolist()))
    best = max((t for t in have if t - 1 in have), key=lambda t: min(have[t], have[t - 1]), default=None)
    assert best is not None, "no two blocks one SAD apart"
    return int(best)


def pick_feature_threshold(c, prevs, kinds):
    """A threshold from the frames: the gate value of a textured block, with textured blocks below it."""
    x0, y0, sx, sy, nx, ny = grids(c)[0]
    j = kinds.index("identical")
    gates = sorted(gate(prevs[j], x0 + bx * sx, y0 + by * sy) for by in range(ny) for bx in range(nx))
    t = gates[len(gates) // 2]
    assert gates[0] < t and gates[0] > 0
    return int(t)


def case_params(c, aof, orc, synth, frames=None):
    """The product's parameters of a case.  A threshold case takes its threshold from the oracle's records (value) or from
    the frames (feature)."""
    make = aof.px4flow_params if c["px4"] else aof.default_params
    kw = params_kw(c)
    if not c["px4"] and c["subpixel"]:
        kw["subpixel"] = 1
    p = make(c["w"], c["h"], **kw)
    if c["threshold"]:
        prevs, curs, kinds = frames or hard_pairs(c, synth)
        if c["threshold"] == "value":
            po = orc.params_from(p)
            sads = np.concatenate([orc.flow_pair(po, a, b)["blocks"]["sad"] for a, b in zip(prevs, curs)])
            p.value_threshold = pick_value_threshold(sads)
        else:
            p.feature_threshold = pick_feature_threshold(c, prevs, kinds)
    return p


def check_inputs(c, p, prevs, curs, kinds, outs):
    """Before the device runs: each input does what it is there for.  outs: the oracle's flow_pair (with level 1) of every
    distinct pair under parameters p."""
    two, nb0 = c["levels"] == 2, blocks(grids(c)[0])
    x0, y0, sx, sy, nx, ny = grids(c)[0]
    rec = {k: outs[kinds.index(k)] for k in set(kinds)}
    sad = lambda o: o["blocks"]["sad"]
    assert (sad(rec["flat"]) == 0xFFFF).all(), "a flat pair: every block gated"
    assert (sad(rec["identical"]) == 0).all() or two or c["threshold"] == "feature", "an identical pair: SAD 0 everywhere"
    assert (sad(rec["identical"]) == 0).any()
    if c["subpixel"]:
        assert (rec["identical"]["subdirs"][sad(rec["identical"]) == 0] == 8).all(), "nothing lies below a SAD of zero"
    un = sad(rec["unrelated"])
    assert (un[un != 0xFFFF] >= p.value_threshold).any(), "an unrelated pair: the value threshold rejects"
    if not two:
        for name, want in (("period-x", (-4, 0)), ("period-y", (0, -4))):
            b = rec[name]["blocks"]
            live = b["sad"] != 0xFFFF
            if name == "period-y":       # (the second block row's windows reach into the flattened band)
                assert ny >= 3 and live[nx:].all()
                live[: 2 * nx] = False
            assert live.any() and (b["sad"][live] == 0).all(), name
            assert (b["dx"][live] == want[0]).all() and (b["dy"][live] == want[1]).all(), (name, "ties go to the first candidate in scan order")
        for j, (name, s1, _, noise, row) in enumerate(KINDS):
            if name == "corner" and not (c["mean_subtract"] and j in BRIGHT):
                b = outs[j]["blocks"]
                live = b["sad"] != 0xFFFF
                assert live.any() and (b["dx"][live] == s1[0]).all() and (b["dy"][live] == s1[1]).all(), (j, "a corner of the reach")
                assert row == (not live[:nx].any()), (j, "the flattened block row is gated")
    else:
        far = outs[kinds.index("far")]
        skipped = [int((sad(o) == 0xFFFF).sum()) for o in outs]
        assert 0 < skipped[0] < nb0, "a predictor pushes edge windows out of the frame: some blocks are skipped, not all"
        assert int(far["flow"]["count"]) < nb0
    if c["mean_subtract"]:
        for j, step in BRIGHT.items():
            delta = rounded_mean(prevs[j]) - rounded_mean(curs[j])
            moved = curs[j].astype(np.int64) + delta
            assert abs(delta) > 60 and ((moved < 0).any() if step > 0 else (moved > 255).any()), (j, delta, "the equalised frame saturates")
    if c["threshold"] == "value":
        every = np.concatenate([sad(o) for o in outs])
        assert (every == p.value_threshold).any() and (every == p.value_threshold - 1).any()
    if c["threshold"] == "feature":
        j = kinds.index("identical")
        gates = np.array([gate(prevs[j], x0 + bx * sx, y0 + by * sy) for by in range(ny) for bx in range(nx)])
        at, below = gates == p.feature_threshold, gates < p.feature_threshold
        assert at.any() and below.any() and (sad(outs[j])[at] != 0xFFFF).all() and (sad(outs[j])[below] == 0xFFFF).all()
    # the pairs that share a workgroup of the grouped search: neighbours differ in vote count and in flow
    for j in range(min(max(list(group_counts(c).values()) + [129 if c["over_128"] else 0]), 9) - 1):
        a, b = outs[j % 8]["flow"], outs[(j + 1) % 8]["flow"]
        assert int(a["count"]) != int(b["count"]), (j, "neighbours with the same vote count")
        assert (a["flow_x"], a["flow_y"]) != (b["flow_x"], b["flow_y"]) or 0 in (int(a["count"]), int(b["count"])), (j, "neighbours with the same flow")
