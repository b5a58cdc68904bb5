"""The launch plan of the flat lane-per-block 8x8 kernels in plain Python -- k_search_lane8 (K3 behind it), k_flow_lane8_flat
(the reduction in the launch) and the chunk walk k_search_lane8_pruned (csrc/aof_lane8_plan.hpp: lane8_flat_plan) --, what
search_chunks (csrc/aof_lane8_kernels.hpp) makes of it lane by lane, the workgroup placement xcd_remap
(csrc/aof_xcd_remap.hpp), the names of the paths a launch can take through all of it, and the case lists of
tests/test_lane8_plan_ref.py, tests/test_host_asan.py (the same plan from the C++ function) and
tests/test_gpu_lane8_plan.py (every case of GPU_CASES on the device, against the oracle).

Written from DESIGN.md ("Kernels": K2) and the launcher's comments:

  slices    a launch indexes its (pair, block) items with 31 bits: per = min(0x7FFF0000 / nb, 2^24 - 1) pairs per slice, every
            array advanced by the pairs in front of the slice.
  flat      k_search_lane8 / k_flow_lane8_flat: 64 lanes per workgroup below 1 572 864 items, 256 from there on; workgroup
            xcd_remap(blockIdx) owns items [wg * threads, (wg + 1) * threads).  The fused form appends
            ceil(pairs / (threads / 64)) finaliser workgroups, one wave per pair; a searching wave votes for the pair of its
            first item (`lead`) and, where it reaches past (lead + 1) * nb, for lead + 1.
  walk      k_search_lane8_pruned: chunks of 256 items, spw = clamp(chunks / 1536, 1, 8) consecutive chunks per workgroup,
            one workgroup in `stride` reports.

No device case's shape is typed in here: a case names nb, the grid kind and the pair count, and the frame is the smallest
the grid rule (small_plan_ref.grid_for_level) gives it."""
import hashlib

import numpy as np

import selftest_rig as rig
from small_plan_ref import blocks, grid_for_level, lane8_supported, rounded_mean

# csrc/aof_lane8_plan.hpp, csrc/aof_engine_args.hpp, csrc/aof_ctx.hpp
THREADS, SMALL_THREADS, MAX_ITEMS, LARGE_ITEMS = 256, 64, 0x7FFF0000, 6 * 256 * 1024
WALK_WGS, WALK_MAX, PRUNE_SLOTS, PRUNE_MIN_CHUNKS = 1536, 8, 256, 2048
VOTE_PAIRS, VOTE_STRIDE = 2048, 128
KINDS = ("exhaustive", "fused", "walk")
VOTES = ("ok", "pruned", "memory", "fault", "bins", "stride", "grid", "capacity")   # enum Lane8Votes, in the order tested


def xcd_remap(b, total):
    """Logical workgroup of hardware workgroup b (numbers or arrays): XCD b % 8 owns one contiguous run of logical ids."""
    q, r, xcd, slot = total // 8, total % 8, b % 8, b // 8
    return np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + slot


def flat_plan(nb, n_pairs, pair_stride, w, h, prune=0, fused=False, rng=4, votes=(1, 1, VOTE_STRIDE), capacity=VOTE_PAIRS, slice=0,
              tile=8, search=4):
    """lane8_flat_plan.  votes: (the context has vote memory, it has a fault word, words per record) or None."""
    n = 2 * (2 * rng + 1) + 1
    mem, fault, stride = votes if votes else (0, 0, 0)
    tests = [("pruned", bool(prune)), ("memory", not mem), ("fault", not fault), ("bins", n > 62), ("stride", stride < 2 + 2 * n),
             ("grid", nb <= 64)]
    verdict = next((name for name, fails in tests if fails), None)
    if verdict is None:
        verdict = "ok" if min(n_pairs, MAX_ITEMS // nb) <= capacity else "capacity"
    pl = dict(supported=int(lane8_supported(w, h, nb, n_pairs, pair_stride, tile, search)), votes=verdict, prune_large=0, chunks_all=0, per=0,
              slices=0, done=0, pairs=0, frame_off=0, block_off=0, pred_off=0, sums_off=0, items=0, kind="exhaustive", threads=0, wgs=0,
              finalisers=0, grid=0, last_live=0, chunks=0, spw=0, last_chunks=0, stride=1, expected=0, nb=nb)
    if nb < 1 or n_pairs < 1:
        return pl
    chunks_all = -(-n_pairs * nb // THREADS)
    per = min(MAX_ITEMS // nb, (1 << 24) - 1)
    pl.update(chunks_all=chunks_all, prune_large=int(chunks_all >= PRUNE_MIN_CHUNKS), per=per, slices=-(-n_pairs // per))
    if not 0 <= slice < pl["slices"]:
        return pl
    done = slice * per
    pairs = min(per, n_pairs - done)
    items = pairs * nb
    kind = "fused" if fused else "walk" if prune else "exhaustive"
    pl.update(done=done, pairs=pairs, frame_off=done * pair_stride, block_off=done * nb, pred_off=done, sums_off=4 * done, items=items, kind=kind)
    if kind == "walk":
        chunks = -(-items // THREADS)
        spw = max(1, min(WALK_MAX, chunks // WALK_WGS))
        wgs = -(-chunks // spw)
        pl.update(threads=THREADS, chunks=chunks, spw=spw, wgs=wgs, grid=wgs, last_chunks=chunks - (wgs - 1) * spw,
                  last_live=items - (chunks - 1) * THREADS)
        if slice == 0:
            stride = -(-wgs // PRUNE_SLOTS)
            pl.update(stride=stride, expected=-(-wgs // stride))
        return pl
    threads = SMALL_THREADS if items < LARGE_ITEMS else THREADS
    wgs = -(-items // threads)
    fin = -(-pairs // (threads // 64)) if fused else 0
    pl.update(threads=threads, wgs=wgs, finalisers=fin, grid=wgs + fin, last_live=items - (wgs - 1) * threads)
    return pl


PLAN_FIELDS = ("supported", "votes", "prune_large", "chunks_all", "per", "slices", "done", "pairs", "frame_off", "block_off", "pred_off",
               "sums_off", "items", "kind", "threads", "wgs", "finalisers", "grid", "last_live", "chunks", "spw", "last_chunks", "stride",
               "expected")


def _plan_fields(pl):
    """The plan as the flat list of numbers the host self-test prints (PLAN_FIELDS)."""
    return [VOTES.index(pl[k]) if k == "votes" else KINDS.index(pl[k]) if k == "kind" else pl[k] for k in PLAN_FIELDS]


# ---- the decodes -----------------------------------------------------------------------------------------------------------

def owners(pl):
    """search_chunks: every (hardware workgroup, chunk, lane) of the slice's searching workgroups -> item, as arrays
    block [wgs * spw * threads], chunk, lane, item0, item, live.  A walk's workgroup leaves at the first chunk whose item0 is
    at or beyond `items` (ran == False from there on); an exhaustive lane beyond `items` returns."""
    wgs, threads, spw = pl["wgs"], pl["threads"], max(pl["spw"], 1)
    b, c, lane = np.meshgrid(np.arange(wgs, dtype=np.int64), np.arange(spw, dtype=np.int64), np.arange(threads, dtype=np.int64), indexing="ij")
    b, c, lane = b.ravel(), c.ravel(), lane.ravel()
    wg = xcd_remap(b, wgs)
    item0 = (wg * spw + c) * threads
    item = item0 + lane
    ran = item0 < pl["items"] if pl["kind"] == "walk" else np.ones_like(item, dtype=bool)
    live = ran & (item < pl["items"])
    return dict(block=b, wg=wg, chunk=c, lane=lane, item0=item0, item=item, ran=ran, live=live, pair=np.where(live, item // pl["nb"], -1),
                blk=np.where(live, item % pl["nb"], -1))


def waves(pl):
    """The fused form, wave by wave (rows) and lane by lane (columns): first_item, lead, next_pair_at, straddles (the scalar
    test first_item + 63 >= next_pair_at), and per lane the pair it votes for (-1: none)."""
    assert pl["kind"] == "fused" and pl["nb"] > 64
    o = owners(pl)
    item, live = o["item"].reshape(-1, 64), o["live"].reshape(-1, 64)
    first_item = item[:, 0]
    lead = first_item // pl["nb"]
    next_at = (lead + 1) * pl["nb"]
    straddles = first_item + 63 >= next_at
    votes_lead = live & (item < next_at[:, None])
    votes_next = live & (item >= next_at[:, None]) & straddles[:, None]
    votes_for = np.where(votes_lead, lead[:, None], np.where(votes_next, lead[:, None] + 1, -1))
    return dict(first_item=first_item, lead=lead, next_pair_at=next_at, straddles=straddles, votes_for=votes_for, item=item, live=live,
                wave_live=first_item < pl["items"])


def finalisers(pl):
    """(hardware workgroup - wgs, wave) -> pair, -1 where the wave has none."""
    per = pl["threads"] // 64
    f, wave = np.meshgrid(np.arange(pl["finalisers"], dtype=np.int64), np.arange(per, dtype=np.int64), indexing="ij")
    pair = f * per + wave
    return np.where(pair < pl["pairs"], pair, -1)


# ---- cases -----------------------------------------------------------------------------------------------------------------

def dense_frame(nb, subpixel=0, wpad=0, levels=1):
    """The fewest bytes of a frame whose dense grid has nb blocks (two levels: and whose level 1 has a grid): (w, h)."""
    m, best = 2 * (4 + subpixel), None
    for nx in range(1, nb + 1):
        if nb % nx == 0:
            w, h = 8 * nx + m + wpad, 8 * (nb // nx) + m
            if levels == 2 and grid_for_level(w, h, 1, False, subpixel) is None:
                continue
            if best is None or w * h < best[0] * best[1]:
                best = (w, h)
    assert best is not None, (nb, "no dense grid of so many blocks has a level 1")
    assert blocks(grid_for_level(*best, 0, False, subpixel)) == nb
    return best


def chunk_walks(g):
    """A grid of more than 256 blocks that does not take the column walk (lane8_cols_supported)."""
    return blocks(g) > 256 and not (g[3] == 8 and g[4] >= 16 and g[5] >= 2)


def px4_frame(nb, levels=1):
    """The smallest square frame (even at two levels) and num_blocks whose PX4Flow grid has nb blocks and is walked in chunks:
    (w, h, num_blocks)."""
    for w in range(24, 400, levels):
        for k in range(17, 64):
            g = grid_for_level(w, w, 0, True, 0, num_blocks=k)
            if blocks(g) == nb and chunk_walks(g) and (levels == 1 or blocks(grid_for_level(w, w, 1, True, 0, num_blocks=k)) >= 8):
                return w, w, k
    raise AssertionError(nb)


def case(id, nb, n_pairs, *paths, grid="dense", mode="exhaustive", fused=False, levels=1, subpixel=0, mean_subtract=1, layout=False):
    """mode: 'exhaustive', 'pruned', 'adaptive-1' / 'adaptive1' (the default mode with belief -1 -- the first chunk of every
    wave judges -- or 1).  fused: the caller asks for the reduction in the launch.  layout: a width off 4, frames at an odd
    address, an odd pair stride beyond the frame, the last frame on the last byte in front of a guard."""
    assert mode in ("exhaustive", "pruned", "adaptive-1", "adaptive1") and grid in ("dense", "px4")
    assert nb > THREADS, "grids of up to 256 blocks go to the grouped search (lane8_group_plan), not to the flat launches"
    if grid == "dense":
        w, h = dense_frame(nb, subpixel, 1 if layout else 0, levels)
        k = 0
    else:
        w, h, k = px4_frame(nb, levels)
    c = dict(id=id, nb=nb, n_pairs=n_pairs, paths=paths, grid=grid, mode=mode, fused=fused, levels=levels, subpixel=subpixel,
             mean_subtract=mean_subtract, layout=layout, w=w, h=h, num_blocks=k)
    assert blocks(case_grid(c)) == nb
    return c


def case_grid(c, level=0):
    return grid_for_level(c["w"], c["h"], level, c["grid"] == "px4", c["subpixel"], num_blocks=c["num_blocks"] or 5)


def params_kw(c):
    kw = dict(pyramid_levels=c["levels"], mean_subtract=c["mean_subtract"], subpixel=c["subpixel"])
    if c["grid"] == "px4":
        kw.update(grid_mode=1, num_blocks=c["num_blocks"])
    return kw


def pair_stride(c):
    return c["w"] * c["h"] + (c["w"] * c["h"] % 2 + 5 if c["layout"] else 0)    # (layout: beyond the frame, and odd)


def hist_range(c):
    return 13 if c["levels"] == 2 else 4


def prune_of(c):
    """SearchArgs.prune of the level-0 launch as choose_lane8 resolves it: 0, 1 or 2 (batch_plan_ref owns the rule)."""
    import batch_plan_ref as bp
    return bp.lane8_prune(bp.of_lane8(c), 1 if c["mode"] == "adaptive1" else -1)


def case_plan(c, slice=0):
    prune = prune_of(c)
    probe = flat_plan(c["nb"], c["n_pairs"], pair_stride(c), c["w"], c["h"], prune, False, hist_range(c))
    fused = c["fused"] and probe["votes"] == "ok"
    assert not (prune and not chunk_walks(case_grid(c))), (c["id"], "a dense grid prunes as a column walk: not this family")
    return flat_plan(c["nb"], c["n_pairs"], pair_stride(c), c["w"], c["h"], prune, fused, hist_range(c), slice=slice)


def instantiation(c):
    pl = case_plan(c)
    sub, eq = "tf"[1 - c["subpixel"]], "tf"[1 - c["mean_subtract"]]
    return {"exhaustive": f"k_search_lane8<{sub},{eq}>", "fused": f"k_flow_lane8_flat<{sub},{eq}>", "walk": f"k_search_lane8_pruned<{sub}>"}[pl["kind"]]


def reach(c):
    """The names of the paths the case takes (VOCABULARY)."""
    pl = case_plan(c)
    nb, n, kind = c["nb"], c["n_pairs"], pl["kind"]
    got = {instantiation(c), "threads_" + str(pl["threads"]) + "_" + kind}
    add = lambda name, hit: got.add(name) if hit else None
    add("one_pair_span_is_the_frame+" + kind, n == 1)
    add("two_levels_" + kind, c["levels"] == 2)
    add("layout_odd_everything", c["layout"])
    if kind != "walk":
        add("items_one_below_the_threads_switch", LARGE_ITEMS - nb <= pl["items"] < LARGE_ITEMS)
        add("items_on_the_threads_switch", pl["items"] == LARGE_ITEMS)
        add("last_workgroup_one_live_lane", pl["last_live"] == 1)
        add("last_workgroup_and_last_wave_partly_live_256", pl["threads"] == 256 and pl["last_live"] % 64 != 0)
        if n > 1:
            at = {(k * nb) % 64 for k in range(1, n)}
            add("every_straddle_position", nb > 64 and at == set(range(64)))
            add("every_straddle_position+" + instantiation(c), nb > 64 and at == set(range(64)))
            add("border_on_the_last_lane", 63 in at and nb % 64 != 0)
            add("borders_on_wave_edges_only", at == {0})
    if kind == "fused":
        wv = waves(pl)
        add("wave_ends_exactly_on_a_border", bool(((wv["first_item"] + 64 == wv["next_pair_at"]) & wv["wave_live"]).any()) and nb % 64 != 0)
        add("finaliser_workgroup_per_pair", pl["threads"] == 64)
        add("finalisers_last_workgroup_one_wave", pl["threads"] == 256 and n % 4 == 1)
        add("finalisers_last_workgroup_three_waves", pl["threads"] == 256 and n % 4 == 3)
        add("pairs_at_the_vote_capacity", n == VOTE_PAIRS)
    add("one_over_the_vote_capacity_takes_k3", c["fused"] and pl["votes"] == "capacity" and n == VOTE_PAIRS + 1)
    if kind == "walk":
        got.add("walk_" + c["mode"])
        add("walk_two_chunks_second_partly_live", pl["chunks"] == 2 and pl["last_live"] < THREADS)
        add("walk_spw_1_at_3071_chunks", pl["chunks"] == 2 * WALK_WGS - 1)
        add("walk_spw_2_at_3072_chunks", pl["chunks"] == 2 * WALK_WGS and pl["wgs"] == WALK_WGS)
        add("walk_spw_2_last_workgroup_one_chunk", pl["chunks"] == 2 * WALK_WGS + 1 and pl["last_chunks"] == 1)
        add("walk_3073_chunks+" + c["mode"], pl["chunks"] == 2 * WALK_WGS + 1 and c["levels"] == 1 and not c["subpixel"])
        add("walk_spw_clamped_at_8_short_last_workgroup", pl["chunks"] >= 9 * WALK_WGS and pl["spw"] == 8 and pl["last_chunks"] < 8)
        add("walk_last_chunk_partly_live", pl["last_live"] < THREADS)
        add("walk_carried_row_crosses_a_pair_border", pl["spw"] > 1 and nb % THREADS != 0)
        add("walk_report_stride_over_1", pl["stride"] > 1)
        add("walk_half_pixel", bool(c["subpixel"]))
    return got


UNREACHABLE = {"second_slice": "two slices need more than 2^31 items in one call -- more frames than the device has memory; the slice "
                               "arithmetic is held on the host (CASES, tests/test_host_asan.py)"}

VOCABULARY = (
    [f"k_search_lane8<{s},{e}>" for s in "tf" for e in "tf"] + [f"k_flow_lane8_flat<{s},{e}>" for s in "tf" for e in "tf"]
    + ["k_search_lane8_pruned<t>", "k_search_lane8_pruned<f>"]
    + ["threads_64_exhaustive", "threads_256_exhaustive", "threads_64_fused", "threads_256_fused", "threads_256_walk",
       "one_pair_span_is_the_frame+exhaustive", "one_pair_span_is_the_frame+walk", "walk_3073_chunks+pruned",
       "every_straddle_position+k_search_lane8<f,f>", "every_straddle_position+k_search_lane8<f,t>", "every_straddle_position+k_search_lane8<t,t>",
       "every_straddle_position+k_flow_lane8_flat<f,f>", "every_straddle_position+k_flow_lane8_flat<f,t>",
       "every_straddle_position+k_flow_lane8_flat<t,t>", "two_levels_exhaustive", "two_levels_walk", "layout_odd_everything",
       "items_one_below_the_threads_switch", "items_on_the_threads_switch", "last_workgroup_one_live_lane",
       "last_workgroup_and_last_wave_partly_live_256", "every_straddle_position", "border_on_the_last_lane", "borders_on_wave_edges_only",
       "wave_ends_exactly_on_a_border", "finaliser_workgroup_per_pair", "finalisers_last_workgroup_one_wave",
       "finalisers_last_workgroup_three_waves", "pairs_at_the_vote_capacity", "one_over_the_vote_capacity_takes_k3",
       "walk_pruned", "walk_adaptive-1", "walk_adaptive1", "walk_two_chunks_second_partly_live", "walk_spw_1_at_3071_chunks",
       "walk_spw_2_at_3072_chunks", "walk_spw_2_last_workgroup_one_chunk", "walk_spw_clamped_at_8_short_last_workgroup",
       "walk_last_chunk_partly_live", "walk_carried_row_crosses_a_pair_border", "walk_report_stride_over_1", "walk_half_pixel"]
    + list(UNREACHABLE))

GPU_CASES = [
    # ---- flat search, K3 behind it
    case("257-one-pair", 257, 1, "one_pair_span_is_the_frame+exhaustive", "last_workgroup_one_live_lane", "threads_64_exhaustive", "k_search_lane8<f,t>"),
    case("257-65-pairs", 257, 65, "every_straddle_position+k_search_lane8<f,f>", "border_on_the_last_lane", "k_search_lane8<f,f>", mean_subtract=0),
    # (257 is prime: its dense grids are one block wide, and level 1 of such a frame has no grid.  321 = 3 x 107 is 1 mod 64 too)
    case("321-65-pairs-two-levels", 321, 65, "every_straddle_position", "two_levels_exhaustive", "k_search_lane8<f,t>", levels=2),
    case("257-65-pairs-half-pixel", 257, 65, "every_straddle_position", "k_search_lane8<t,t>", subpixel=1),
    case("320-9-pairs-half-pixel-no-sums", 320, 9, "borders_on_wave_edges_only", "k_search_lane8<t,f>", subpixel=1, mean_subtract=0),
    case("384-4095-pairs", 384, 4095, "items_one_below_the_threads_switch", "threads_64_exhaustive"),
    case("384-4096-pairs", 384, 4096, "items_on_the_threads_switch", "threads_256_exhaustive"),
    case("385-4086-pairs", 385, 4086, "last_workgroup_and_last_wave_partly_live_256", "threads_256_exhaustive"),
    case("272-9-pairs-layout", 272, 9, "layout_odd_everything", layout=True),
    # ---- the reduction in the launch
    case("257-65-pairs-fused", 257, 65, "finaliser_workgroup_per_pair", "wave_ends_exactly_on_a_border", "threads_64_fused",
         "k_flow_lane8_flat<f,t>", fused=True),
    case("257-65-pairs-fused-no-sums", 257, 65, "k_flow_lane8_flat<f,f>", fused=True, mean_subtract=0),
    case("257-65-pairs-fused-half-pixel", 257, 65, "k_flow_lane8_flat<t,t>", fused=True, subpixel=1),
    case("320-9-pairs-fused-half-pixel-no-sums", 320, 9, "k_flow_lane8_flat<t,f>", "borders_on_wave_edges_only", fused=True, subpixel=1,
         mean_subtract=0),
    case("1024-1537-pairs-fused", 1024, 1537, "threads_256_fused", "finalisers_last_workgroup_one_wave", fused=True),
    case("1024-1539-pairs-fused", 1024, 1539, "threads_256_fused", "finalisers_last_workgroup_three_waves", fused=True, mean_subtract=0),
    case("258-2048-pairs-fused", 258, 2048, "pairs_at_the_vote_capacity", fused=True),
    case("258-2049-pairs-fused", 258, 2049, "one_over_the_vote_capacity_takes_k3", fused=True),
    # ---- the chunk walk
    case("289-one-pair-pruned", 289, 1, "walk_two_chunks_second_partly_live", "walk_pruned", "k_search_lane8_pruned<f>", grid="px4", mode="pruned"),
    case("289-2720-pairs-judging", 289, 2720, "walk_spw_1_at_3071_chunks", "walk_adaptive-1", grid="px4", mode="adaptive-1"),
    case("289-2721-pairs-believing", 289, 2721, "walk_spw_2_at_3072_chunks", "walk_adaptive1", "walk_carried_row_crosses_a_pair_border",
         grid="px4", mode="adaptive1"),
    case("289-2722-pairs-pruned", 289, 2722, "walk_spw_2_last_workgroup_one_chunk", "walk_3073_chunks+pruned", grid="px4", mode="pruned"),
    case("289-12250-pairs-judging", 289, 12250, "walk_spw_clamped_at_8_short_last_workgroup", "walk_last_chunk_partly_live",
         "walk_report_stride_over_1", grid="px4", mode="adaptive-1"),
    case("289-2722-pairs-two-levels-believing", 289, 2722, "two_levels_walk", grid="px4", mode="adaptive1", levels=2),
    case("289-2722-pairs-half-pixel-judging", 289, 2722, "walk_half_pixel", "k_search_lane8_pruned<t>", grid="px4", mode="adaptive-1", subpixel=1),
]


def plan_case(id, nb, n_pairs, **kw):
    """A launch for the plan alone (kw of flat_plan; w, h default to a frame of 640 x 480)."""
    return dict(id=id, nb=nb, n_pairs=n_pairs, kw=kw)


# plans and decodes alone: the boundaries of every rule at their value and one either side
CPU_CASES = [
    plan_case("threads-1572863", 1, 1572863), plan_case("threads-1572864", 1, 1572864), plan_case("threads-1572865", 1, 1572865),
    plan_case("threads-1572863-fused", 1023, 1537, fused=True), plan_case("threads-switch-fused", 1024, 1536, fused=True),
    plan_case("walk-1535-chunks", 256, 1535, prune=1), plan_case("walk-3071-chunks", 256, 3071, prune=1),
    plan_case("walk-3072-chunks", 256, 3072, prune=1), plan_case("walk-3073-chunks", 256, 3073, prune=2),
    plan_case("walk-4607-chunks", 256, 4607, prune=1), plan_case("walk-4608-chunks", 256, 4608, prune=1),
    plan_case("walk-12287-chunks", 256, 12287, prune=1), plan_case("walk-12288-chunks", 256, 12288, prune=1),
    plan_case("walk-13824-chunks", 256, 13824, prune=1), plan_case("walk-13825-chunks", 256, 13825, prune=2),
    plan_case("walk-256-workgroups", 256, 256, prune=1), plan_case("walk-257-workgroups", 256, 257, prune=1),
    plan_case("walk-one-item", 1, 1, prune=1), plan_case("walk-257-items", 257, 1, prune=1),
    plan_case("prune-large-2047", 256, 2047), plan_case("prune-large-2048", 256, 2048),
    plan_case("vga-128", 4661, 128), plan_case("vga-1024", 4661, 1024, fused=True), plan_case("vga-1024-pruned", 4661, 1024, prune=1),
    plan_case("nb-65-fused", 65, 100, fused=True), plan_case("nb-127-fused", 127, 1000, fused=True),
]

# the plan alone, against the C++ function: slices, verdicts, extreme shapes
PLAN_ONLY = [
    plan_case("per-at-the-24-bit-cap", 127, (1 << 24) + 5),                    # 0x7FFF0000 / 127 = 16 908 804 > 2^24 - 1
    plan_case("per-at-the-24-bit-cap-slice-1", 127, (1 << 24) + 5, slice=1),
    plan_case("per-just-under-the-cap", 129, (1 << 24) + 5),                   # 0x7FFF0000 / 129 = 16 646 652
    plan_case("two-slices-first", 4661, 460720 + 100, w=640, h=480),          # 0x7FFF0000 / 4661 = 460 720
    plan_case("two-slices-second", 4661, 460720 + 100, slice=1, prune=1),
    plan_case("two-slices-exact", 4661, 2 * 460720, slice=1),
    plan_case("three-slices-first", 4661, 2 * 460720 + 1, fused=True, capacity=1 << 20),
    plan_case("three-slices-second", 4661, 2 * 460720 + 1, slice=1, fused=True, capacity=1 << 20),
    plan_case("three-slices-third", 4661, 2 * 460720 + 1, slice=2, prune=1),
    plan_case("slice-beyond-the-last", 4661, 2 * 460720 + 1, slice=3),
    plan_case("no-pairs", 300, 0), plan_case("no-blocks", 0, 5),
    plan_case("votes-pruned", 300, 10, prune=1, fused=False), plan_case("votes-no-memory", 300, 10, votes=(0, 1, 128)),
    plan_case("votes-none", 300, 10, votes=None),
    plan_case("votes-no-fault-word", 300, 10, votes=(1, 0, 128)), plan_case("votes-bins-63", 300, 10, rng=15),
    plan_case("votes-bins-59", 300, 10, rng=14), plan_case("votes-stride-111", 300, 10, rng=13, votes=(1, 1, 111)),
    plan_case("votes-stride-112", 300, 10, rng=13, votes=(1, 1, 112)), plan_case("votes-grid-64", 64, 10), plan_case("votes-grid-65", 65, 10),
    plan_case("votes-capacity", 300, 2048), plan_case("votes-over-capacity", 300, 2049),
    plan_case("votes-capacity-of-a-slice", 4661, 460720 + 100, capacity=460720), plan_case("votes-capacity-of-a-slice-less-1", 4661, 460720 + 100, capacity=460719),
    plan_case("tile-16", 300, 10, tile=16), plan_case("search-8", 300, 10, search=8),
    plan_case("frame-2^24", 300, 10, w=4096, h=4096), plan_case("frame-over-2^24", 300, 10, w=4097, h=4096),
    plan_case("nb-2^24", 1 << 24, 1, w=4096, h=4096), plan_case("stride-negative", 300, 10, pair_stride=-307200),
    plan_case("span-at-2^32", 300, 10, pair_stride=(0xFFFFFFFF - 307200) // 2), plan_case("span-over-2^32", 300, 10, pair_stride=(0xFFFFFFFF - 307200) // 2 + 1),
    plan_case("span-nb-7", 7, 10, pair_stride=(0xFFFFFFFF - 307200) // 11), plan_case("span-nb-7-over", 7, 10, pair_stride=(0xFFFFFFFF - 307200) // 11 + 1),
    plan_case("one-pair-any-stride", 300, 1, pair_stride=1 << 40),
]


def plan_args(c):
    """A case of any list as the arguments of flat_plan."""
    if "kw" in c:
        kw = dict(c["kw"])
        w, h = kw.pop("w", 640), kw.pop("h", 480)
        base = dict(nb=c["nb"], n_pairs=c["n_pairs"], pair_stride=w * h, w=w, h=h, prune=0, fused=False, rng=4, votes=(1, 1, VOTE_STRIDE),
                    capacity=VOTE_PAIRS, slice=0, tile=8, search=4)
        base.update(kw)
        return base
    pl = case_plan(c)
    return dict(nb=c["nb"], n_pairs=c["n_pairs"], pair_stride=pair_stride(c), w=c["w"], h=c["h"], prune=prune_of(c), fused=pl["kind"] == "fused",
                rng=hist_range(c), votes=(1, 1, VOTE_STRIDE), capacity=VOTE_PAIRS, slice=0, tile=8, search=4)


def plan_of(c):
    return flat_plan(**plan_args(c))


CASES = CPU_CASES + GPU_CASES + PLAN_ONLY


def _selftest_line(c):
    """The case as tests/native/host_selftest.cpp reads it: nb n_pairs pair_stride w h prune fused rng votes_memory votes_fault
    votes_stride (votes_memory -1: no VoteMem at all) capacity slice tile search"""
    a = plan_args(c)
    mem, fault, stride = a["votes"] if a["votes"] else (-1, 0, 0)
    return rig.joined([a["nb"], a["n_pairs"], a["pair_stride"], a["w"], a["h"], a["prune"], int(a["fused"]), a["rng"], mem, fault, stride, a["capacity"],
                       a["slice"], a["tile"], a["search"]])


def selftest_families():
    """lane8_flat_plan == flat_plan(), on every case of every list; the C++ xcd_remap (the text the kernels run) == xcd_remap()
    at every probe, a probe a line: total b."""
    return [rig.family("lane8-plan", "lane8 plan: ", CASES, _selftest_line, lambda c: _plan_fields(plan_of(c)), PLAN_FIELDS),
            rig.family("xcd-probes", "xcd remap: ", [dict(id=f"{total}/{b}", total=total, b=b) for total, b in _xcd_probes()],
                       lambda p: f"{p['total']} {p['b']}", lambda p: [int(xcd_remap(p["b"], p["total"]))], ("logical id",), summary="xcd_remap: {} probes")]


def _xcd_probes():
    """(total, b) pairs at which the self-test prints the C++ xcd_remap: every b of small totals with each remainder mod 8, and
    for the workgroup count of every case the first and last sixteen hardware ids and the XCD borders."""
    probes = [(total, b) for total in list(range(1, 18)) + [63, 64, 65, 255, 257] for b in range(total)]
    for total in sorted({plan_of(c)["grid"] for c in CASES} - {0}):
        q = total // 8
        bs = set(range(min(16, total))) | set(range(max(0, total - 16), total)) | {b for k in range(8) for b in (8 * (q - 1) + k, 8 * q + k)}
        probes += [(total, b) for b in sorted(bs) if 0 <= b < total]
    return probes


# ---- the frames of a device case --------------------------------------------------------------------------------------------

DISTINCT = 7     # coprime to 2, 4, 8 and 64: every content meets every lane position, chunk slot and finaliser slot
# (name, shift at one level, shift at two levels, what is added to cur)
CONTENTS = (("texture", (3, -2), (-8, 6), 0), ("texture", (-1, 4), (6, -8), 40), ("texture", (2, 3), (-6, -4), -35),
            ("bright", (-3, -4), (4, 8), -30), ("noise", (0, 0), (-4, -6), 12), ("flat", None, None, 7), ("terraces", (0, 0), (8, 2), 17))
REACH = 12
PINNED = {   # sha256 of the seven prevs and curs of a geometry: (w, h, levels) -> digest
    (16, 2064, 1): "a9de5bdda0983bbbcfb46b941fc8cdf08f1e99eb410558cb9461c60c6f3bf890",
    (32, 864, 2): "3d4cae023f91544064307035c186a68e2ba8648b87f2519b71d51d5f3ad5cf34",
    (18, 2066, 1): "d7c17338825d04998b43843d0d6073e35446b5e7535171a5ed6f013418d6bbf2",
    (138, 170, 1): "1f5ab8b4fb38a530fd87daa06ff8a7976bee6d8d4e8ed987104162d391b9122f",
    (136, 200, 1): "32e17a6436ffa18e8c93ef9f336a84d455e99d431518e57e8f61624ff13514db",
    (96, 288, 1): "a5b4aa7542320a718275f84ac17b923a076771a5a23474f4f2a683dc1751ccdc",
    (145, 136, 1): "70d053ae7ead804c7ad089b4fe283c2006478c0c036fd1100bcf2ad8d1b03077",
    (264, 264, 1): "55c28cee715e754b42b6395a643f822a5b41b355d4ba027d847f048955c9961d",
    (56, 352, 1): "d3c2f67f66d7483e1beca59e96eee7dbbcc1f1787e32ce3cc1935a8edff4b94a",
    (35, 35, 1): "11d636e3d6f1a8ebb481fdc40217c0c4d9bd86632e8843da71b2e871fd14e4ab",
    (52, 52, 2): "f11f45516de32865c841abc1b950d1a40ddb535cb2b913485e870200b1e51010",
}


def _crop(canvas, w, h, shift):
    dx, dy = shift
    return canvas[REACH:REACH + h, REACH:REACH + w], canvas[REACH - dy:REACH - dy + h, REACH - dx:REACH - dx + w]


def pairs_for(c, synth):
    """The case's seven distinct pairs (prevs, curs: uint8 [7, h, w]), integers only.  texture: synth.make_pair's blurred
    field at an integer shift, as drawn, with cur + 40 and with cur - 35; bright: values of 230 and more with cur - 30 and a few
    hot pixels, so that adding the delta saturates; noise: unrelated in every pixel (at two levels: a level-1 texture under noise
    whose 2 x 2 sums are zero, so that level 1 still finds a predictor); flat; terraces: rows constant inside stripes of 24
    columns, so that horizontal candidates tie exactly."""
    w, h, two = c["w"], c["h"], c["levels"] == 2
    prevs, curs = np.empty((DISTINCT, h, w), np.uint8), np.empty((DISTINCT, h, w), np.uint8)
    for j, (name, one, both, add) in enumerate(CONTENTS):
        shift = both if two else one
        rng = np.random.Generator(np.random.PCG64(7700 + j))
        H, W = h + 2 * REACH, w + 2 * REACH
        if name == "texture":
            a, b, _ = synth.make_pair(w, h, REACH, 7700, shift=shift)      # (the same field three times)
        elif name == "bright":
            a, b = _crop(230 + rng.integers(0, 26, size=(H, W)), w, h, shift)
        elif name == "noise" and not two:
            a, b = rng.integers(0, 256, size=(h, w)), rng.integers(20, 200, size=(h, w))
        elif name == "noise":
            cells = 70 + rng.integers(0, 116, size=(H // 2 + 1, W // 2 + 1))
            base = np.repeat(np.repeat(cells, 2, axis=0), 2, axis=1)[:H, :W]
            sign = np.where((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2 == 0, 1, -1)
            rows = np.where(np.arange(H)[:, None] % 2 == 0, 1, -1)          # (cur: another pattern whose 2 x 2 sums are zero)
            amp = lambda: np.repeat(np.repeat(rng.integers(50, 66, size=(H // 2 + 1, W // 2 + 1)), 2, axis=0), 2, axis=1)[:H, :W]
            a, _ = _crop(base + sign * amp(), w, h, (0, 0))
            _, b = _crop(base, w, h, shift)
            b = b + (rows * amp())[REACH:REACH + h, REACH:REACH + w]
        elif name == "flat":
            a, b = np.full((h, w), 90), np.full((h, w), 90)
        else:
            level = rng.integers(0, 5, size=(H // 3 + 1, W // 24 + 1))
            level = (level + np.arange(H // 3 + 1)[:, None]) % 5              # (consecutive terraces of a stripe always differ)
            field = 60 + 35 * np.repeat(np.repeat(level, 3, axis=0), 24, axis=1)[:H, :W]
            a, b = _crop(field, w, h, shift)
        a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64) + add
        if name == "bright":
            b.reshape(-1)[5::37] = 255
        prevs[j], curs[j] = np.clip(a, 0, 255), np.clip(b, 0, 255)
    return prevs, curs


def digest(prevs, curs):
    return hashlib.sha256(prevs.tobytes() + curs.tobytes()).hexdigest()


def delta_of(prev, cur):
    return rounded_mean(prev) - rounded_mean(cur)


def check_inputs(c, p, prevs, curs, outs):
    """Before the device runs: each content does what it is there for.  outs: the oracle's flow_pair of the seven pairs."""
    two, nb = c["levels"] == 2, c["nb"]
    sad = lambda j: outs[j]["blocks"]["sad"]
    name = [k[0] for k in CONTENTS]
    flat, noise, terr, bright = name.index("flat"), name.index("noise"), name.index("terraces"), name.index("bright")
    assert (sad(flat) == 0xFFFF).all(), "a flat pair: every block gated"
    live = sad(noise) != 0xFFFF
    assert live.any() and (sad(noise)[live] >= p.value_threshold).all(), "unrelated noise: every block rejected"
    deltas = [delta_of(a, b) for a, b in zip(prevs, curs)]
    # (-40 and +35 next to 0; the shift and the pixels that saturate move the mean of a small frame by an LSB or two)
    assert all(abs(d - w) <= 2 for d, w in zip(deltas[:3], (0, -40, 35))), deltas
    assert all(deltas[j] != deltas[(j + 1) % DISTINCT] for j in range(DISTINCT)), ("neighbours share a delta", deltas)
    if c["mean_subtract"]:
        assert deltas[bright] >= 25 and (curs[bright].astype(np.int64) + deltas[bright] > 255).any(), "adding the delta saturates"
        for j in range(3):
            ok = sad(j) != 0xFFFF
            assert ok.any() and (sad(j)[ok] < p.value_threshold).mean() > 0.9, (j, "a textured pair matches under its delta")
    if not two:
        b = outs[terr]["blocks"]
        tied = (b["sad"] == (0 if c["mean_subtract"] else 64 * 17)) & (b["dx"] == -4)    # (cur + 17: the delta takes it off again)
        assert tied.any(), "terraces: exact ties, won by the first candidate in scan order"
        for j in range(3 if c["mean_subtract"] else 1):      # (without equalisation only the pair drawn as it is matches where it was put)
            ok = sad(j) < p.value_threshold
            hit =(outs[j]["blocks"]["dx"][ok] == CONTENTS[j][1][0]) & (outs[j]["blocks"]["dy"][ok] == CONTENTS[j][1][1])
            assert hit.mean() > 0.9 and (j or hit.all()), (j, "the blocks report the shift (a delta an LSB off lets a few weak ones stray)")
    else:
        preds = [(int(o["flow"]["pred_x"]), int(o["flow"]["pred_y"])) for o in outs]
        assert len(set(preds)) == DISTINCT and preds[flat] == (0, 0), ("seven different predictors, (0, 0) among them", preds)
        assert all(preds[j] != preds[(j + 1) % DISTINCT] for j in range(DISTINCT)), preds
        for axis in (0, 1):
            assert min(q[axis] for q in preds) < 0 < max(q[axis] for q in preds), ("both signs on both axes", preds)
        skipped = [int((sad(j) == 0xFFFF).sum()) for j in range(3)]
        assert any(0 < s < nb for s in skipped), ("a predictor pushes edge windows out of the frame", skipped)
    key = (c["w"], c["h"], c["levels"])
    assert PINNED.get(key) == digest(prevs, curs), (key, digest(prevs, curs))
