"""The column walk's segment plan in plain Python (csrc/aof_cols8_plan.hpp: cols_plan_make), the kernel's unit decode in
integer arithmetic (csrc/aof_cols8_kernels.hpp: the head of cols_walk), the names of the paths a launch can take through
both, and the case lists of tests/test_cols_plan_ref.py, tests/test_host_asan.py (the same plan from the C++ function)
and tests/test_gpu_cols_plan.py (every case of GPU_CASES on the device, against the oracle).

A case is a frame size (through its dense grid), a pair count and the form of the launch; reach() says which paths it
takes, the census of tests/test_cols_plan_ref.py fails on a path no device case takes."""
import numpy as np

import selftest_rig as rig

# csrc/aof_cols8_plan.hpp, csrc/aof_ctx.hpp, csrc/aof_engine_args.hpp
THREADS, MAX_ROWS, MIN_ROWS, WAVES_WANTED, WAVE_SLOTS, MAX_UNITS = 256, 8, 2, 3072, 4096, 0x7FFF0000
VOTE_PAIRS, PRUNE_MIN_CHUNKS = 2048, 2048
TILE, SEARCH = 8, 4


# ---- the plan ----------------------------------------------------------------------------------------------------

def fastdiv_make(d):
    """(mul, shift) of aof_fastdiv.hpp's fastdiv_make."""
    if d == 0:
        return 0, 0
    l = 0
    while (1 << l) < d:
        l += 1
    return (((1 << 32) * ((1 << l) - d)) // d + 1) & 0xFFFFFFFF, l


def fast_div(n, fd):
    """aof_device.hpp's fast_div on numpy uint64 arrays (or ints) holding 32-bit values: every step in 32 bits."""
    mul, shift = fd
    n = np.asarray(n, dtype=np.uint64)
    return (((n * np.uint64(mul)) >> np.uint64(32)) + n & np.uint64(0xFFFFFFFF)) >> np.uint64(shift)


def segments(nx, ny, length):
    length = min(length, ny)
    segs = (ny + length - 1) // length
    upp = (segs * nx + 63) // 64 * 64
    return dict(len=length, segs=segs, units_per_pair=upp, div_units=fastdiv_make(upp))


def plan(nx, ny, n_pairs, w=None, h=None, pair_stride=None, cur=0, step_x=8, done=0):
    """cols_plan_make for the launch that starts at pair `done` of a call of n_pairs pairs.  w, h default to the smallest
    plain frame of the grid, pair_stride to w * h, cur (the frame array's address) to an aligned one."""
    w = 8 * nx + 8 if w is None else w
    h = 8 * ny + 8 if h is None else h
    pair_stride = w * h if pair_stride is None else pair_stride
    length, clipped_in_loop = MAX_ROWS, False
    while length > MIN_ROWS and n_pairs * (segments(nx, ny, length)["units_per_pair"] // 64) < WAVES_WANTED:
        clipped_in_loop |= length > ny
        length -= 1
    head, tail = segments(nx, ny, length), segments(nx, ny, max(length // 2, MIN_ROWS))
    aligned = int(step_x == 8 and w % 4 == 0 and pair_stride % 4 == 0 and cur % 4 == 0 and (w * h) % 4 == 0)
    per = MAX_UNITS // tail["units_per_pair"]
    pairs = min(n_pairs - done, per)
    wpp = head["units_per_pair"] // 64
    all_waves = pairs * wpp
    rest = all_waves % WAVE_SLOTS
    # the four conditions of a tail class, each by itself: a launch without a tail names the ones that fail
    why = dict(all_le_slots=all_waves <= WAVE_SLOTS, rest_zero=rest == 0, rest_large=rest * 5 >= WAVE_SLOTS * 4,
               len_equal=tail["len"] >= head["len"])
    tail_pairs = 0 if any(why.values()) else (rest + wpp - 1) // wpp
    head_pairs = pairs - tail_pairs
    head_units = (head_pairs * head["units_per_pair"]) & 0xFFFFFFFF
    units = head_units + tail_pairs * tail["units_per_pair"]
    return dict(nx=nx, ny=ny, n_pairs=pairs, head=head, tail=tail, div_nx=fastdiv_make(nx), aligned=aligned, per=per,
                tail_pairs=tail_pairs, head_pairs=head_pairs, head_units=head_units, units=units,
                wgs=(units + THREADS - 1) // THREADS, wpp=wpp, all=all_waves, rest=rest, no_tail_because=why,
                asked=(length, max(length // 2, MIN_ROWS)), clipped_in_loop=clipped_in_loop)


PLAN_FIELDS = ("head.len", "head.segs", "head.units_per_pair", "head.mul", "head.shift", "tail.len", "tail.segs",
               "tail.units_per_pair", "tail.mul", "tail.shift", "head_pairs", "head_units", "nx.mul", "nx.shift", "aligned",
               "per", "pairs", "tail_pairs", "units", "wgs")


def _plan_fields(pl):
    """The plan as the flat list of numbers the host self-test prints for cols_plan_make (PLAN_FIELDS)."""
    out = []
    for cls in ("head", "tail"):
        s = pl[cls]
        out += [s["len"], s["segs"], s["units_per_pair"], s["div_units"][0], s["div_units"][1]]
    return out + [pl["head_pairs"], pl["head_units"], pl["div_nx"][0], pl["div_nx"][1], pl["aligned"], pl["per"], pl["n_pairs"],
                  pl["tail_pairs"], pl["units"], pl["wgs"]]


# ---- the kernel's decode -------------------------------------------------------------------------------------------

def decode(pl, unit0=None):
    """What cols_walk makes of the launch's threads (unit0: their global indices, default all wgs * 256 of them), lane by
    lane, the way the kernel computes it: the class and the pair are the FIRST lane's (readfirstlane) for the whole wave.
    Returns arrays over the threads: in_tail, pair, returns (the wave leaves: pair >= n_pairs), local, seg, bx, live, by0,
    len; and `lane_class` / `lane_pair`, what every lane would have computed for itself -- a wave in which those differ
    from the first lane's is a wave that holds two classes or two pairs."""
    u64 = np.uint64
    if unit0 is None:
        unit0 = np.arange(pl["wgs"] * THREADS, dtype=np.uint64)
    unit0 = np.asarray(unit0, dtype=np.uint64)
    assert unit0.size % 64 == 0 and (unit0[::64] % u64(64) == 0).all(), "whole waves"
    first = np.repeat(unit0[::64], 64)
    hu, hp, nx = u64(pl["head_units"]), u64(pl["head_pairs"]), u64(pl["nx"])

    def of(first_lane):
        in_tail = first_lane >= hu
        upp = np.where(in_tail, u64(pl["tail"]["units_per_pair"]), u64(pl["head"]["units_per_pair"]))
        return in_tail, upp

    in_tail, upp = of(first)
    unit = np.where(in_tail, unit0 - hu & u64(0xFFFFFFFF), unit0)
    unit_first = np.where(in_tail, first - hu & u64(0xFFFFFFFF), first)
    q = lambda n: np.where(in_tail, fast_div(n, pl["tail"]["div_units"]), fast_div(n, pl["head"]["div_units"]))
    base = np.where(in_tail, hp, u64(0))
    pair = base + q(unit_first) & u64(0xFFFFFFFF)
    returns = pair >= u64(pl["n_pairs"])
    local = unit - (pair - base) * upp & u64(0xFFFFFFFF)
    seg = fast_div(local, pl["div_nx"])
    bx = local - (seg & u64(0xFFFFFF)) * (nx & u64(0xFFFFFF)) & u64(0xFFFFFFFF)   # __umul24
    segs = np.where(in_tail, u64(pl["tail"]["segs"]), u64(pl["head"]["segs"]))
    length = np.where(in_tail, pl["tail"]["len"], pl["head"]["len"]).astype(np.int64)
    live = local < segs * nx
    # every lane for itself
    lane_class = unit0 >= hu
    lane_unit = np.where(lane_class, unit0 - hu & u64(0xFFFFFFFF), unit0)
    lane_pair = np.where(lane_class, hp + fast_div(lane_unit, pl["tail"]["div_units"]), fast_div(lane_unit, pl["head"]["div_units"]))
    return dict(unit0=unit0, in_tail=in_tail, pair=pair.astype(np.int64), returns=returns, local=local.astype(np.int64),
                seg=seg.astype(np.int64), bx=bx.astype(np.int64), live=live, by0=seg.astype(np.int64) * length, len=length,
                lane_class=lane_class, lane_pair=lane_pair.astype(np.int64))


def coverage(pl, d):
    """How often the walk writes each (pair, by, bx) of the launch: an int array [n_pairs, ny, nx].  Lanes of waves that
    leave and lanes that are not live write nothing; a record index outside the launch's arrays raises."""
    nx, ny, n = pl["nx"], pl["ny"], pl["n_pairs"]
    count = np.zeros(n * ny * nx, dtype=np.int64)
    walks = d["live"] & ~d["returns"]
    pair, bx, by0, length = d["pair"][walks], d["bx"][walks], d["by0"][walks], d["len"][walks]
    assert (pair < n).all() and (bx < nx).all()
    for step in range(MAX_ROWS):
        act = (step < length) & (by0 + step < ny)
        count += np.bincount(((pair[act] * ny + by0[act] + step) * nx + bx[act]), minlength=count.size)
    return count.reshape(n, ny, nx)


# ---- cases and what they reach -------------------------------------------------------------------------------------

def case(id, nx, ny, n_pairs, *paths, subpixel=0, levels=1, wpad=0, hpad=0, mode="pruned", fused=False, graph=False, px=()):
    """nx x ny: the dense grid; the frame is the smallest that has it (8 nx + 8, with the half-pixel step 8 nx + 10) plus
    wpad / hpad pixels (< 8: the grid stays).  levels=2 comes with mean_subtract=1 (a predictor and an equalisation
    delta per pair); px: the predictors' x of the distinct pairs, as the oracle computes them from pairs_for()'s frames
    (tests/test_cols_plan_ref.py holds the list to the oracle).  mode: 'pruned' (AOF_SEARCH_PRUNED), 'adaptive1' /
    'adaptive0' (the default mode told that pruning pays / does not: the first block of every wave judges).  fused: the
    caller asks for the reduction in the launch; graph: the launch is also captured and replayed."""
    assert 0 <= wpad < 8 and 0 <= hpad < 8 and mode in ("pruned", "adaptive1", "adaptive0") and levels in (1, 2)
    m = 2 * (SEARCH + subpixel)
    return dict(id=id, nx=nx, ny=ny, n_pairs=n_pairs, paths=paths, subpixel=subpixel, levels=levels, w=TILE * nx + m + wpad,
                h=TILE * ny + m + hpad, mode=mode, fused=fused, graph=graph, px=tuple(px))


def params_kw(c):
    kw = dict()
    if c["subpixel"]:
        kw["subpixel"] = 1
    if c["levels"] == 2:
        kw.update(pyramid_levels=2, mean_subtract=1)
    return kw


def case_plan(c):
    return plan(c["nx"], c["ny"], c["n_pairs"], c["w"], c["h"])


def launch_of(c):
    """choose_lane8 of the case's level-0 launch (batch_plan_ref owns the rule): a context in the case's mode, told what the
    mode's name says -- 'adaptive0' at the launch that looks again --, the in-launch reduction switched as the case asks."""
    import batch_plan_ref as bp
    call = bp.of_cols(c)
    st = bp.fresh_state({"pruned": -1, "adaptive1": 1, "adaptive0": 0}[c["mode"]], bp.PROBE_EVERY - 1 if c["mode"] == "adaptive0" else 0)
    return bp.choose_lane8(call["mode"], st, bp.lane8_args(call), separate=not c["fused"])


def votes(c):
    """The reduction runs in the launch (k_flow_lane8_cols): asked for, and the context's vote records hold the launch."""
    return launch_of(c)["fused"]


def runs_the_walk(c):
    """lane8_cols_supported, and for the adaptive mode a launch large enough to prune (adaptive_lane8_prunes)."""
    return launch_of(c)["cols"]


def misalignments(c, pl):
    """wx0 & 3 of the case's pairs where the shifted-load route is on (plan.aligned), else only 0: wx0 = x0 + 8 bx + px - 4
    with x0 = 4, or 5 with the half-pixel step."""
    if not pl["aligned"]:
        return {0}
    return {(c["subpixel"] + px) & 3 for px in (c["px"] or (0,))}


UNREACHABLE = {"second_launch_of_the_per_split": "needs more than 2^31 units in one call: at two rows per unit that is over 400 GB of "
                                                 "frames on any grid, more than the device has memory"}

# forms the issue wants seen with a tail class and with a head length of 4 to 7
FORMS = {
    "mode_pruned": lambda c: c["mode"] == "pruned",
    "mode_adaptive_belief_1": lambda c: c["mode"] == "adaptive1",
    "mode_adaptive_belief_0": lambda c: c["mode"] == "adaptive0",
    "vote_on": votes,
    "vote_off": lambda c: not votes(c),
    "plain": lambda c: not c["subpixel"] and c["levels"] == 1,
    "subpixel_on": lambda c: bool(c["subpixel"]),
    "two_levels": lambda c: c["levels"] == 2,
    "aligned_0": lambda c: not case_plan(c)["aligned"],
}


def reach(c):
    """The names of the paths the case takes (VOCABULARY)."""
    assert runs_the_walk(c), c["id"]
    pl = case_plan(c)
    d = decode(pl)
    got = {f"head_len_{pl['head']['len']}"}
    tail = pl["tail_pairs"] > 0
    if tail:
        got.add(f"tail_len_{pl['tail']['len']}")
    else:
        got |= {"no_tail_because_" + k for k, v in pl["no_tail_because"].items() if v}
    if pl["asked"][0] > pl["ny"]:
        got.add("head_len_clipped_to_ny")
    if pl["asked"][1] > pl["ny"]:
        got.add("tail_len_clipped_to_ny")
    if pl["clipped_in_loop"]:
        got.add("len_clipped_to_ny_while_choosing_the_length")
    walks = d["live"] & ~d["returns"]
    if (walks & (d["by0"] + d["len"] > pl["ny"])).any():
        got.add("ragged_last_segment")
    seg_w, walks_w = d["seg"].reshape(-1, 64), walks.reshape(-1, 64)
    lo = np.where(walks_w, seg_w, 1 << 40).min(axis=1)
    hi = np.where(walks_w, seg_w, -1).max(axis=1)
    if (hi > lo).any():
        got.add("wave_spans_two_segments")
    if (~d["live"] & ~d["returns"]).any():
        got.add("padding_lanes_in_a_pairs_last_wave")
    if tail and pl["head_units"] % THREADS != 0:
        got.add("workgroup_spans_the_class_border")
    pair_g = np.where(d["returns"], -1, d["pair"]).reshape(-1, THREADS)
    top = pair_g.max(axis=1)
    bottom = np.where(pair_g < 0, 1 << 40, pair_g).min(axis=1)
    if (top > bottom).any():
        got.add("workgroup_spans_two_pairs")
    got.add(f"aligned_{pl['aligned']}")
    mis = misalignments(c, pl)
    got |= {f"mis_{m}" for m in mis}
    if mis - {0}:
        lane = d["unit0"] % np.uint64(64)
        if (walks & (d["bx"] + 1 == pl["nx"])).any():
            got.add("lonely_lane_by_row_end")
        if (walks & (lane == 63) & (d["bx"] + 1 != pl["nx"])).any():
            got.add("lonely_lane_by_lane_63")
    got |= {"vote_on" if votes(c) else "vote_off", "subpixel_on" if c["subpixel"] else "subpixel_off", "mode_" + dict(
        pruned="pruned", adaptive1="adaptive_belief_1", adaptive0="adaptive_belief_0")[c["mode"]]}
    if c["levels"] == 2:
        got |= {"delta_nonzero", "predictor"}     # (pairs_for() gives every pair a brightness step; held to the oracle)
    if c["fused"] and not votes(c):
        got.add("fusion_asked_but_over_the_vote_records")
    if c["graph"]:
        got.add("graph_replay" + ("_fused_tail" if votes(c) and tail else ""))
    for name, pred in FORMS.items():
        if pred(c):
            if tail:
                got.add(name + "+tail")
            if 4 <= pl["head"]["len"] <= 7:
                got.add(name + "+head_4_to_7")
    if tail and mis - {0}:
        got.add("misaligned_pair+tail")
    if pl["tail_pairs"] == 1:
        got.add("tail_of_one_pair")
    if (c["w"] * c["h"]) % 4:
        got.add("pair_bases_not_dword_aligned")   # the frames of every other pair start two bytes off a dword
    return got


VOCABULARY = (
    [f"head_len_{k}" for k in range(2, 9)] + [f"tail_len_{k}" for k in (2, 3, 4)]
    + ["no_tail_because_" + k for k in ("all_le_slots", "rest_zero", "rest_large", "len_equal")]
    + ["head_len_clipped_to_ny", "tail_len_clipped_to_ny", "len_clipped_to_ny_while_choosing_the_length", "ragged_last_segment", "wave_spans_two_segments", "padding_lanes_in_a_pairs_last_wave",
       "workgroup_spans_the_class_border", "workgroup_spans_two_pairs", "aligned_0", "aligned_1", "mis_0", "mis_1", "mis_2", "mis_3",
       "lonely_lane_by_row_end", "lonely_lane_by_lane_63", "vote_on", "vote_off", "subpixel_on", "subpixel_off", "delta_nonzero",
       "predictor", "mode_pruned", "mode_adaptive_belief_1", "mode_adaptive_belief_0", "fusion_asked_but_over_the_vote_records",
       "graph_replay_fused_tail", "misaligned_pair+tail", "tail_of_one_pair", "pair_bases_not_dword_aligned"]
    + [f + "+tail" for f in FORMS] + [f + "+head_4_to_7" for f in FORMS] + list(UNREACHABLE))


# ---- plan-only cases: every boundary of the plan at its value and one either side -----------------------------------

def plan_case(id, nx, ny, n_pairs, **kw):
    """A launch for the plan and the decode alone (kw: w, h, pair_stride, cur, step_x of plan())."""
    return dict(id=id, nx=nx, ny=ny, n_pairs=n_pairs, kw=kw)


CPU_CASES = [
    # 17 x 16 at eight rows: one wave per pair, so the pair count IS the wave count
    plan_case("waves-wanted-minus-1", 17, 16, WAVES_WANTED - 1),      # 3 071 waves at every length down to 6: five rows, two waves
    plan_case("waves-wanted", 17, 16, WAVES_WANTED),                  # eight rows
    plan_case("waves-wanted-plus-1", 17, 16, WAVES_WANTED + 1),
    plan_case("slots-minus-1", 17, 16, WAVE_SLOTS - 1),
    plan_case("slots", 17, 16, WAVE_SLOTS),                           # all == kWaveSlots: no tail (and rest == 0)
    plan_case("slots-plus-1", 17, 16, WAVE_SLOTS + 1),                # one tail pair
    plan_case("slots-plus-2", 17, 16, WAVE_SLOTS + 2),
    plan_case("rest-3275", 17, 16, WAVE_SLOTS + 3275),
    plan_case("rest-3276", 17, 16, WAVE_SLOTS + 3276),                # 16 380 < 16 384: the last launch with a tail
    plan_case("rest-3277", 17, 16, WAVE_SLOTS + 3277),                # 16 385: none
    plan_case("rest-3278", 17, 16, WAVE_SLOTS + 3278),
    plan_case("two-generations-minus-1", 17, 16, 2 * WAVE_SLOTS - 1),
    plan_case("two-generations", 17, 16, 2 * WAVE_SLOTS),             # rest == 0 and nothing else in the way
    plan_case("two-generations-plus-1", 17, 16, 2 * WAVE_SLOTS + 1),
    # three waves per pair: the border falls inside a workgroup, a tail pair is a ROUNDED-UP share of the rest
    plan_case("3wpp-4095", 65, 6, 1365),
    plan_case("3wpp-4098", 65, 6, 1366),
    plan_case("3wpp-4101", 65, 6, 1367),
    plan_case("3wpp-rest-1", 65, 6, 2731),                            # 8 193 waves: rest 1, one tail pair for a third of a pair
    plan_case("3wpp-rest-3276", 65, 6, 2457),                         # 7 371 waves: rest 3 275
    plan_case("3wpp-rest-3278", 65, 6, 2458),                         # 7 374 waves: rest 3 278
    # the length clipped to the grid's rows: while choosing, in the head, in the tail
    plan_case("ny5-clipped-while-choosing", 100, 5, 1100),
    plan_case("ny5-head-clipped", 65, 5, 2100),
    plan_case("ny3-both-clipped", 87, 3, 2100),
    plan_case("ny2-both-clipped", 130, 2, 1500),
    plan_case("ny9-one-row-segment", 65, 9, 1400),                    # 9 = 8 + 1: the last head segment is one row
    plan_case("ny17-tail", 16, 17, 4100),                             # the narrowest grid the walk takes
    # columns against the wave: nx a multiple of 64 (no padding, no wave across segments), one short, one over
    plan_case("nx64", 64, 5, 1400),
    plan_case("nx63", 63, 5, 1400),
    plan_case("nx128", 128, 3, 1100),
    plan_case("nx129", 129, 3, 1100),
    # every head length on one grid by the pair count alone (79 x 59: VGA)
    plan_case("vga-40", 79, 59, 40), plan_case("vga-64", 79, 59, 64), plan_case("vga-80", 79, 59, 80),
    plan_case("vga-96", 79, 59, 96), plan_case("vga-112", 79, 59, 112), plan_case("vga-128", 79, 59, 128),
    plan_case("vga-256", 79, 59, 256), plan_case("vga-600", 79, 59, 600), plan_case("vga-1024", 79, 59, 1024),
    plan_case("one-pair", 79, 59, 1),
    # `aligned`: each of its five conditions alone
    plan_case("aligned", 65, 6, 1400, w=528, h=56),
    plan_case("width-2-mod-4", 65, 6, 1400, w=530, h=56),
    plan_case("width-odd", 65, 6, 1400, w=529, h=56),
    plan_case("stride-2-mod-4", 65, 6, 1400, w=528, h=56, pair_stride=528 * 56 + 2),
    plan_case("base-1-mod-4", 65, 6, 1400, w=528, h=56, cur=0x7F0000000001),
    plan_case("base-2-mod-4", 65, 6, 1400, w=528, h=56, cur=0x7F0000000002),
    plan_case("frame-2-mod-4-stride-0-mod-4", 65, 6, 1400, w=530, h=57, pair_stride=530 * 57 + 2),
    plan_case("columns-9-apart", 20, 18, 1400, w=192, h=160, step_x=9),
]

# launches nobody can decode lane by lane (or run): the plan alone, against cols_plan_make
PLAN_ONLY = [
    plan_case("per-split-first-launch", 17, 16, 0x7FFF0000 // 128 + 5),
    plan_case("per-split-second-launch", 17, 16, 0x7FFF0000 // 128 + 5, done=0x7FFF0000 // 128),
    plan_case("per-split-exact", 17, 16, 0x7FFF0000 // 128),
    plan_case("per-split-tail-units-larger", 65, 5, 3 * (0x7FFF0000 // 192) + 1400, done=2 * (0x7FFF0000 // 192)),
]


def plan_of(c):
    """The plan of a case of any of the lists."""
    return plan(c["nx"], c["ny"], c["n_pairs"], **c["kw"]) if "kw" in c else case_plan(c)


def _selftest_line(c):
    """The case as tests/native/host_selftest.cpp reads it: nx ny step_x w h pair_stride cur n_pairs done."""
    if "kw" in c:
        kw = c["kw"]
        w, h = kw.get("w", 8 * c["nx"] + 8), kw.get("h", 8 * c["ny"] + 8)
        return rig.joined((c["nx"], c["ny"], kw.get("step_x", 8), w, h, kw.get("pair_stride", w * h), kw.get("cur", 0), c["n_pairs"], kw.get("done", 0)))
    return rig.joined((c["nx"], c["ny"], 8, c["w"], c["h"], c["w"] * c["h"], 0, c["n_pairs"], 0))


def selftest_families():
    """cols_plan_make == plan(), on every case of every list."""
    return [rig.family("cols-plan", "cols plan: ", CPU_CASES + GPU_CASES + PLAN_ONLY, _selftest_line, lambda c: _plan_fields(plan_of(c)), PLAN_FIELDS)]


# ---- device cases ----------------------------------------------------------------------------------------------------

GPU_CASES = [
    case("65x4-1400-fused-graph", 65, 4, 1400, "head_len_3", "tail_len_2", "workgroup_spans_the_class_border", "ragged_last_segment",
         "wave_spans_two_segments", "padding_lanes_in_a_pairs_last_wave", "workgroup_spans_two_pairs", "vote_on+tail", "plain+tail",
         "mode_pruned+tail", "graph_replay_fused_tail", "aligned_1", "mis_0", "subpixel_off", fused=True, graph=True),
    case("65x5-1400-half-pixel-fused", 65, 5, 1400, "head_len_4", "tail_len_2", "subpixel_on+tail", "subpixel_on+head_4_to_7", "mis_1",
         "misaligned_pair+tail", "lonely_lane_by_row_end", "lonely_lane_by_lane_63", "vote_on+head_4_to_7",
         "len_clipped_to_ny_while_choosing_the_length", subpixel=1, wpad=2, fused=True),
    case("65x6-1400-two-levels-judging", 65, 6, 1400, "head_len_5", "mode_adaptive_belief_0+tail", "mode_adaptive_belief_0+head_4_to_7",
         "two_levels+tail", "two_levels+head_4_to_7", "vote_off+tail", "vote_off+head_4_to_7", "mis_1", "mis_2", "mis_3", "delta_nonzero",
         "predictor", levels=2, mode="adaptive0", px=(-7, 3, 0, 2, -2, 6, -5, 8)),
    case("65x7-1400-believing-fused", 65, 7, 1400, "head_len_6", "tail_len_3", "mode_adaptive_belief_1+tail",
         "mode_adaptive_belief_1+head_4_to_7", "plain+head_4_to_7", mode="adaptive1", fused=True),
    case("65x8-1400-two-levels-width-530-fused", 65, 8, 1400, "head_len_7", "tail_len_3", "aligned_0", "aligned_0+tail",
         "aligned_0+head_4_to_7", "mode_pruned+head_4_to_7", levels=2, wpad=2, fused=True, px=(-7, 2, 0, -6, -2, 6, -5, 8)),
    case("65x9-1400", 65, 9, 1400, "head_len_8", "tail_len_4", "vote_off", "ragged_last_segment"),
    case("17x16-2100-over-the-vote-records", 17, 16, 2100, "head_len_5", "tail_len_2", "fusion_asked_but_over_the_vote_records", fused=True),
    case("100x5-1100-half-pixel-frame-2-mod-4", 100, 5, 1100, "head_len_4", "tail_len_2", "aligned_0+tail", "subpixel_on+tail",
         "pair_bases_not_dword_aligned", subpixel=1, hpad=1, fused=True),
    case("65x6-1365-no-tail", 65, 6, 1365, "no_tail_because_all_le_slots", "no_tail_because_rest_large", fused=True),
    case("65x6-1366-one-tail-pair", 65, 6, 1366, "tail_of_one_pair", "tail_len_2", "workgroup_spans_the_class_border", fused=True),
    case("23x19-1400-two-levels-believing-fused", 23, 19, 1400, "head_len_3", "tail_len_2", "mode_adaptive_belief_1+tail", "two_levels+tail",
         "ragged_last_segment", levels=2, mode="adaptive1", fused=True, px=(-7, 3, 0, -6, -2, 6, -5, 8)),
    case("65x4-1000-two-rows", 65, 4, 1000, "head_len_2", "no_tail_because_len_equal", "no_tail_because_all_le_slots"),
    case("87x3-2100-half-pixel-clipped", 87, 3, 2100, "head_len_clipped_to_ny", "tail_len_clipped_to_ny", "no_tail_because_len_equal",
         "mis_1", subpixel=1, wpad=2),
    case("65x7-1400-fused", 65, 7, 1400, "head_len_6", "tail_len_3", "vote_on+tail", "mode_pruned+head_4_to_7", fused=True),
    # two waves per pair: one whole generation, and as many pairs as the context has vote records
    case("17x16-2048-whole-generation-fused", 17, 16, 2048, "head_len_5", "no_tail_because_rest_zero", "no_tail_because_all_le_slots",
         "vote_on", fused=True),
]

DISTINCT = 8   # distinct pairs of a device case; 7 where 8 divides the head pair count (both classes see every content)


def distinct_pairs(c):
    k = DISTINCT if case_plan(c)["head_pairs"] % DISTINCT else DISTINCT - 1
    assert case_plan(c)["head_pairs"] % k != 0
    return k


# content of the distinct pairs: (name, shift at one level, shift at two levels)
CONTENTS = [("common", (2, -3), (-7, 3)), ("split", (-1, 2), (2, -3)), ("flat", None, None), ("noise", None, None),
            ("half", (1, 1), (-2, 0)), ("common", (-4, 4), (6, 1)), ("common", (3, 0), (-5, -8)), ("common", (0, -4), (9, -9))]
SPLIT_LOWER = {(-1, 2): (3, -1), (2, -3): (3, 3)}   # the motion of the split pair's lower half


def pairs_for(c, synth):
    """The case's distinct pairs (prevs, curs: uint8 [k, h, w]): one common motion; one whose motion changes between the
    upper and the lower half (a flush inside a walk); one flat (every block gated: arrivals without votes); one of
    unrelated noise; with the half-pixel step one displaced by half a pixel; more common motions, the last with sensor
    noise.  Two levels: shifts beyond the one-level reach whose predictors take every residue mod 4 (case's px), and a
    brightness step for the equalisation."""
    w, h, two = c["w"], c["h"], c["levels"] == 2
    reach = 12 if two else 4
    bright = 9 if two else 0
    prevs, curs = [], []
    for i, (kind, one, both) in enumerate(CONTENTS[:distinct_pairs(c)]):
        shift = both if two else one
        seed = 3100 + 10 * i
        if kind == "flat":
            a, b = np.full((h, w), 7, np.uint8), np.full((h, w), 7 + bright, np.uint8)
        elif kind == "noise":
            rng = np.random.default_rng(seed)   # (low contrast: junk matches under the SAD gate, votes all over the histogram)
            a, b = rng.integers(100, 157, (h, w), dtype=np.uint8), rng.integers(100 + bright, 157 + bright, (h, w), dtype=np.uint8)
        elif kind == "split":
            a, b, _ = synth.make_pair(w, h, reach, seed, shift=shift, brightness=bright)
            _, b2, _ = synth.make_pair(w, h, reach, seed, shift=SPLIT_LOWER[shift], brightness=bright)
            b = b.copy()
            b[h // 2:] = b2[h // 2:]
        elif kind == "half" and c["subpixel"]:
            a, b, _ = synth.make_pair(w, h, reach, seed, shift=shift, half=(1, -1), brightness=bright)
        else:
            a, b, _ = synth.make_pair(w, h, reach, seed, shift=shift, noise=3 if i == 7 else 1, brightness=bright)
        prevs.append(a)
        curs.append(b)
    return np.stack(prevs), np.stack(curs)


def delta_of(c, prev, cur):
    """The equalisation delta of a pair as cols_walk computes it from the pixel sums (0 at one level)."""
    if c["levels"] != 2:
        return 0
    npix = c["w"] * c["h"]
    return (int(prev.sum(dtype=np.uint64)) + npix // 2) // npix - (int(cur.sum(dtype=np.uint64)) + npix // 2) // npix
