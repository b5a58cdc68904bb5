"""The plan of a batch in plain Python: which kernels, with which arguments, serve one aof_flow_batch_device call
(csrc/aof_batch_plan.hpp: plan_batch, search_kind, choose_lane8) and the launch plan of the 16x16 search
(csrc/aof_tile16_plan.hpp: tile16_plan).  This file and aof_batch_plan.hpp are the two statements of the rule;
tests/test_host_asan.py holds them to each other field by field.  The models of the kernel families
(coarse_plan_ref, small_plan_ref, lane8_plan_ref, cols_plan_ref) ask here which family serves a case.

  call()         one call: parameters, pair count, stride, frame addresses, the context's switches
  plan()         plan_batch of it: kind per level, coarse kind, small / small_class, refine, sequence, k1_pass, the five
                 profiling counters, the 16x16 search's resolved prune flag
  tile16_plan()  tile16_plan of one search's arguments (t16())
  choose_lane8() the per-launch decision of a flat 8x8 launch and the adaptive state after it
"""
import coarse_plan_ref as coarse
import lane8_plan_ref as lane8
import selftest_rig as rig
import small_plan_ref as small
from tile16_probe_ref import K_SIDE, probe_samples, sample_strides

# csrc/aof_batch_plan.hpp
SMALL_MAX_PAIRS, PAYING_PCT, PROBE_EVERY = 128, 40, 16
SEARCH_KINDS = ("tile16", "lane8_group", "lane8", "generic")    # enum SearchKind
COARSE_KINDS = ("none", "fused", "k1")                          # enum CoarseKind
EXHAUSTIVE, PRUNED, ADAPTIVE = 0, 1, 2                          # AOF_SEARCH_*
CAPTURES = ("none", "active", "unknown")                        # enum Capture
# csrc/aof_tile16_plan.hpp, csrc/aof_engine_args.hpp
T16_THREADS, T16_LDS_LIMIT, T16_ATTR_ABOVE, FILL_THREADS, MAX_FORCED = 512, 156 * 1024, 64 * 1024, 256, 8
T16_VERDICTS = ("ok", "tile", "grid", "width", "stride", "prev", "cur", "frame", "lds")   # enum Tile16Verdict, in the order tested
FRONTS = ("none", "probe", "fill")                              # enum Tile16Front
BASE = small.BASE
CUS = coarse.CENSUS_CUS


# ---- one call ------------------------------------------------------------------------------------------------------------

def call(id, w, h, n_pairs, *, tile=8, search=4, px4=False, num_blocks=5, subpixel=0, levels=1, mean_subtract=0, mode=ADAPTIVE,
         force_generic=False, split=False, cus=CUS, stride=None, prev=BASE, cur=BASE + (1 << 32), k1_ready=False):
    """aof_params (px4: grid_mode), the call's n_pairs, pair_stride (default: a frame) and frame addresses, and what the
    context's switches say (search mode, aof_set_force_generic, aof_set_split_coarse, the device's CUs)."""
    return dict(id=id, w=w, h=h, n_pairs=n_pairs, tile=tile, search=search, px4=bool(px4), num_blocks=num_blocks, subpixel=int(bool(subpixel)),
                levels=levels, mean_subtract=int(bool(mean_subtract)), mode=mode, force_generic=bool(force_generic), split=bool(split), cus=cus,
                stride=w * h if stride is None else stride, prev=prev, cur=cur, k1_ready=bool(k1_ready))


def grid_of(c, level):
    return small.grid_for_level(c["w"], c["h"], level, c["px4"], c["subpixel"], c["tile"], c["search"], c["num_blocks"])


def params_valid(c):
    """aof_params_check."""
    if c["tile"] not in (8, 16) or not 1 <= c["search"] <= 8 or c["levels"] not in (1, 2) or (c["px4"] and c["num_blocks"] < 1):
        return False
    if c["w"] < 1 or c["h"] < 1 or c["w"] * c["h"] > 1 << 24 or (c["levels"] == 2 and (c["w"] | c["h"]) & 1):
        return False
    return all(grid_of(c, l) is not None for l in range(c["levels"]))


def search_args(c, level, g, prev, cur, stride):
    """SearchArgs of a level as plan_batch fills them (the fields the plans read)."""
    return dict(w=c["w"] >> level, h=c["h"] >> level, tile=c["tile"], search=c["search"], grid=g or (0,) * 6, subpixel=c["subpixel"],
                subdirs=c["subpixel"], n_pairs=c["n_pairs"], stride=stride, prev=prev, cur=cur, prune=c["mode"], level=level,
                rng=small.level_range(c["levels"], level, c["search"]), hints=int(c["tile"] == 16))


# ---- the 16x16 search --------------------------------------------------------------------------------------------------

def t16(id, w, h, n_pairs=4, *, subpixel=0, subdirs=None, prune=0, grid=None, tile=16, search=8, stride=None, prev=BASE, cur=BASE + (1 << 32),
        hints=1, forced=0):
    """The arguments of one 16x16 search (grid: the dense one of the frame unless given) and the test hook's verdict count."""
    m = 8 + (1 if subpixel else 0)
    g = grid if grid is not None else (m, m, 16, 16, (w - 2 * m) // 16, (h - 2 * m) // 16)
    return dict(id=id, w=w, h=h, tile=tile, search=search, grid=tuple(g), subpixel=int(bool(subpixel)),
                subdirs=int(bool(subpixel)) if subdirs is None else subdirs, n_pairs=n_pairs, stride=w * h if stride is None else stride,
                prev=prev, cur=cur, prune=prune, hints=hints, forced=forced)


def tile16_refines(a):
    return bool(a["subpixel"] and a["subdirs"])


def tile16_lds(a):
    nx = a["grid"][4]
    return 48 * a["w"] + 4 * nx + 16 + (2 * a["w"] + 32 if tile16_refines(a) else 0) + (4 * K_SIDE * nx + 16 if a["prune"] else 0)


def tile16_verdict(a):
    org = 1 if a["subpixel"] else 0
    g = a["grid"]
    tests = [("tile", a["tile"] != 16 or a["search"] != 8), ("grid", g[:4] != (8 + org, 8 + org, 16, 16)), ("width", a["w"] % 16 != 0),
             ("stride", a["stride"] % 16 != 0), ("prev", a["prev"] % 16 != 0), ("cur", a["cur"] % 16 != 0), ("frame", a["w"] * a["h"] > 0x7FFFFFFF),
             ("lds", tile16_lds(a) > T16_LDS_LIMIT)]
    return next((name for name, fails in tests if fails), "ok")


def tile16_plan(a, forced=None):
    """tile16_plan(a, forced_count)."""
    forced = a.get("forced", 0) if forced is None else forced
    nx, ny = a["grid"][4], a["grid"][5]
    lds, total = tile16_lds(a), a["n_pairs"] * ny
    pl = dict(verdict=tile16_verdict(a), refines=int(tile16_refines(a)), lds=lds, attr=int(lds > T16_ATTR_ABOVE), prune=int(bool(a["prune"])),
              refine=int(tile16_refines(a)), total=total, overflow=int(total > 0x7FFFFFFF), front="none", refused=int(total > 0x7FFFFFFF),
              front_wgs=0, stx=0, sty=0, sx=0, sy=0)
    if a["prune"] != 2 or pl["overflow"]:
        return pl
    if forced > 0:
        pl.update(front="fill", refused=int(not a["hints"] or forced > MAX_FORCED), front_wgs=-(-a["n_pairs"] // FILL_THREADS))
        return pl
    stx, sty = sample_strides(nx, ny)
    pl.update(front="probe", refused=int(not a["hints"]), front_wgs=a["n_pairs"], stx=stx, sty=sty, sx=probe_samples(nx, stx), sy=probe_samples(ny, sty))
    return pl


T16_FIELDS = ("verdict", "refines", "lds", "attr", "prune", "refine", "total", "overflow", "front", "refused", "front_wgs", "stx", "sty", "sx", "sy")


def _tile16_fields(pl):
    """The plan as the flat list of numbers the host self-test prints (T16_FIELDS)."""
    return [T16_VERDICTS.index(pl[k]) if k == "verdict" else FRONTS.index(pl[k]) if k == "front" else pl[k] for k in T16_FIELDS]


def _tile16_line(a):
    """The case as tests/native/host_selftest.cpp reads it: w h pair_stride prev cur tile search grid[6] subpixel subdirs prune
    hints n_pairs forced"""
    return rig.joined([a["w"], a["h"], a["stride"], a["prev"], a["cur"], a["tile"], a["search"], *a["grid"], a["subpixel"], a["subdirs"], a["prune"],
                       a["hints"], a["n_pairs"], a["forced"]])


def tile16_edge_width(prune=0, subpixel=0):
    """The last width (a multiple of 16) whose block row fits the 16x16 kernel's LDS, for the exhaustive or the pruned
    tables, without or with the refinement in the launch."""
    w = 32
    while tile16_verdict(t16("", w + 16, 48, subpixel=subpixel, prune=prune)) == "ok":
        w += 16
    return w


# ---- plan_batch ------------------------------------------------------------------------------------------------------------

def lane8_supported(a):
    nb = a["grid"][4] * a["grid"][5]
    return small.lane8_supported(a["w"], a["h"], nb, a["n_pairs"], a["stride"], a["tile"], a["search"])


def search_kind(c, a):
    """(kind, prune): the search kernel of one level and the 16x16 tile's resolved prune flag."""
    if c["force_generic"]:
        return "generic", a["prune"]
    if tile16_verdict(a) == "ok":
        return "tile16", a["prune"]
    if a["prune"] and tile16_verdict(dict(a, prune=0)) == "ok":   # (the pruned steps' tables may not fit LDS where the exhaustive tile does)
        return "tile16", 0
    if lane8_supported(a):
        grouped = small.group_plan(a["w"], a["h"], a["grid"], a["n_pairs"], a["stride"], a["rng"], a["tile"], a["search"])["ppw"] > 0
        return ("lane8_group" if grouped else "lane8"), a["prune"]
    return "generic", a["prune"]


def plan(c):
    """plan_batch.  valid: aof_params_check takes the parameters; where it does not, no context exists, and the plan is the
    function's answer with an empty grid (all zero) in place of each one the parameters do not have."""
    two, eq, n = c["levels"] == 2, bool(c["mean_subtract"]), c["n_pairs"]
    w, h = c["w"], c["h"]
    frame, l1_frame = w * h, (w // 2) * (h // 2)
    g0, g1 = grid_of(c, 0), grid_of(c, 1) if two else None
    a0 = search_args(c, 0, g0, c["prev"], c["cur"], c["stride"])
    sm1 = search_args(c, 1, g1, 0, 0, l1_frame)      # (the workspace's level-1 regions: 256-byte aligned)
    kind0, prune0 = search_kind(c, a0)
    pl = dict(valid=params_valid(c), small=False, small_class=False, coarse="none", k1_pass=False, sequence=False, kind=[kind0, None], prune=[prune0, 0],
              refine=[kind0 == "tile16" and bool(c["subpixel"]) and not tile16_refines(a0), False], a0=dict(a0, prune=prune0), g=(g0, g1))
    small_plan = small.small_plan(w, h, c["levels"], g0, g1, n, c["stride"], c["prev"], c["cur"], c["subpixel"], c["tile"], c["search"])
    pl["small_verdict"] = small_plan["verdict"]
    pl["small_l1_kind"] = search_kind(c, sm1)[0] if two else None
    pl["small_class"] = (not c["force_generic"] and not c["split"] and kind0 == "lane8_group" and (not two or pl["small_l1_kind"] == "lane8_group")
                         and small_plan["verdict"] == "ok")
    pl["small"] = pl["small_class"] and n <= SMALL_MAX_PAIRS
    if pl["small"] or (not two and not eq):
        return finish(c, pl)
    pl["coarse_verdict"] = coarse.coarse_verdict(w, h, c["stride"], c["prev"], c["cur"], g1 or (0,) * 6, c["search"], c["tile"], c["search"],
                                                 c["subpixel"], n)
    if two and not c["force_generic"] and not c["split"] and pl["coarse_verdict"] == "ok":
        pl["coarse"] = "fused"
        return finish(c, pl)
    pl["coarse"] = "k1"
    pl["sequence"] = c["cur"] - c["prev"] == frame and c["stride"] == frame
    pl["k1_pass"] = not (pl["sequence"] and c["k1_ready"])
    if two:
        a1 = dict(sm1, cur=l1_frame if pl["sequence"] else 0)
        pl["kind"][1], pl["prune"][1] = search_kind(c, a1)
        pl["refine"][1] = pl["kind"][1] == "tile16" and bool(c["subpixel"]) and not tile16_refines(a1)
    return finish(c, pl)


COUNTERS = ("K_PYRAMID", "K_SEARCH_L1", "K_REDUCE_L1", "K_SEARCH", "K_REDUCE")


def finish(c, pl):
    """The launches of the call by profiling counter, as the executor times the plan.  A flat 8x8 search may reduce in its
    own launch (choose_lane8 decides per launch): its K3 count is None here."""
    k3 = lambda kind: 0 if kind == "lane8_group" else None if kind == "lane8" else 1
    if pl["small"]:
        pl["counters"] = dict(zip(COUNTERS, (0, 0, 0, 1, 0)))
        return pl
    level1 = pl["coarse"] == "k1" and c["levels"] == 2
    pl["counters"] = dict(K_PYRAMID=int(pl["coarse"] == "fused") + int(pl["k1_pass"]), K_SEARCH_L1=int(level1),
                          K_REDUCE_L1=k3(pl["kind"][1]) if level1 else 0, K_SEARCH=1, K_REDUCE=k3(pl["kind"][0]))
    return pl


PLAN_FIELDS = ("valid", "small", "small_class", "coarse", "k1_pass", "sequence", "kind0", "refine0", "prune0", "kind1", "refine1", "prune1")


def _plan_fields(pl):
    """The plan as the flat list of numbers the host self-test prints (PLAN_FIELDS); level 1's are 0 where no level-1 search
    is planned (BatchPlan is zero there: SK_TILE16 is 0)."""
    k1 = pl["kind"][1]
    return [int(pl["valid"]), int(pl["small"]), int(pl["small_class"]), COARSE_KINDS.index(pl["coarse"]), int(pl["k1_pass"]), int(pl["sequence"]),
            SEARCH_KINDS.index(pl["kind"][0]), int(pl["refine"][0]), pl["prune"][0], SEARCH_KINDS.index(k1) if k1 else 0, int(pl["refine"][1]),
            pl["prune"][1] if k1 else 0]


def _call_line(c):
    """The call as tests/native/host_selftest.cpp reads it: w h tile search px4 num_blocks subpixel levels mean_subtract n_pairs
    pair_stride prev cur mode force_generic split cus k1_ready"""
    return rig.joined([c["w"], c["h"], c["tile"], c["search"], int(c["px4"]), c["num_blocks"], c["subpixel"], c["levels"], c["mean_subtract"], c["n_pairs"],
                       c["stride"], c["prev"], c["cur"], c["mode"], int(c["force_generic"]), int(c["split"]), c["cus"], int(c["k1_ready"])])


# ---- the cases of the family models as calls ----------------------------------------------------------------------------------

def of_coarse(c, cus=CUS):
    """A case of coarse_plan_ref's lists (case() or a PLAN_ONLY dict)."""
    a = coarse.plan_args(c, cus)
    return call("coarse:" + c["id"], a["w"], a["h"], a["n_pairs"], tile=a["tile"], search=a["search"], subpixel=a["subpixel"],
                levels=c.get("levels", 2), mean_subtract=a["sums"], split=c.get("split", False), cus=a["cus"], stride=a["pair_stride"],
                prev=a["prev"], cur=a["cur"])


def of_small(c, n_pairs=None, split=False):
    """A case of small_plan_ref's lists with a frame and a grid rule (case())."""
    stride, prev, cur = small.frame_layout(c)
    return call("small:" + c["id"], c["w"], c["h"], c["n_pairs"] if n_pairs is None else n_pairs, px4=c["px4"], subpixel=c["subpixel"],
                levels=c["levels"], mean_subtract=c["mean_subtract"], split=split, stride=stride, prev=prev, cur=cur)


LANE8_MODES = {"exhaustive": EXHAUSTIVE, "pruned": PRUNED, "adaptive-1": ADAPTIVE, "adaptive1": ADAPTIVE}


def of_lane8(c):
    """A case of lane8_plan_ref's lists: a device case as it stands, a plan case on the smallest dense frame of its nb."""
    if "kw" in c:
        kw = c["kw"]
        w, h = lane8.dense_frame(c["nb"])
        return call("lane8:" + c["id"], w, h, c["n_pairs"], mode=kw.get("prune", 0), tile=kw.get("tile", 8), search=kw.get("search", 4))
    return call("lane8:" + c["id"], c["w"], c["h"], c["n_pairs"], px4=c["grid"] == "px4", num_blocks=c["num_blocks"] or 5, subpixel=c["subpixel"],
                levels=c["levels"], mean_subtract=c["mean_subtract"], mode=LANE8_MODES[c["mode"]], stride=lane8.pair_stride(c))


def of_cols(c):
    """A case of cols_plan_ref's lists with a frame (case())."""
    return call("cols:" + c["id"], c["w"], c["h"], c["n_pairs"], subpixel=c["subpixel"], levels=c["levels"], mean_subtract=int(c["levels"] == 2),
                mode=PRUNED if c["mode"] == "pruned" else ADAPTIVE)


def union_cases():
    """Every case of the family models that names parameters: coarse and small lists whole, the flat 8x8 list but for the
    plan cases whose nb no frame of 2^24 pixels has."""
    cases = [of_coarse(c) for c in coarse.CPU_CASES + coarse.GPU_CASES + coarse.PLAN_ONLY]
    cases += [of_small(c) for c in small.CPU_CASES + small.GPU_CASES]
    cases += [of_small(c, 129) for c in small.GPU_CASES if c["over_128"]] + [of_small(c, split=True) for c in small.GPU_CASES[:4]]
    cases += [of_lane8(c) for c in lane8.CASES if "kw" not in c or 1 <= c["nb"] <= 5000]
    return cases


# the rule's own switches and edges, beyond what the family lists reach
OWN_CASES = [
    call("forced-generic-8x8", 64, 64, 9, force_generic=True), call("forced-generic-16x16", 160, 128, 9, tile=16, search=8, force_generic=True),
    call("forced-generic-two-levels", 128, 96, 9, levels=2, mean_subtract=1, force_generic=True),
    call("search-3-generic", 64, 64, 9, search=3), call("tile-16-search-4-generic", 160, 128, 9, tile=16, search=4),
    call("small-128", 64, 64, 128, mean_subtract=1), call("small-129", 64, 64, 129, mean_subtract=1),
    call("small-split", 64, 64, 9, levels=2, mean_subtract=1, split=True),
    call("one-level-no-sums", 640, 480, 9), call("one-level-sums-k1", 640, 480, 9, mean_subtract=1),
    call("sequence-view", 640, 480, 9, levels=2, mean_subtract=1, split=True, cur=BASE + 640 * 480),
    call("sequence-view-k1-ready", 640, 480, 9, levels=2, mean_subtract=1, split=True, cur=BASE + 640 * 480, k1_ready=True),
    call("sequence-view-fused-keeps-k1-off", 640, 480, 9, levels=2, mean_subtract=1, cur=BASE + 640 * 480, k1_ready=True),
    call("sequence-stride-off", 640, 480, 9, levels=2, mean_subtract=1, split=True, cur=BASE + 640 * 480, stride=640 * 480 + 16),
    call("16x16-vga", 640, 480, 9, tile=16, search=8), call("16x16-vga-half-pixel", 640, 480, 9, tile=16, search=8, subpixel=1),
    call("16x16-two-levels", 640, 480, 9, tile=16, search=8, levels=2, mean_subtract=1),
    call("16x16-two-levels-sequence-odd-l1-frame", 648, 488, 9, tile=16, search=8, levels=2, mean_subtract=1, cur=BASE + 648 * 488),
    call("16x16-px4", 640, 480, 9, tile=16, search=8, px4=True), call("16x16-exhaustive", 640, 480, 9, tile=16, search=8, mode=EXHAUSTIVE),
    call("16x16-pruned", 640, 480, 9, tile=16, search=8, mode=PRUNED),
    call("16x16-width-off", 648, 480, 9, tile=16, search=8), call("16x16-prev-off", 640, 480, 9, tile=16, search=8, prev=BASE + 8),
    call("16x16-cur-off", 640, 480, 9, tile=16, search=8, cur=BASE + (1 << 32) + 4), call("16x16-stride-off", 640, 480, 9, tile=16, search=8, stride=640 * 480 + 8),
    call("invalid-odd-two-levels", 641, 480, 9, levels=2), call("invalid-no-grid", 8, 8, 9), call("invalid-2^24-pixels", 4112, 4096, 9),
]


def edge_calls():
    """16x16 contexts at the widths where a block row stops fitting LDS: the exhaustive tile, the pruned tables (the plan
    then clears the prune flag and keeps the kernel), the refining forms."""
    out = []
    for sub in (0, 1):
        last0, last1 = tile16_edge_width(0, sub), tile16_edge_width(1, sub)
        assert last1 < last0
        for name, w in (("last-pruned", last1), ("first-pruned-over", last1 + 16), ("last-exhaustive", last0), ("first-over", last0 + 16)):
            for mode in (EXHAUSTIVE, PRUNED, ADAPTIVE):
                out.append(call(f"16x16-{name}-sub{sub}-mode{mode}", w, 48, 4, tile=16, search=8, subpixel=sub, mode=mode))
    return out


def batch_cases():
    return union_cases() + OWN_CASES + edge_calls()


# ---- the 16x16 plan's own cases --------------------------------------------------------------------------------------------

def tile16_cases():
    E0, P0, E1, P1 = (tile16_edge_width(p, s) for s in (0, 1) for p in (0, 1))
    assert 48 * E0 + 4 * ((E0 - 16) // 16) + 16 <= T16_LDS_LIMIT < 48 * (E0 + 16) + 4 * (E0 // 16) + 16
    # more than 128 samples at the first strides: 127 x 95 blocks -> 16 x 12 = 192 samples; the longer axis doubles first
    big = t16("2048x1536-strides-double", 2048, 1536, prune=2)
    pl = tile16_plan(big)
    assert probe_samples(127, 8) * probe_samples(95, 8) == 192 and (pl["stx"], pl["sty"]) == (16, 8) and pl["sx"] * pl["sy"] == 96
    cases = [big, t16("4096x4096-both-double", 4096, 4096, prune=2), t16("nx-1", 32, 160, prune=2), t16("ny-1", 160, 32, prune=2),
             t16("one-block", 32, 32, prune=2)]
    for k in (1, 3, 4, 7, 8, 9):
        cases += [t16(f"nx-{k}-blocks", 16 * k + 16, 16 * 5 + 16, prune=2), t16(f"ny-{k}-blocks", 16 * 5 + 16, 16 * k + 16, prune=2),
                  t16(f"{k}x{k}-blocks-half-pixel", 16 * k + 32, 16 * k + 32, subpixel=1, prune=2)]
    for name, w, prune, sub in (("exhaustive", E0, 0, 0), ("pruned", P0, 1, 0), ("adaptive", P0, 2, 0), ("exhaustive-refining", E1, 0, 1),
                                ("pruned-refining", P1, 1, 1)):
        cases += [t16(f"last-{name}-{w}", w, 48, subpixel=sub, prune=prune), t16(f"first-over-{name}-{w + 16}", w + 16, 48, subpixel=sub, prune=prune)]
    cases += [t16("pruned-over-exhaustive-fits", P0 + 16, 48, prune=1), t16("pruned-over-exhaustive-fits-0", P0 + 16, 48, prune=0),
              t16("half-pixel-k2b-behind", 160, 128, subpixel=1, subdirs=0, prune=2),
              t16("width-off-16", 168, 128), t16("prev-off", 160, 128, prev=BASE + 4), t16("cur-off", 160, 128, cur=BASE + (1 << 32) + 8),
              t16("stride-off", 160, 128, stride=160 * 128 + 8), t16("tile-8", 160, 128, tile=8, search=4), t16("search-4", 160, 128, search=4),
              t16("sparse-px4-grid", 640, 480, grid=(9, 9, 77, 56, 8, 9), prune=2), t16("grid-origin-off", 160, 128, grid=(9, 8, 16, 16, 9, 7)),
              t16("frame-2^31", 65536, 32768), t16("frame-2^31-less", 65520, 32768),
              t16("total-2^31-1", 64, 48, n_pairs=(1 << 30) - 1, grid=(8, 8, 16, 16, 3, 2), prune=2),
              t16("total-just-under", 64, 32, n_pairs=0x7FFFFFFF, prune=2), t16("total-2^31", 64, 48, n_pairs=1 << 30, prune=2),
              t16("total-2^31-exhaustive", 64, 48, n_pairs=1 << 30), t16("no-hints-probe", 160, 128, prune=2, hints=0),
              t16("no-hints-pruned", 160, 128, prune=1, hints=0)]
    cases += [t16(f"forced-{k}", 160, 128, n_pairs=257, prune=2, forced=k) for k in (0, 1, 8, 9)]
    cases += [t16("forced-no-hints", 160, 128, prune=2, forced=3, hints=0), t16("forced-not-adaptive", 160, 128, prune=1, forced=3)]
    return cases


# ---- flat 8x8 launches: choose_lane8 ----------------------------------------------------------------------------------------

def fresh_state(belief=-1, since_probe=0, launch_no=0, slots=True):
    return dict(slots=bool(slots), launch_no=launch_no, expected=0, words=[], belief=belief, since_probe=since_probe,
                stats=dict(pruned_launches=0, exhaustive_launches=0, reports_read=0, belief=belief, paying_pct=0))


def report(st, expected, arrived, paying, seen):
    """The previous launch's report as the host finds it: `expected` words, the first `arrived` of them carrying the
    launch's tag with `paying` of `seen` chunks each, the rest stale."""
    tag = st["launch_no"] & 0xFFFF
    st["expected"] = expected
    st["words"] = [(tag << 16 | paying << 8 | seen) if i < arrived else ((tag ^ 1) << 16 | 0xFFFF) for i in range(expected)]
    return st


def adaptive_lane8_prunes(st, a):
    nb = a["grid"][4] * a["grid"][5]
    if a["level"] != 0 or not st["slots"] or -(-a["n_pairs"] * nb // lane8.THREADS) < lane8.PRUNE_MIN_CHUNKS or nb < 1 or a["n_pairs"] < 1:
        return False
    if st["expected"]:
        tag = st["launch_no"] & 0xFFFF
        mine = [w for w in st["words"][:lane8.PRUNE_SLOTS] if w >> 16 == tag]
        paying, seen = sum(w >> 8 & 0xFF for w in mine), sum(w & 0xFF for w in mine)
        if len(mine) * 4 >= st["expected"] and seen:
            st["belief"] = int(paying * 100 >= seen * PAYING_PCT)
            st["stats"].update(paying_pct=paying * 100 // seen, belief=st["belief"], reports_read=st["stats"]["reports_read"] + 1)
    if st["belief"] != 0:
        return True
    st["since_probe"] += 1
    if st["since_probe"] >= PROBE_EVERY:
        st["since_probe"] = 0
        return True
    return False


def cols_supported(a):
    g = a["grid"]
    return lane8_supported(a) and g[3] == 8 and g[4] >= 16 and g[5] >= 2 and g[4] * g[5] > 256


def choose_lane8(mode, st, a, capture="none", votes=(1, 1, lane8.VOTE_STRIDE), vote_pairs=lane8.VOTE_PAIRS, separate=False, captured=False):
    """choose_lane8: dict(prune, cols, fused, reports, tag) of this launch; `st` is changed as the context's state is.
    a: search_args() of the launch, a['prune'] the context's mode; votes: (memory, fault word, words per record)."""
    l = dict(prune=a["prune"], cols=False, fused=False, reports=False, tag=0)
    if l["prune"] and mode == ADAPTIVE:
        if not adaptive_lane8_prunes(st, a):
            l["prune"] = 0
            st["stats"]["exhaustive_launches"] += 1
        else:
            l["prune"] = 1 if st["belief"] == 1 else 2
            st["launch_no"] = (st["launch_no"] + 1) & 0xFFFFFFFF
            if st["launch_no"] % 0x10000 == 0:
                st["launch_no"] += 1
            l.update(reports=st["slots"], tag=st["launch_no"] & 0xFFFF)
            st["stats"]["pruned_launches"] += 1
    x = dict(a, prune=l["prune"])
    nb, n = x["grid"][4] * x["grid"][5], 2 * (2 * x["rng"] + 1) + 1
    mem, fault, stride = votes
    l["cols"] = bool(l["prune"]) and cols_supported(x)
    if l["cols"]:
        fits = bool(mem and fault and n <= 62 and stride >= 2 + 2 * n and x["n_pairs"] <= vote_pairs)
    else:
        fits = not l["prune"] and lane8.flat_plan(nb, x["n_pairs"], x["stride"], x["w"], x["h"], 0, False, x["rng"], votes, vote_pairs)["votes"] == "ok"
    l["fused"] = fits and not separate and (capture == "active" or (capture == "none" and not captured))
    return l


def lane8_args(c):
    """The level-0 search arguments of a call whose level 0 is a flat 8x8 launch."""
    pl = plan(c)
    assert pl["valid"] and pl["kind"][0] == "lane8", c["id"]
    return pl["a0"]


def lane8_prune(c, belief):
    """SearchArgs.prune of the level-0 launch of a fresh context told `belief`."""
    return choose_lane8(c["mode"], fresh_state(belief), lane8_args(c))["prune"]


# the table of the self-test: geometry x mode x belief x since_probe x report x capture x captured x separate
CHOOSE_GEOMETRIES = (("vga-1024-column-walk", 640, 480, 1024, False, 1), ("vga-64-too-small-to-prune", 640, 480, 64, False, 1),
                     ("px4-289-chunk-walk", *lane8.px4_frame(289)[:2], 2722, True, 1), ("vga-4096-over-the-vote-capacity", 640, 480, 4096, False, 1),
                     ("vga-two-levels-55-bins", 640, 480, 1024, False, 2))
REPORTS = (("none", 0, 0, 0, 0), ("under-a-quarter", 8, 1, 100, 100), ("a-quarter", 8, 2, 39, 100), ("a-quarter-paying", 8, 2, 40, 100),
           ("all-39-pct", 8, 8, 39, 100), ("all-40-pct", 8, 8, 40, 100), ("arrived-nothing-seen", 8, 8, 0, 0))


def choose_rows():
    rows = []
    for gname, w, h, n, px4, levels in CHOOSE_GEOMETRIES:
        for mode in (EXHAUSTIVE, PRUNED, ADAPTIVE):
            for belief in (-1, 0, 1):
                for since in (PROBE_EVERY - 2, PROBE_EVERY - 1):
                    for rep in REPORTS:
                        for capture in CAPTURES:
                            for captured, separate in ((0, 0), (1, 0), (0, 1)):
                                if mode != ADAPTIVE and (rep[0] != "none" or since != PROBE_EVERY - 2 or belief != -1):
                                    continue   # (the fixed modes read no state)
                                rows.append(dict(id=f"{gname}/mode{mode}/belief{belief}/since{since}/{rep[0]}/{capture}/{captured}{separate}", w=w, h=h,
                                                 n_pairs=n, px4=px4, num_blocks=lane8.px4_frame(289)[2] if px4 else 5, levels=levels, mode=mode,
                                                 belief=belief, since=since, launch_no=7, report=rep[1:], capture=capture, captured=captured,
                                                 separate=separate, votes=(1, 1, lane8.VOTE_STRIDE)))
    base = dict(rows[0], mode=ADAPTIVE, belief=1, since=0, report=(0, 0, 0, 0), capture="none", captured=0, separate=0, w=640, h=480, n_pairs=1024,
                px4=False, num_blocks=5, levels=1)
    rows += [dict(base, id="tag-wraps-past-0", launch_no=0xFFFF), dict(base, id="tag-wraps-past-0-at-2^32", launch_no=0xFFFFFFFF),
             dict(base, id="no-vote-memory", votes=(0, 1, lane8.VOTE_STRIDE)), dict(base, id="no-fault-word", votes=(1, 0, lane8.VOTE_STRIDE)),
             dict(base, id="vote-stride-short", votes=(1, 1, 39)), dict(base, id="vote-stride-just", votes=(1, 1, 40)),
             dict(base, id="300-slots-expected", report=(300, 300, 40, 100)), dict(base, id="300-slots-expected-64-arrived", report=(300, 64, 40, 100))]
    return rows


def choose_call(r):
    return call(r["id"], r["w"], r["h"], r["n_pairs"], px4=r["px4"], num_blocks=r["num_blocks"], levels=r["levels"],
                mean_subtract=int(r["levels"] == 2), mode=r["mode"], split=True)


def choose_row(r):
    """The row's launch and the state after it, as the flat list the self-test prints (CHOOSE_FIELDS)."""
    st = report(fresh_state(r["belief"], r["since"], r["launch_no"]), *r["report"])
    l = choose_lane8(r["mode"], st, lane8_args(choose_call(r)), r["capture"], r["votes"], lane8.VOTE_PAIRS, bool(r["separate"]), bool(r["captured"]))
    s = st["stats"]
    return [l["prune"], int(l["cols"]), int(l["fused"]), int(l["reports"]), l["tag"], st["belief"], st["since_probe"], st["launch_no"],
            s["pruned_launches"], s["exhaustive_launches"], s["reports_read"], s["belief"], s["paying_pct"]]


CHOOSE_FIELDS = ("prune", "cols", "fused", "reports", "tag", "belief", "since_probe", "launch_no", "pruned_launches", "exhaustive_launches",
                 "reports_read", "stats.belief", "stats.paying_pct")


def _choose_line(r):
    """The row as tests/native/host_selftest.cpp reads it: the call's line, then belief since_probe launch_no expected arrived
    paying seen capture captured separate votes_memory votes_fault votes_stride"""
    v = [r["belief"], r["since"], r["launch_no"], *r["report"], CAPTURES.index(r["capture"]), r["captured"], r["separate"], *r["votes"]]
    return _call_line(choose_call(r)) + " " + rig.joined(v)


def selftest_families():
    """plan_batch == plan(), tile16_plan == tile16_plan() and choose_lane8 == choose_row(), on every case of every list."""
    return [rig.family("batch-plan", "batch plan: ", batch_cases(), _call_line, lambda c: _plan_fields(plan(c)), PLAN_FIELDS),
            rig.family("tile16-plan", "tile16 plan: ", tile16_cases(), _tile16_line, lambda c: _tile16_fields(tile16_plan(c)), T16_FIELDS),
            rig.family("choose-lane8", "choose lane8: ", choose_rows(), _choose_line, choose_row, CHOOSE_FIELDS, summary="choose lane8: {} rows printed")]
