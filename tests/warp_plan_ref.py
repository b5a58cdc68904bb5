"""The launch plans of the two lens kernels in plain Python -- the warp launch k_bank_warp (csrc/aof_warp_plan.hpp:
warp_plan_make, behind aof_ingest_warped_device and the composed bank push) and the one-launch tick with the warp inside it,
k_bank_tick_warped (csrc/aof_small_plan.hpp: small_warp_plan_make) --, what the kernels make of them lane by lane, the names
of the paths a launch can take through them, and the case lists of tests/test_warp_plan_ref.py, tests/test_host_asan.py (the
warp launch plan from the C++ function), tests/test_bank_warp_ref.py (the numpy warp model against the host build at the cases'
sizes), tests/test_gpu_bank_warp.py (WARP_CASES on the device) and tests/test_gpu_bank_warp_tick_plan.py (TICK_CASES).

Written from the header text and the kernels' comments:

  k_bank_warp   256 lanes, a workgroup per (frame, strip).  A strip has 128 crop rows, halved while the nodes it clamps into
                LDS -- rows / 8 + 1 node rows of nx nodes of 8 bytes -- are more than 32 KiB; a crop whose 8-row strip still
                needs more than 60 KiB is refused.  The node loop walks node_rows * nx nodes 256 at a time.  W % 16 == 0 and
                a 16-byte aligned destination: an item is 16 pixels of a row, item = row * (W / 16) + piece, 256 items a
                trip; a lane counts its pixels in 12-bit fields and the wave flushes them after the loop (and inside it
                every 255 trips, which no served shape reaches: test_the_mid_loop_flush_is_unreachable).  Else a lane per
                pixel.  One strip: the workgroup stores the frame's histogram; several: they add to words zeroed first.
  k_bank_tick_warped   one workgroup per stream.  nx * ny nodes behind the small plan's dynamic LDS, clamped 256 at a time;
                H * W / 16 items of 16 pixels, 256 a trip, into LDS buffer 1; then flow_small_pair as ever.  When plan plus
                nodes do not fit LDS the push falls back to the composed launches.

No size is asserted here as a literal beyond what the case tables state: a case names a shape and the properties it is
there for, and reach() derives every property from the plan."""
import selftest_rig as rig
import small_plan_ref as small

# csrc/aof_warp_plan.hpp, csrc/aof_warp_step.hpp
THREADS, CELL, POINT_BYTES = 256, 8, 8
STRIP_ROWS, NODE_BYTES_WANTED, NODE_BYTES_MAX, LANE_ITEMS = 128, 32768, 61440, 255
ATTR_ABOVE = small.ATTR_ABOVE
MASK = 128
VERDICTS = ("ok", "too_wide", "too_many")
BASE = 0x7F0000000000   # a destination address for the plans: 16-byte aligned


def nodes(size):
    """Nodes along an axis of `size` crop pixels."""
    return (size + 7) // 8 + 1


def trips(items, per=THREADS):
    return 0 if items <= 0 else -(-items // per)


def node_bytes(rows, nx):
    """The launcher's estimate for a strip of `rows` rows (a multiple of the cell)."""
    return (rows // CELL + 1) * nx * POINT_BYTES


def strip_rows_of(w):
    """The strip the halving arrives at for a crop of width w."""
    nx, rows = nodes(w), STRIP_ROWS
    while rows > CELL and node_bytes(rows, nx) > NODE_BYTES_WANTED:
        rows //= 2
    return rows


def mask(w, h):
    """(x0, y0, x1, y1) of the exposure mask: the centred 128 x 128 region, clipped to the crop."""
    x0, y0 = w // 2 - MASK // 2, h // 2 - MASK // 2
    return max(x0, 0), max(y0, 0), min(x0 + MASK, w), min(y0 + MASK, h)


# ---- the warp launch ---------------------------------------------------------------------------------------------------

def warp_plan(w, h, n_frames=1, cropped=BASE, cropped_stride=None, hist=1):
    """warp_plan_make.  cropped: the destination's address (0: none); cropped_stride: bytes between crops (default: dense)."""
    cropped_stride = w * h if cropped_stride is None else cropped_stride
    nx, ny = nodes(w), nodes(h)
    strip = strip_rows_of(w)
    nstrips = -(-h // strip)
    rows = (min(h, strip), h - (nstrips - 1) * strip)
    vec = int(w % 16 == 0 and (not cropped or (cropped % 16 == 0 and cropped_stride % 16 == 0)))
    node_rows = tuple((r - 1) // CELL + 2 for r in rows)
    items = tuple(r * (w // 16) if vec else r * w for r in rows)
    lds = node_rows[0] * nx * POINT_BYTES
    wgs = n_frames * nstrips
    verdict = "too_wide" if node_bytes(strip, nx) > NODE_BYTES_MAX else "too_many" if wgs > 0x7FFFFFFF else "ok"
    return dict(w=w, h=h, verdict=verdict, nx=nx, ny=ny, strip_rows=strip, nstrips=nstrips, rows=rows, node_rows=node_rows,
                node_bytes=tuple(n * nx * POINT_BYTES for n in node_rows), vec=vec, lds=lds, attr=int(lds > ATTR_ABOVE),
                zero_hist=int(bool(hist) and nstrips > 1), items=items, trips=tuple(trips(i) for i in items), wgs=wgs)


WARP_FIELDS = ("verdict", "nx", "ny", "strip_rows", "nstrips", "rows[0]", "rows[1]", "node_rows[0]", "node_rows[1]", "node_bytes[0]",
               "node_bytes[1]", "vec", "lds", "attr", "zero_hist", "items[0]", "items[1]", "trips[0]", "trips[1]", "wgs")


def _warp_fields(pl):
    """The plan as the flat list of numbers the host self-test prints for warp_plan_make (WARP_FIELDS)."""
    return [VERDICTS.index(pl["verdict"]), pl["nx"], pl["ny"], pl["strip_rows"], pl["nstrips"], *pl["rows"], *pl["node_rows"], *pl["node_bytes"],
            pl["vec"], pl["lds"], pl["attr"], pl["zero_hist"], *pl["items"], *pl["trips"], pl["wgs"]]


def warp_case(id, w, h, *tags, skew=0, plane=None, wide=False, n_frames=None):
    """A w x h crop out of a plane of crop + (32, 16) (plane: another size); skew: the destination starts that many bytes
    off a 16-byte boundary; wide: grey8 and one grouped format, three designs (else every format and design of the test)."""
    return dict(id=id, w=w, h=h, tags=tags, skew=skew, plane=plane or (w + 32, h + 16), wide=wide, n_frames=n_frames)


WIDE_DESIGNS = ("barrel", "far-outside", "smooth-random")
ALL_DESIGNS = 10   # bank_warp_ref.designs


def case_frames(c):
    """The frames of a case's one launch: its designs, one unwarped and one refused frame."""
    return c["n_frames"] or (len(WIDE_DESIGNS) if c["wide"] else ALL_DESIGNS) + 2


def case_warp_plan(c, hist=1):
    return warp_plan(c["w"], c["h"], case_frames(c), BASE + c["skew"], None, hist)


def width_limit():
    """The first width (a multiple of 16) the launch refuses."""
    w = 16
    while warp_plan(w, 8)["verdict"] == "ok":
        w += 16
    return w


def warp_reach(c):
    """The names of the paths the case's launch takes (WARP_VOCABULARY)."""
    pl = case_warp_plan(c)
    w, h = c["w"], c["h"]
    if pl["verdict"] != "ok":
        return {"w_" + pl["verdict"]} | ({"w_first_width_refused"} if warp_plan(w - 16, h)["verdict"] == "ok" else set())
    x0, y0, x1, y1 = mask(w, h)
    vec, two = bool(pl["vec"]), pl["nstrips"] > 1
    last = pl["items"][1] if two else pl["items"][0]
    got = {name for name, hit in (
        ("w_vector", vec), ("w_per_pixel_by_width", not vec and w % 16 != 0), ("w_per_pixel_by_alignment", not vec and w % 16 == 0),
        ("w_items_one_trip", vec and max(pl["trips"]) == 1),
        ("w_items_partial_last_trip", vec and pl["trips"][0] >= 2 and pl["items"][0] % THREADS != 0),
        ("w_second_trip_partial", vec and pl["trips"][0] == 2 and pl["items"][0] % THREADS != 0),
        ("w_items_full_trips", vec and pl["trips"][0] >= 2 and pl["items"][0] % THREADS == 0),
        ("w_nodes_two_trips", pl["node_rows"][0] * pl["nx"] > THREADS),
        ("w_nodes_second_trip_partial_one_strip", not two and THREADS < pl["node_rows"][0] * pl["nx"] < 2 * THREADS),
        ("w_last_cell_row_partial", h % CELL != 0),
        ("w_two_strips", two), ("w_last_strip_short", two and pl["rows"][1] < pl["rows"][0]),
        ("w_last_strip_under_a_trip", two and vec and last < THREADS),
        ("w_vector_two_strips", vec and two), ("w_per_pixel_two_strips", not vec and two),
        ("w_histogram_zeroed_first", bool(pl["zero_hist"])), ("w_histogram_stored_by_its_owner", not pl["zero_hist"]),
        ("w_mask_x_inside_an_item", vec and (x0 % 16 != 0 or x1 % 16 != 0)), ("w_mask_rows_off_the_crop_edge", y0 > 0 and y1 < h),
        ("w_mask_cuts_items_and_rows", vec and x0 % 16 != 0 and x1 % 16 != 0 and y0 > 0 and y1 < h), ("w_mask_is_the_crop", (x0, y0, x1, y1) == (0, 0, w, h)),
        ("w_strip_halved", pl["strip_rows"] < STRIP_ROWS), ("w_first_width_halved", pl["strip_rows"] == STRIP_ROWS // 2 and strip_rows_of(w - 16) == STRIP_ROWS),
        ("w_strip_of_one_cell", pl["strip_rows"] == CELL),
        ("w_lds_over_48k", pl["attr"] == 1), ("w_first_width_over_48k", pl["attr"] == 1 and warp_plan(w - 16, h)["attr"] == 0),
        ("w_last_width_served", warp_plan(w + 16, h)["verdict"] == "too_wide"),
    ) if hit}
    return got


WARP_VOCABULARY = [
    "w_vector", "w_per_pixel_by_width", "w_per_pixel_by_alignment", "w_items_one_trip", "w_items_partial_last_trip", "w_second_trip_partial", "w_items_full_trips",
    "w_nodes_two_trips", "w_nodes_second_trip_partial_one_strip", "w_last_cell_row_partial", "w_two_strips", "w_last_strip_short", "w_last_strip_under_a_trip", "w_vector_two_strips",
    "w_per_pixel_two_strips", "w_histogram_zeroed_first", "w_histogram_stored_by_its_owner", "w_mask_x_inside_an_item", "w_mask_rows_off_the_crop_edge",
    "w_mask_cuts_items_and_rows", "w_mask_is_the_crop", "w_strip_halved", "w_first_width_halved", "w_strip_of_one_cell", "w_lds_over_48k", "w_first_width_over_48k",
    "w_last_width_served", "w_too_wide", "w_first_width_refused"]
# no launch ends on it: aof_ingest_warped_device refuses n_frames * ((h + 7) / 8) beyond 31 bits first, the bank has S streams
UNREACHABLE_WARP_VERDICTS = {"too_many": "2^31 workgroups: more frames than the cases' device bytes"}

WARP_CASES = [
    # ---- the sizes the kernel arrived with
    warp_case("vector-64x64", 64, 64, "w_vector", "w_items_one_trip", "w_histogram_stored_by_its_owner", "w_mask_is_the_crop", plane=(96, 80)),
    warp_case("per-pixel-20x12", 20, 12, "w_per_pixel_by_width", plane=(44, 36)),
    warp_case("two-strips-16x136", 16, 136, "w_vector_two_strips", "w_last_strip_under_a_trip", plane=(40, 150)),
    # ---- the edges of the plan
    warp_case("vector-partial-trips", 80, 76, "w_items_partial_last_trip", "w_second_trip_partial", "w_last_cell_row_partial"),
    warp_case("vector-node-trips", 128, 128, "w_nodes_two_trips", "w_nodes_second_trip_partial_one_strip", "w_items_full_trips"),
    warp_case("vector-mask-inside-an-item", 144, 136, "w_mask_x_inside_an_item", "w_mask_rows_off_the_crop_edge", "w_mask_cuts_items_and_rows", "w_two_strips", "w_last_strip_short"),
    warp_case("per-pixel-two-strips", 20, 136, "w_per_pixel_two_strips", "w_histogram_zeroed_first"),
    warp_case("per-pixel-by-alignment", 64, 64, "w_per_pixel_by_alignment", skew=3),
    warp_case("strip-halved", 1920, 72, "w_strip_halved", "w_first_width_halved", wide=True),
    warp_case("nodes-over-48k", 24576, 8, "w_lds_over_48k", "w_first_width_over_48k", "w_strip_of_one_cell", wide=True),
    warp_case("nodes-at-the-limit", 30704, 8, "w_last_width_served", "w_lds_over_48k", wide=True),
    warp_case("too-wide", 30720, 8, "w_too_wide", "w_first_width_refused", wide=True),
]

# the plan alone, against the C++ function
WARP_PLAN_ONLY = [
    dict(id="1x1", w=1, h=1), dict(id="8x8", w=8, h=8), dict(id="9x9", w=9, h=9), dict(id="16x128", w=16, h=128), dict(id="16x129", w=16, h=129),
    dict(id="1904x72-not-halved", w=1904, h=72), dict(id="1912x128-per-pixel-halved", w=1912, h=128), dict(id="3840x2160", w=3840, h=2160),
    dict(id="24560x8-under-48k", w=24560, h=8), dict(id="24576x9-two-strips", w=24576, h=9), dict(id="30712x8-per-pixel-limit", w=30712, h=8),
    dict(id="30713x8-refused", w=30713, h=8), dict(id="65536x4096", w=65536, h=4096), dict(id="no-destination", w=64, h=64, cropped=0),
    dict(id="no-destination-odd-width", w=63, h=64, cropped=0), dict(id="stride-off-16", w=64, h=64, cropped_stride=4100, n_frames=2),
    dict(id="destination-off-8", w=64, h=64, cropped=BASE + 8), dict(id="no-histogram-two-strips", w=16, h=136, hist=0),
    dict(id="too-many", w=16, h=1 << 20, n_frames=1 << 18), dict(id="most-workgroups", w=16, h=128, n_frames=0x7FFFFFFF),
    dict(id="too-wide-before-too-many", w=30720, h=1 << 20, n_frames=1 << 18),
]


def _warp_plan_args(c):
    if "tags" in c:
        return dict(w=c["w"], h=c["h"], n_frames=case_frames(c), cropped=BASE + c["skew"], cropped_stride=c["w"] * c["h"], hist=1)
    return dict(w=c["w"], h=c["h"], n_frames=c.get("n_frames", 1), cropped=c.get("cropped", BASE), cropped_stride=c.get("cropped_stride", c["w"] * c["h"]),
                hist=c.get("hist", 1))


def selftest_plan(c):
    """The warp launch plan of a case of WARP_CASES or WARP_PLAN_ONLY."""
    return warp_plan(**_warp_plan_args(c))


def selftest_families():
    """warp_plan_make == warp_plan(), on every case of both lists.  The case as tests/native/host_selftest.cpp reads it: w h
    n_frames cropped cropped_stride hist"""
    def line(c):
        a = _warp_plan_args(c)
        return rig.joined(a[k] for k in ("w", "h", "n_frames", "cropped", "cropped_stride", "hist"))

    return [rig.family("warp-plan", "warp plan: ", WARP_CASES + WARP_PLAN_ONLY, line, lambda c: _warp_fields(selftest_plan(c)), WARP_FIELDS)]


# ---- what the warp kernel's lanes do --------------------------------------------------------------------------------------

def vector_items(pl, strip):
    """Every live (trip, lane) of the vector path of a strip: lists trip, lane, y, x (the item's row and first pixel)."""
    w = pl["w"]
    pieces = w // 16
    row_begin = strip * pl["strip_rows"]
    row_end = min(pl["h"], row_begin + pl["strip_rows"])
    items = (row_end - row_begin) * pieces
    out = []
    for base in range(0, items, THREADS):
        for lane in range(THREADS):
            it = base + lane
            if it < items:
                out.append((base // THREADS, lane, row_begin + it // pieces, (it % pieces) * 16))
    return out, items


# ---- the one-launch warped tick ------------------------------------------------------------------------------------------

def tick_plan(w, h, levels):
    """small_warp_plan_make on the configuration's small plan, and the kernel's loops."""
    plain = small.small_lds(w, h, levels)
    nx, ny = nodes(w), nodes(h)
    lds = plain + POINT_BYTES * nx * ny
    items = h * (w // 16)
    t = trips(items)
    return dict(w=w, h=h, levels=levels, nx=nx, ny=ny, plain=plain, plain_fits=plain + small.STATIC_LDS <= small.LDS_LIMIT, nodes_at=plain, lds=lds,
                attr=int(lds > ATTR_ABOVE), plain_attr=int(plain > ATTR_ABOVE), fits=lds + small.STATIC_LDS <= small.LDS_LIMIT,
                spare=small.LDS_LIMIT - small.STATIC_LDS - lds, items=items, trips=t, last_live=items - (t - 1) * THREADS if t else 0,
                node_trips=trips(nx * ny), l1_items=(h // 2) * (w // 16) if levels == 2 else 0)


def tick_case(id, w, h, *tags, levels=1, mean_subtract=0, subpixel=(1,), S=5, T=6, formats=(), burst=False, unbound_first=False):
    """A bank of S streams of w x h crops out of planes of crop + (32, 16), T ticks under path 1.  subpixel: the values the
    case runs at; formats: pixel formats it also runs at (names of crop_source_ref); burst: one burst of K = 3 follows the
    ticks; unbound_first: an engine with nothing bound ticks first in the same process."""
    return dict(id=id, w=w, h=h, tags=tags, levels=levels, mean_subtract=mean_subtract, subpixel=tuple(subpixel), S=S, T=T, formats=tuple(formats),
                burst=burst, unbound_first=unbound_first)


def case_tick_plan(c):
    return tick_plan(c["w"], c["h"], c["levels"])


def tick_small_plan(c, subpixel=1):
    """The one-workgroup plan of the case on the published sparse grid (5 x 5 blocks a level)."""
    g0 = small.grid_for_level(c["w"], c["h"], 0, True, subpixel)
    g1 = small.grid_for_level(c["w"], c["h"], 1, True, subpixel) if c["levels"] == 2 else None
    return small.small_plan(c["w"], c["h"], c["levels"], g0, g1, c["S"], c["w"] * c["h"], small.BASE, small.BASE + (1 << 32), subpixel)


def tick_path(c):
    """aof_bank_last_path of a camera push with warps bound under aof_set_bank_path(1)."""
    return 1 if tick_small_plan(c)["verdict"] == "ok" and case_tick_plan(c)["fits"] else 2


def tick_reach(c):
    """The names of the paths the case's launches take (TICK_VOCABULARY)."""
    pl = case_tick_plan(c)
    w, h, two = c["w"], c["h"], c["levels"] == 2
    assert tick_small_plan(c)["verdict"] in ("ok",), "every tick case is of the one-workgroup class"
    if tick_path(c) == 2:
        return {"t_fallback_nodes_do_not_fit"} | ({"t_fallback_one_row_over"} if tick_plan(w, h - 1, c["levels"])["fits"] else set())
    x0, y0, x1, y1 = mask(w, h)
    return {name for name, hit in (
        ("t_one_launch", True),
        ("t_items_one_full_trip", pl["items"] == THREADS), ("t_idle_waves", pl["items"] <= THREADS - 64),
        ("t_items_partial_last_trip", pl["trips"] >= 2 and pl["last_live"] < THREADS), ("t_items_full_trips", pl["trips"] >= 2 and pl["last_live"] == THREADS),
        ("t_nodes_under_a_trip", pl["nx"] * pl["ny"] < THREADS), ("t_nodes_two_trips", pl["node_trips"] >= 2),
        ("t_last_cell_row_partial", h % CELL != 0), ("t_odd_height", h % 2 == 1),
        ("t_two_levels", two), ("t_level_1_partial_last_trip", two and pl["l1_items"] % THREADS != 0), ("t_mean_subtract", bool(c["mean_subtract"])),
        ("t_half_pixel", 1 in c["subpixel"]), ("t_integer", 0 in c["subpixel"]), ("t_other_formats", bool(c["formats"])), ("t_burst", c["burst"]),
        ("t_attr_not_set", pl["attr"] == 0), ("t_attr_set", pl["attr"] == 1), ("t_attr_set_by_the_nodes", pl["attr"] == 1 and pl["plain_attr"] == 0),
        ("t_attr_unwarped_tick_first", pl["attr"] == 1 and pl["plain_attr"] == 0 and c["unbound_first"]),
        ("t_mask_off_zero", x0 > 0 and y0 > 0), ("t_mask_x_inside_an_item", x0 % 16 != 0), ("t_mask_is_the_crop", (x0, y0, x1, y1) == (0, 0, w, h)),
        ("t_last_row_that_fits", not tick_plan(w, h + 1, c["levels"])["fits"]),
    ) if hit}


TICK_VOCABULARY = [
    "t_one_launch", "t_items_one_full_trip", "t_idle_waves", "t_items_partial_last_trip", "t_items_full_trips", "t_nodes_under_a_trip", "t_nodes_two_trips",
    "t_last_cell_row_partial", "t_odd_height", "t_two_levels", "t_level_1_partial_last_trip", "t_mean_subtract", "t_half_pixel", "t_integer",
    "t_other_formats", "t_burst", "t_attr_not_set", "t_attr_set", "t_attr_set_by_the_nodes", "t_attr_unwarped_tick_first", "t_mask_off_zero",
    "t_mask_x_inside_an_item", "t_mask_is_the_crop", "t_last_row_that_fits", "t_fallback_nodes_do_not_fit", "t_fallback_one_row_over"]

TICK_CASES = [
    tick_case("idle-waves", 48, 40, "t_idle_waves", "t_nodes_under_a_trip", "t_attr_not_set"),
    tick_case("partial-second-trip", 80, 76, "t_items_partial_last_trip", "t_last_cell_row_partial", "t_integer", "t_half_pixel", "t_other_formats", "t_burst",
              subpixel=(1, 0), formats=("Y10P", "LUMA16_LO"), burst=True),
    tick_case("two-levels-partial", 96, 84, "t_two_levels", "t_level_1_partial_last_trip", "t_mean_subtract", levels=2, mean_subtract=1),
    tick_case("flagship-128", 128, 128, "t_items_full_trips", "t_nodes_two_trips", "t_two_levels", "t_burst", levels=2, mean_subtract=1, T=4, burst=True),
    tick_case("mask-off-zero", 144, 136, "t_mask_off_zero", "t_mask_x_inside_an_item", T=4),
    tick_case("attr-by-the-nodes", 80, 307, "t_attr_set_by_the_nodes", "t_attr_unwarped_tick_first", "t_odd_height", S=4, T=3, unbound_first=True),
    tick_case("lds-border-fits", 160, 467, "t_last_row_that_fits", "t_attr_set", S=4, T=3),
    tick_case("lds-border-over", 160, 468, "t_fallback_nodes_do_not_fit", "t_fallback_one_row_over", S=4, T=3),
]
# the shape every other GPU test of the tick runs at (tests/bank_warp_rig.py's defaults)
TICK_BASELINE = tick_case("baseline-64x64", 64, 64, "t_items_one_full_trip", "t_mask_is_the_crop")

VOCABULARY = WARP_VOCABULARY + TICK_VOCABULARY
GPU_CASES = WARP_CASES + TICK_CASES + [TICK_BASELINE]


def reach(c):
    """The names of the paths a case of either list takes (VOCABULARY)."""
    return tick_reach(c) if "levels" in c else warp_reach(c)


def by_id(cid):
    return next(c for c in GPU_CASES if c["id"] == cid)
