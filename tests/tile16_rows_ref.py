"""The block-row plan of the 16x16 search in plain Python / numpy: what ONE workgroup of k_search_tile16<PRUNE, REFINE>
(csrc/k_search_tile16.hip) stages, from which bytes of the frame arrays, into which bytes of its LDS, and how many trips
each of its loops makes against the 512 lanes.  It imports nothing of the product: tests/test_tile16_rows_ref.py holds it
to aof.grid, to the oracle's skipped blocks and to the LDS size of tests/batch_plan_ref.py; tests/test_gpu_tile16_rows.py
walks CASES on the device.

  extents()     the bytes a workgroup reads of the batch's prev and cur arrays (over-reads included) and the LDS bytes it
                writes, numpy-broadcast over by / px / py (the property sweep)
  workgroup()   everything the kernel computes before its first SAD: the pre-shift, the skipped columns, the chunk counts,
                the staging form and its trips, the item / B1 / refinement trips, the extents
  paths()       the names of the branches a launch takes (VOCABULARY), one per branch of workgroup()
  CASES         the launches of the device file, each with the reason it is there
"""
import numpy as np

THREADS, SIDE, WAVE = 512, 17, 64
HINTS = (0, 1, 2, 3, 4)                         # the probe's verdicts: exhaustive scan; two-, one-, four-, eight-row bounds
FORMS = ("scan",) + tuple(f"hint{h}" for h in HINTS)   # <false, ..>; <true, ..> under each verdict (PRUNED: hint 1)


def grid(w, h, org):
    """(nx, ny) of the dense 16x16 grid at (8 + org, 8 + org), step 16, reach 8: every window inside the frame."""
    m = 8 + org
    return (w - 2 * m) // 16, (h - 2 * m) // 16


def xcd_remap(b, total):
    q, r, xcd, slot = total // 8, total % 8, b % 8, b // 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + slot


def placement(n_pairs, ny):
    """(pair, by) of every workgroup of the launch, by blockIdx.x."""
    total = n_pairs * ny
    return [(xcd_remap(b, total) // ny, xcd_remap(b, total) % ny) for b in range(total)]


def lds_layout(w, nx, prune, refine):
    """Byte offsets in the dynamic LDS: pad, s_flat (row -1), s_cur, s_prev, s_best, the pruned tables' end."""
    lead, pad = (1, 16) if refine else (0, 0)
    s_cur = pad + lead * w
    s_prev = pad + (32 + 2 * lead) * w
    s_best = pad + (48 + 2 * lead) * w
    end = s_best + 4 * nx + (2 * 2 * SIDE * nx + 4 if prune else 0)   # s_best, then s_pmin, s_list, s_count
    return dict(s_cur=s_cur, s_prev=s_prev, s_best=s_best, end=end)


def extents(w, h, org, by, px, py, pair, pair_stride, refine):
    """The first and the last byte the staging reads of the batch's cur and prev arrays (relative to their starts), and of
    the LDS bytes it writes relative to smem.  by, px, py, pair may be numpy arrays (broadcast).  cur_lo > cur_hi: nothing
    of cur is read (the block row's windows left the frame)."""
    by, px, py, pair = (np.asarray(v, dtype=np.int64) for v in (by, px, py, pair))
    sh = px & 15
    hm = h - 2 * org
    yc0 = 16 * by + py
    rows_ok = (yc0 >= 0) & (yc0 + 32 <= hm)
    base = pair * pair_stride + org * (w + 1)
    g_cur = base + yc0 * w + sh
    g_prev = base + (16 * by + 8) * w + 8
    k = w // 16
    lead, pad = (1, 16) if refine else (0, 0)
    s_cur = pad + lead * w
    s_prev = pad + (32 + 2 * lead) * w
    tail_guard = (sh != 0) & (org == 0) & rows_ok & (yc0 + 32 == hm)
    none = np.int64(-1)
    if refine:
        # rows -1 .. 31 flat, row 32 as far as W - 1 - sh bytes (chunks, then bytewise), the byte in front of row -1
        last_bytes = np.where(rows_ok, w - 1 - sh, 0)
        cur_lo = np.where(rows_ok, g_cur - w - 1, 0)
        cur_hi = np.where(rows_ok, g_cur + 32 * w + last_bytes - 1, none)
        lds_cur_lo = np.where(rows_ok, s_cur - w - 1, s_prev)
        lds_cur_hi = np.where(rows_ok, s_cur + 32 * w + last_bytes - 1, s_prev)
    else:
        # 32 rows flat; under the tail guard the last chunk shrinks to its 16 - sh bytes inside the frame
        cur_lo = np.where(rows_ok, g_cur, 0)
        cur_hi = np.where(rows_ok, g_cur + 32 * 16 * k - 1 - np.where(tail_guard, sh, 0), none)
        lds_cur_lo = np.where(rows_ok, s_cur, s_prev)
        lds_cur_hi = np.where(rows_ok, s_cur + 32 * 16 * k - 1 - np.where(tail_guard, sh, 0), s_prev)
    # prev: 16 rows from column 8 on as one flat copy -- it ends 8 bytes into the row behind them
    prev_lo, prev_hi = g_prev, g_prev + 16 * 16 * k - 1
    return dict(sh=sh, rows_ok=rows_ok, tail_guard=tail_guard, cur_lo=cur_lo, cur_hi=cur_hi, prev_lo=prev_lo + 0 * cur_lo, prev_hi=prev_hi + 0 * cur_lo,
                lds_lo=np.minimum(lds_cur_lo, s_prev), lds_hi=np.maximum(lds_cur_hi, s_prev + 16 * 16 * k - 1))


def trips(n, per=THREADS):
    return -(-n // per)


def workgroup(w, h, org, nx, ny, by, px, py, pair, n_pairs, pair_stride, prune, refine, hint=0):
    """One workgroup (k_search_tile16.hip lines 214-300, 355, 400-418, 461).  prune / refine: the instantiation; hint: the
    pair's verdict (read by the PRUNE instantiations; PRUNED mode is hint 1)."""
    assert 0 <= by < ny and 0 <= pair < n_pairs and (not refine or org == 1) and w % 16 == 0
    hint = hint if prune else 0
    pays = bool(prune and hint != 0)
    sh, q16 = px & 15, px >> 4
    hm, wb = h - 2 * org, w - 2 * org
    yc0 = 16 * by + py
    rows_ok = yc0 >= 0 and yc0 + 32 <= hm
    k = w // 16
    skip_left = [bx for bx in range(nx) if 16 * bx + px < 0]
    skip_right = [bx for bx in range(nx) if 16 * bx + px + 32 > wb]
    live = [bx for bx in range(nx) if rows_ok and bx not in skip_left and bx not in skip_right]
    cur_chunks, prev_chunks = (32 * k if rows_ok else 0), 16 * k
    tail_guard = sh != 0 and org == 0 and rows_ok and yc0 + 32 == hm
    tail_bytes = 16 - sh if tail_guard else 0
    if tail_guard:
        cur_chunks -= 1
    L = lds_layout(w, nx, prune, refine)
    base = pair * pair_stride + org * (w + 1)
    g_cur, g_prev = base + yc0 * w + sh, base + (16 * by + 8) * w + 8
    reads = dict(cur=[], prev=[(g_prev, g_prev + 16 * prev_chunks - 1)])       # inclusive byte ranges, 16-byte copies whole
    writes = [(L["s_prev"], L["s_prev"] + 16 * prev_chunks - 1), (L["s_best"], L["end"] - 1)]
    out = dict(sh=sh, q16=q16, rows_ok=rows_ok, above=yc0 < 0, below=yc0 + 32 > hm, skip_left=skip_left, skip_right=skip_right, live=live,
               cur_chunks=cur_chunks, prev_chunks=prev_chunks, tail_guard=tail_guard, tail_bytes=tail_bytes, pays=pays, hint=hint)
    if refine:
        flat_chunks = 33 * k if rows_ok else 0
        last_bytes = w - 1 - sh if rows_ok else 0
        last_chunks = last_bytes // 16
        odd = last_bytes - 16 * last_chunks
        g_flat, g_last = g_cur - w, g_cur + 32 * w
        s_flat, s_last = L["s_cur"] - w, L["s_cur"] + 32 * w
        if flat_chunks:
            reads["cur"].append((g_flat, g_flat + 16 * flat_chunks - 1)); writes.append((s_flat, s_flat + 16 * flat_chunks - 1))
        if last_chunks:
            reads["cur"].append((g_last, g_last + 16 * last_chunks - 1)); writes.append((s_last, s_last + 16 * last_chunks - 1))
        if odd:
            reads["cur"].append((g_last + 16 * last_chunks, g_last + last_bytes - 1)); writes.append((s_last + 16 * last_chunks, s_last + last_bytes - 1))
        if rows_ok:
            reads["cur"].append((g_flat - 1, g_flat - 1)); writes.append((s_flat - 1, s_flat - 1))
        total, per = flat_chunks + last_chunks + prev_chunks, 8
        # what the rings of the live blocks read of the staged rows -1 .. 32 (flat LDS offsets from s_cur): columns
        # xs - 1 .. xs + 32 over the 17 dx; all of it must have been staged
        staged = [(-w - 1, -w - 1), (-w, 32 * w - 1), (32 * w, 32 * w + last_bytes - 1)] if rows_ok else []
        ring = [(r * w + 16 * (bx + q16) - 1, r * w + 16 * (bx + q16) + 32) for bx in live for r in range(-1, 33)]
        out.update(flat_chunks=flat_chunks, last_chunks=last_chunks, odd=odd, pad_written=rows_ok, staged=staged, ring=ring,
                   row32_ends_on_last_byte=bool(rows_ok and g_last + last_bytes == n_pairs * pair_stride))
    else:
        if cur_chunks:
            reads["cur"].append((g_cur, g_cur + 16 * cur_chunks - 1)); writes.append((L["s_cur"], L["s_cur"] + 16 * cur_chunks - 1))
        if tail_bytes:
            reads["cur"].append((g_cur + 16 * cur_chunks, g_cur + 16 * cur_chunks + tail_bytes - 1))
            writes.append((L["s_cur"] + 16 * cur_chunks, L["s_cur"] + 16 * cur_chunks + tail_bytes - 1))
        total, per = cur_chunks + prev_chunks, 8 if pays else 1
    # the windows of the live blocks: LDS columns [xs, xs + 32) of rows 0 .. 31, xs = 16 (bx + (px >> 4))
    out["windows"] = [(16 * (bx + q16), 16 * (bx + q16) + 31) for bx in live]
    st = trips(total, per * THREADS)
    rest = total - (st - 1) * per * THREADS
    items = SIDE * nx if rows_ok else 0
    b1_lanes = 4 * ((nx + 15) // 16 * 16) if rows_ok and pays else 0
    rq_lanes = (4 * nx + 63) // 64 * 64 if refine else 0
    out.update(stage=per, stage_total=total, stage_trips=st, stage_clamped=per == 8 and rest < 8 * THREADS, stage_partial=per == 1 and rest < THREADS,
               items=items, item_trips=trips(items), last_wave_lanes=items % WAVE, wave_walk_trips=trips((items + 63) // 64 * 64),
               b1_lanes=b1_lanes, b1_trips=trips(b1_lanes), b1_idle=b1_lanes > 4 * nx,
               rq_lanes=rq_lanes, rq_trips=trips(rq_lanes), rq_idle=rq_lanes > 4 * nx,
               reads=reads, writes=writes, lds_end=L["end"], layout=L, total_wgs=n_pairs * ny)
    return out


VOCABULARY = (
    "form:plain:scan", "form:plain:hint0", "form:plain:hint1", "form:plain:hint2", "form:plain:hint3", "form:plain:hint4",
    "form:refine:scan", "form:refine:hint0", "form:refine:hint1", "form:refine:hint2", "form:refine:hint3", "form:refine:hint4",
    "preshift:none", "preshift:displaced", "shift16:-2", "shift16:-1", "shift16:0", "shift16:1",
    "rows:ok", "rows:above-the-frame", "rows:below-the-frame", "skip:none", "skip:left", "skip:right",
    "tail-guard:taken", "tail-guard:not-needed", "tail-guard:displaced-inside-the-frame",
    "row32:odd-bytes", "row32:whole-chunks", "row32:ends-on-the-last-byte", "pad:written", "pad:not-written",
    "stage8:one-trip", "stage8:second-trip", "stage8:clamped-lanes", "stage1:partial-last-trip", "stage1:whole-trips",
    "items:none", "items:one-trip", "items:second-trip", "items:more-trips", "items:partial-wave", "items:whole-waves",
    "b1:one-trip", "b1:second-trip", "b1:idle-quads", "b1:every-quad-a-block",
    "refine-loop:one-wave", "refine-loop:more-waves", "refine-loop:second-trip", "refine-loop:idle-quads", "refine-loop:every-quad-a-block",
    "place:one-block-row", "place:more-block-rows", "place:total-off-8",
)


def names_of(g):
    """The branch names of one workgroup() result."""
    kind = "refine" if "odd" in g else "plain"
    n = set()
    n.add("preshift:displaced" if g["sh"] else "preshift:none")
    n.add(f"shift16:{g['q16']}")
    n.add("rows:ok" if g["rows_ok"] else "rows:above-the-frame" if g["above"] else "rows:below-the-frame")
    if g["rows_ok"]:
        n.add("skip:none" if not g["skip_left"] and not g["skip_right"] else "skip:left" if g["skip_left"] else "skip:right")
        if g["skip_left"] and g["skip_right"]:
            n.add("skip:right")
    if kind == "plain":
        n.add("tail-guard:taken" if g["tail_guard"] else "tail-guard:displaced-inside-the-frame" if g["sh"] and g["rows_ok"] else "tail-guard:not-needed")
        if g["stage"] == 8:
            n.add("stage8:one-trip" if g["stage_trips"] == 1 else "stage8:second-trip")
        else:
            n.add("stage1:partial-last-trip" if g["stage_partial"] else "stage1:whole-trips")
    else:
        n.add("pad:written" if g["pad_written"] else "pad:not-written")
        if g["rows_ok"]:
            n.add("row32:odd-bytes" if g["odd"] else "row32:whole-chunks")
        if g["row32_ends_on_last_byte"]:
            n.add("row32:ends-on-the-last-byte")
        n.add("stage8:one-trip" if g["stage_trips"] == 1 else "stage8:second-trip")
    if g["stage_clamped"]:
        n.add("stage8:clamped-lanes")
    t = g["item_trips"]
    n.add("items:none" if t == 0 else "items:one-trip" if t == 1 else "items:second-trip" if t == 2 else "items:more-trips")
    if t:
        n.add("items:partial-wave" if g["last_wave_lanes"] else "items:whole-waves")
    if g["b1_lanes"]:
        n.add("b1:one-trip" if g["b1_trips"] == 1 else "b1:second-trip")
        n.add("b1:idle-quads" if g["b1_idle"] else "b1:every-quad-a-block")
    if kind == "refine":
        n.add("refine-loop:one-wave" if g["rq_lanes"] == WAVE else "refine-loop:more-waves")
        if g["rq_trips"] > 1:
            n.add("refine-loop:second-trip")
        n.add("refine-loop:idle-quads" if g["rq_idle"] else "refine-loop:every-quad-a-block")
    return n


# ---- launches ---------------------------------------------------------------------------------------------------------------

def case(id, w, h, why, *, sub=0, levels=1, eq=0, n=4, frames="designed", batches=1, **kw):
    org = 1 if sub else 0
    nx, ny = grid(w, h, org)
    assert nx >= 1 and ny >= 1 and w % 16 == 0 and w <= 2096 and h <= 128, id
    return dict(id=id, w=w, h=h, sub=sub, org=org, levels=levels, eq=eq, n_pairs=n, nx=nx, ny=ny, frames=frames, batches=batches, why=why, **kw)


def workgroups(c, preds=None, forms=FORMS, n_pairs=None):
    """Every workgroup of every form of the case's launch; preds: (px, py) per pair (two levels: the oracle's), else zeros."""
    n = c["n_pairs"] if n_pairs is None else n_pairs
    preds = preds if preds is not None else [(0, 0)] * n
    assert len(preds) == n and (c["levels"] == 2 or all(p == (0, 0) for p in preds))
    seen = {}
    for form in forms:
        prune, hint = (0, 0) if form == "scan" else (1, int(form[4:]))
        for pair, (px, py) in enumerate(preds):
            for by in range(c["ny"]):
                key = (form, px, py, by, pair == n - 1)     # (the pair index matters to the last pair's extents alone)
                if key not in seen:
                    seen[key] = workgroup(c["w"], c["h"], c["org"], c["nx"], c["ny"], by, px, py, pair, n, c["w"] * c["h"], prune, bool(c["sub"]), hint)
                    yield form, seen[key]


def paths(c, preds=None, n_pairs=None):
    """The names of the branches the case's launches take between them (every form on the same frames)."""
    n = c["n_pairs"] if n_pairs is None else n_pairs
    out = {"place:one-block-row" if c["ny"] == 1 else "place:more-block-rows"}
    if (n * c["ny"]) % 8:
        out.add("place:total-off-8")
    for form, g in workgroups(c, preds, n_pairs=n_pairs):
        out.add(f"form:{'refine' if c['sub'] else 'plain'}:{form}")
        out |= names_of(g)
    return out


def stage8_border_widths(refine):
    """The last width whose block row is staged in one trip of stage_chunks<8> (4 096 chunks) and the next one."""
    w = 48
    while workgroup(w + 16, 50 if refine else 48, int(refine), *grid(w + 16, 50 if refine else 48, int(refine)), 0, 0, 0, 0, 1, 0, 1, refine, 1)["stage_trips"] == 1:
        w += 16
    return w, w + 16


PLAIN_BORDER, REFINE_BORDER = stage8_border_widths(False), stage8_border_widths(True)

H_SHIFTS = [(sx, (k % 7) - 3) for k, sx in enumerate(range(-17, 18))]     # one pair per horizontal shift, sy cycling -3 .. 3
V_SHIFTS = [(0, -17), (3, -9), (-5, 9), (0, 17)]

CASES = [
    # item trips
    case("items-510", 496, 48, "nx 30: 510 items, one trip, two idle lanes"),
    case("items-510-half-pixel", 512, 50, "nx 30 with the refinement", sub=1),
    case("items-527", 512, 48, "nx 31: 527 items, a second trip of 15 lanes; 1 536 chunks: stage<1> in whole trips"),
    case("items-527-half-pixel", 528, 50, "nx 31 with the refinement", sub=1),
    case("items-561-list-over-512", 544, 48, "nx 33: the first grid whose B2 list (16 rows per block) can outgrow 512 entries", b2=True),
    case("one-block", 32, 48, "nx 1: 17 items, a quarter of a wave"),
    case("one-block-half-pixel", 48, 50, "nx 1 with the refinement: one quad of the refinement's wave works", sub=1),
    case("two-blocks", 48, 48, "nx 2"),
    # quad loops
    case("quads-16", 272, 48, "nx 16: B1's round-up changes nothing"), case("quads-17", 288, 48, "nx 17: B1 rounds up to 32 blocks"),
    case("quads-16-half-pixel", 288, 50, "nx 16: the refinement fills one wave exactly", sub=1),
    case("quads-17-half-pixel", 304, 50, "nx 17: the refinement spills into a second wave", sub=1),
    case("quads-128", 2064, 48, "nx 128: B1 fills one 512-lane trip exactly; 2 176 items are whole waves", n=2),
    case("quads-129", 2080, 48, "nx 129: B1 needs a second trip", n=2),
    case("quads-128-half-pixel", 2080, 50, "nx 128: B1 and the refinement fill one trip exactly", sub=1, n=2),
    case("quads-129-half-pixel", 2096, 50, "nx 129: B1 and the refinement need a second trip; 113 KB of LDS", sub=1, n=2),
    # staging trips
    case("stage8-last-one-trip", PLAIN_BORDER[0], 48, "4 080 chunks: one trip of stage<8>, clamped lanes; stage<1> partial", n=2),
    case("stage8-first-two-trips", PLAIN_BORDER[1], 48, "4 128 chunks: a second trip of 32 chunks", n=2),
    case("stage8-last-one-trip-half-pixel", REFINE_BORDER[0], 50, "4 049 chunks with rows -1 and 32", sub=1, n=2),
    case("stage8-first-two-trips-half-pixel", REFINE_BORDER[1], 50, "4 099 chunks: a second trip of 3 chunks", sub=1, n=2),
    # the predictor's pre-shift
    case("shifts-x", 320, 128, "every px & 15, px >> 4 in -1 .. 1, windows out at both edges, the tail guard", levels=2, n=35, frames="h-shifts"),
    case("shifts-x-half-pixel", 320, 128, "the same, px >> 4 down to -2, byte-aligned sources", levels=2, sub=1, n=35, frames="h-shifts"),
    case("shifts-y", 320, 128, "block rows pushed out above and below", levels=2, n=4, frames="v-shifts"),
    case("shifts-y-half-pixel", 320, 128, "the same with rows -1 and 32", levels=2, sub=1, n=4, frames="v-shifts"),
    # the ring on the last byte
    case("ring-160x50", 160, 50, "H % 16 == 2: row 32 of the last block row ends on the frame arrays' last byte", sub=1, n=3, frames="ring", batches=10),
    case("ring-160x50-equalised", 160, 50, "the same under a delta", sub=1, eq=1, n=3, frames="ring", batches=10),
    case("ring-304x98", 304, 98, "six block rows, nx 17", sub=1, n=3, frames="ring", batches=10),
    case("ring-304x98-equalised", 304, 98, "the same under a delta", sub=1, eq=1, n=3, frames="ring", batches=10),
    case("ring-304x50", 304, 50, "the wide frame at two block rows", sub=1, n=3, frames="ring", batches=10),
    case("ring-304x50-equalised", 304, 50, "the same under a delta", sub=1, eq=1, n=3, frames="ring", batches=10),
    case("ring-160x98", 160, 98, "the narrow frame at six block rows", sub=1, n=3, frames="ring", batches=10),
    case("ring-160x98-equalised", 160, 98, "the same under a delta", sub=1, eq=1, n=3, frames="ring", batches=10),
    case("ring-corner-bytes", 160, 50, "one ring byte decides the direction: row 32's last bytewise byte on the frame's last row, the pad byte on its first",
         sub=1, n=3, frames="corners", batches=3, gate_off=True),
    # placement
    case("place-1x1", 96, 32, "one workgroup", n=1), case("place-3x1", 96, 32, "3 workgroups, one block row", n=3),
    case("place-7x1", 96, 32, "7 workgroups", n=7), case("place-9x1", 96, 32, "9 workgroups: XCD 0 gets two", n=9),
    case("place-3x2", 96, 48, "6 workgroups, two block rows", n=3), case("place-5x2", 96, 48, "10 workgroups", n=5),
    # equalisation under the pre-shift
    case("equalised-pre-shift", 320, 128, "a saturating brightness step staged displaced: sat_add on the unaligned copy", levels=2, sub=1, eq=1, n=4,
         frames="bright-steps"),
]


def batch_pairs(c, k=0):
    """Pairs of batch k of the case (the ring and corner cases: texture k is the LAST pair of a batch of 1 .. 3)."""
    return 1 + k % 3 if c["frames"] in ("ring", "corners") else c["n_pairs"]
