"""Frame ingest (k_ingest.hip) in plain numpy: the model of both kernel forms, the geometries the edge tests run, and
the launch arithmetic ("reach") that says which path of the kernel a geometry gets to.

  ingest(cam, crop_w, crop_h)  -> (crop, hist)       centre crop + 10-bin masked histogram (independent of the oracle)
  pyramid(crops)               -> (l1, sums)         what the PYRAMID form leaves in K1's place
  reach(cam, crop, ...)        -> dict               vec / strips / trips / rounds / flushes / source alignments / mask

reach() restates what the LAUNCHER and the loop headers compute (strip height, pieces per row, trip and round counts),
not the kernel's index arithmetic: it answers "does this geometry get there", never "what comes out".  Every case
names the paths it is in the list for; tests/test_ingest_ref.py asserts that reach() agrees and that the lists together
reach every path -- a geometry edited away from its path fails there, on a machine without a device.

Tests only."""
import numpy as np

# the kernel's launch constants (k_ingest.hip: kThreads, kRowsPerBlock, kUnroll, kWavePieces; aof.h: the mask, the bins)
THREADS, ROWS_PER_BLOCK, UNROLL, WAVE_PIECES = 256, 128, 4, 63
MASK, BINS = 128, 10
TRIP = UNROLL * THREADS   # items (16-byte pieces) of one trip of a workgroup


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------

def ingest(cam, crop_w, crop_h):
    h, w = cam.shape
    x0, y0 = w // 2 - crop_w // 2, h // 2 - crop_h // 2
    crop = cam[y0:y0 + crop_h, x0:x0 + crop_w].copy()
    mx0, my0 = max(crop_w // 2 - 64, 0), max(crop_h // 2 - 64, 0)
    mx1, my1 = min(crop_w // 2 + 64, crop_w), min(crop_h // 2 + 64, crop_h)
    m = crop[my0:my1, mx0:mx1].astype(np.float64)
    idx = np.floor(m * (10 / 255.0)).astype(np.int64)
    hist = np.bincount(idx[idx < 10].ravel(), minlength=10).astype(np.uint32)
    return crop, hist


def pyramid(crops):
    """crops [n][h][w] (h, w even) -> (l1 [n][h/2][w/2], sums [n-1][2][2]): the rounded 2x2 box of every frame, and per
    PAIR k the byte sums [[sum crop_k, sum l1_k], [sum crop_k+1, sum l1_k+1]] -- aof_ws_layout.sums' [pair][prev, cur][level]."""
    q = np.asarray(crops).astype(np.int64)
    n = q.shape[0]
    l1 = ((q[:, 0::2, 0::2] + q[:, 0::2, 1::2] + q[:, 1::2, 0::2] + q[:, 1::2, 1::2] + 2) >> 2).astype(np.uint8)
    s0, s1 = q.sum(axis=(1, 2)), l1.astype(np.int64).sum(axis=(1, 2))
    assert s0.max(initial=0) < 1 << 32
    sums = np.zeros((max(n - 1, 0), 2, 2), np.uint32)
    sums[:, 0, 0], sums[:, 0, 1] = s0[:-1], s1[:-1]
    sums[:, 1, 0], sums[:, 1, 1] = s0[1:], s1[1:]
    return l1, sums


# ---------------------------------------------------------------------------------------------------------------
# which path a geometry reaches
# ---------------------------------------------------------------------------------------------------------------

def launch_vec(crop_w, dst_aligned, want_crop):
    """launch_ingest's choice of the vector path: whole 16-byte pieces, and a crop buffer (if any) that takes 16-byte stores."""
    return crop_w % 16 == 0 and (not want_crop or dst_aligned)


def reach(cam, crop, *, dst_aligned=True, want_crop=True):
    """The launch of k_ingest for sensor `cam` = (w, h) and crop `crop` = (w, h).  dst_aligned: the caller's d_cropped
    and cropped_stride are multiples of 16 (irrelevant without a crop output).  The source alignments assume a
    16-byte aligned camera base and frame stride, which the device tests assert of their buffers."""
    cam_w, cam_h = cam
    cw, ch = crop
    x0, y0 = cam_w // 2 - cw // 2, cam_h // 2 - ch // 2
    vec = launch_vec(cw, dst_aligned, want_crop)
    nstrips = (ch + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK
    strip_rows = [min(ch, (s + 1) * ROWS_PER_BLOCK) - s * ROWS_PER_BLOCK for s in range(nstrips)]
    mx0, my0 = max(cw // 2 - MASK // 2, 0), max(ch // 2 - MASK // 2, 0)
    mx1, my1 = min(cw // 2 - MASK // 2 + MASK, cw), min(ch // 2 - MASK // 2 + MASK, ch)
    r = dict(vec=vec, nstrips=nstrips, strip_rows=strip_rows, x0=x0, y0=y0,
             pyramid_supported=cw % 16 == 0 and ch % 2 == 0 and dst_aligned,   # ingest_pyramid_supported
             mask=(mx0, my0, mx1, my1), mask_clamped_x=cw < MASK, mask_clamped_y=ch < MASK,
             crop_is_sensor=(cw, ch) == (cam_w, cam_h),
             # the same crop into a buffer whose base or stride is no multiple of 16 / with no crop output at all
             vec_if_dst_unaligned=launch_vec(cw, False, True), vec_if_hist_only=launch_vec(cw, False, False),
             src_align=sorted({(y0 * cam_w + x0 + y * cam_w) % 16 for y in range(ch)}))
    if vec:
        pieces = cw // 16
        items = [rows * pieces for rows in strip_rows]
        trips = [(it + TRIP - 1) // TRIP for it in items]
        rounds = [t * UNROLL for t in trips]                      # rounds of a lane: uniform, active or not
        r.update(pieces=pieces, items=items, trips=trips, rounds=rounds,
                 ragged_last_trip=[it % TRIP != 0 for it in items],
                 # round % kWavePieces == kWavePieces - 1 inside the loop (the flush behind the loop is not counted)
                 flushes_in_loop=[sum(1 for k in range(n) if k % WAVE_PIECES == WAVE_PIECES - 1) for n in rounds],
                 mask_edge_in_piece=mx0 % 16 != 0 or mx1 % 16 != 0)
    else:
        r.update(pieces=0, items=[rows * cw for rows in strip_rows], trips=[], rounds=[], ragged_last_trip=[],
                 flushes_in_loop=[], mask_edge_in_piece=False)
    return r


# What a case list has to reach, by name: predicate over reach().  The census of tests/test_ingest_ref.py asserts that
# every name is claimed by a case and that reach() of that case satisfies it.
def _vec(r):
    return r["vec"]


STATELESS_PATHS = {
    # the vector path from an unaligned source
    "vec_odd_source": lambda r: _vec(r) and any(a % 2 for a in r["src_align"]),
    "vec_all_16_alignments": lambda r: _vec(r) and len(r["src_align"]) == 16,
    "vec_alignment_moves_with_row": lambda r: _vec(r) and len(r["src_align"]) > 1,
    "vec_odd_origin_even_pitch": lambda r: _vec(r) and all(a % 2 for a in r["src_align"]),
    "vec_less_than_one_trip": lambda r: _vec(r) and r["trips"] == [1] and r["ragged_last_trip"] == [True],
    # the caller's buffer decides (the device test runs these forms on every case that satisfies the predicate)
    # crop_w % 16 == 0: vector with an aligned buffer, scalar at base + 1 or an odd stride, vector again without a crop output
    "scalar_because_of_the_buffer": lambda r: _vec(r) and not r["vec_if_dst_unaligned"] and r["vec_if_hist_only"],
    "hist_overwrite_one_strip": lambda r: r["nstrips"] == 1,
    "hist_zero_then_atomic": lambda r: r["nstrips"] >= 2,
    # the mid-loop wave flush
    "flush_in_loop": lambda r: _vec(r) and max(r["flushes_in_loop"]) >= 1,
    "two_flushes_in_loop": lambda r: _vec(r) and max(r["flushes_in_loop"]) >= 2,
    "flush_in_loop_second_strip": lambda r: _vec(r) and r["nstrips"] >= 2 and r["flushes_in_loop"][-1] >= 1,
    # ragged strips
    "vec_second_strip_one_row": lambda r: _vec(r) and r["nstrips"] == 2 and r["strip_rows"][-1] == 1,
    "vec_second_strip_two_rows": lambda r: _vec(r) and r["nstrips"] == 2 and r["strip_rows"][-1] == 2,
    "vec_three_strips_last_one_row": lambda r: _vec(r) and r["nstrips"] == 3 and r["strip_rows"][-1] == 1,
    "vec_odd_height": lambda r: _vec(r) and sum(r["strip_rows"]) % 2 == 1,
    "vec_pieces_not_pow2": lambda r: _vec(r) and r["pieces"] & (r["pieces"] - 1) != 0,
    # the mask
    "mask_edge_in_piece": lambda r: _vec(r) and r["mask_edge_in_piece"],
    "mask_clamped_both_axes": lambda r: r["mask_clamped_x"] and r["mask_clamped_y"],
    "mask_clamped_vec_one_piece": lambda r: _vec(r) and r["pieces"] == 1 and r["mask_clamped_x"] and r["mask_clamped_y"],
    "one_pixel": lambda r: r["items"] == [1],
    # scalar
    "scalar": lambda r: not r["vec"],
    "scalar_crop_is_sensor": lambda r: not r["vec"] and r["crop_is_sensor"],
}

PYRAMID_PATHS = {
    "second_trip": lambda r: max(r["trips"]) >= 2,                              # base / 2 with base > 0
    "ragged_second_trip": lambda r: any(t >= 2 and g for t, g in zip(r["trips"], r["ragged_last_trip"])),
    "ragged_trip": lambda r: any(r["ragged_last_trip"]),                        # pr >= items / 2 on an active trip
    # 64 x 64: 256 of a trip's 1024 items, i.e. 128 row-pair items for the 256 lanes -- HALF of the lanes are active in
    # the first row-pair slot of the one trip, none in the second (the issue's "half a trip")
    "quarter_trip_half_the_lanes": lambda r: r["items"] == [TRIP // 4],
    "pieces_not_pow2": lambda r: r["pieces"] & (r["pieces"] - 1) != 0,          # pr / pieces, pr % pieces
    "three_pieces": lambda r: r["pieces"] == 3,
    "two_strips": lambda r: r["nstrips"] == 2,                                  # atomics of several workgroups into one frame's sums
    "three_strips": lambda r: r["nstrips"] == 3,
    "last_strip_one_row_pair": lambda r: r["nstrips"] >= 2 and r["strip_rows"][-1] == 2,
    "odd_source_offset": lambda r: any(a % 2 for a in r["src_align"]),
    "one_full_trip_control": lambda r: r["items"] == [TRIP] and r["pieces"] == 8,
}


def case(cam, crop, *paths, note=""):
    return dict(cam=cam, crop=crop, paths=paths, note=note, id=f"{cam[0]}x{cam[1]}-{crop[0]}x{crop[1]}")


# Each size is the smallest that reaches its path.
STATELESS = [
    case((321, 241), (64, 64), "vec_odd_source", "vec_all_16_alignments", "vec_alignment_moves_with_row", "vec_less_than_one_trip",
         "scalar_because_of_the_buffer", "hist_overwrite_one_strip"),
    case((323, 243), (144, 96), "vec_odd_source", "vec_alignment_moves_with_row", "mask_edge_in_piece", "vec_pieces_not_pow2"),
    case((322, 242), (128, 128), "vec_odd_origin_even_pitch", "vec_odd_source"),
    case((320, 240), (128, 129), "vec_second_strip_one_row", "vec_odd_height", "hist_zero_then_atomic"),
    case((320, 240), (128, 130), "vec_second_strip_two_rows"),
    case((640, 480), (400, 257), "vec_three_strips_last_one_row", "vec_pieces_not_pow2", "mask_edge_in_piece", "vec_odd_height"),
    # The two wide cases reach the flush inside the loop and catch one that counts twice or does not reset.  They are
    # no overflow test and cannot catch a MISSING flush: the mask is 128 pixels wide, at most 8 pieces of a row count,
    # and no geometry brings a wave's 16-bit counters near 65 536.
    case((2048, 128), (2048, 128), "flush_in_loop"),
    case((4096, 192), (4096, 192), "two_flushes_in_loop", "flush_in_loop_second_strip", "hist_zero_then_atomic"),
    case((64, 48), (16, 1), "mask_clamped_both_axes", "mask_clamped_vec_one_piece"),
    case((64, 48), (16, 2), "mask_clamped_both_axes", "mask_clamped_vec_one_piece"),
    case((64, 48), (1, 1), "mask_clamped_both_axes", "one_pixel", "scalar"),
    case((64, 48), (15, 7), "mask_clamped_both_axes", "scalar"),
    case((100, 90), (100, 90), "scalar", "scalar_crop_is_sensor"),
]

PYRAMID = [
    case((259, 201), (192, 160), "second_trip", "ragged_second_trip", "ragged_trip", "pieces_not_pow2", "two_strips", "odd_source_offset"),
    case((640, 480), (400, 258), "three_strips", "last_strip_one_row_pair", "pieces_not_pow2", "second_trip", "ragged_second_trip"),
    case((160, 120), (64, 64), "quarter_trip_half_the_lanes", "ragged_trip"),
    case((100, 80), (48, 38), "three_pieces", "pieces_not_pow2", "ragged_trip",
         note="48x32 as first proposed is refused by aof_params_check at two levels: the PX4Flow grid of the 24x16 level-1 "
              "frame has no row of tiles (16 - 5 - 8 <= 5), and neither has 48x36 (18 - 13 <= 5); 48x38 is the smallest "
              "height of a 48-wide crop that is accepted"),
    case((320, 240), (128, 128), "one_full_trip_control"),
]

# the three forms of the PYRAMID kernel's outputs (aof_params overrides) and the sequence lengths every geometry runs at
PYRAMID_FORMS = {
    "l1_and_sums": dict(pyramid_levels=2, mean_subtract=1),
    "l1_only": dict(pyramid_levels=2),          # sums == nullptr
    "sums_only": dict(mean_subtract=1),         # l1 == nullptr
}
PYRAMID_FRAMES = (5, 2)                         # 2: frame 0 adds only as prev, frame 1 only as cur
# the production route into the same kernel (more than 128 pairs, no split_coarse), and a crop the ingest kernel
# cannot serve (width no multiple of 16): K1 itself leaves the outputs, which validates where the tests read them
PYRAMID_LONG = case((160, 120), (64, 64), "quarter_trip_half_the_lanes")
PYRAMID_LONG_FRAMES = 131
K1_VALIDATION = case((200, 160), (100, 90))


# ---------------------------------------------------------------------------------------------------------------
# frame contents
# ---------------------------------------------------------------------------------------------------------------

BIG = 512 * 1024   # sensors above this get three frames (the all-255 family is left out: the band family carries its value)


def _seed(c):
    return c["cam"][0] * 7919 + c["cam"][1] * 31 + c["crop"][0] * 131 + c["crop"][1]


def _band(rng, cam_w, cam_h):
    f = rng.integers(0, 256, (cam_h, cam_w), dtype=np.uint8)
    f[max(cam_h // 2 - 20, 0):cam_h // 2 + 20] = 255   # a band of dropped values across the mask
    return f


def frames_for(c):
    """The frame families of a stateless case [n][cam_h][cam_w]: uniform random bytes; all 255 (nothing counts); all
    37 (one bin: counter pressure and contention); random with a band of 255 across the mask."""
    cam_w, cam_h = c["cam"]
    rng = np.random.default_rng(_seed(c))
    fam = [rng.integers(0, 256, (cam_h, cam_w), dtype=np.uint8)]
    if cam_w * cam_h <= BIG:
        fam.append(np.full((cam_h, cam_w), 255, np.uint8))
    fam.append(np.full((cam_h, cam_w), 37, np.uint8))
    fam.append(_band(rng, cam_w, cam_h))
    return np.stack(fam)


def sequence_frames_for(c, n):
    """n frames of a PYRAMID case: random, the same scene moved by (+2, -1) (a pair with a flow to find), all 255, all
    37, the band family, and so on round."""
    cam_w, cam_h = c["cam"]
    rng = np.random.default_rng(_seed(c) + n)
    out = []
    while len(out) < n:
        base = rng.integers(0, 256, (cam_h, cam_w), dtype=np.uint8)
        out +=[base, np.roll(base, (-1, 2), (0, 1)), np.full((cam_h, cam_w), 255, np.uint8),
                np.full((cam_h, cam_w), 37, np.uint8), _band(rng, cam_w, cam_h)]
    return np.stack(out[:n])


def crops_of(frames, crop):
    return np.stack([ingest(f, crop[0], crop[1])[0] for f in frames])
