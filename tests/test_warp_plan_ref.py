"""The model of the two lens kernels' plans (tests/warp_plan_ref.py) at its boundaries, worked out by hand; every device case
reaching the paths it is listed for; the census: a path of the vocabulary that no device case takes fails; the model against
the library where the library answers without a GPU (aof_bank_warp_one_launch; tests/test_host_asan.py holds warp_plan_make
to the same model); the coverage of the vector path's decode -- every 16-pixel item of every strip made by one (trip, lane)
--; and the proof that the warp kernel's mid-loop flush cannot be reached at any served shape.  No GPU."""
import numpy as np
import pytest

import bank_warp_ref as wref
import bank_warp_tick_cases as tc
import warp_plan_ref as ref


def wp(cid):
    return ref.case_warp_plan(ref.by_id(cid))


def tp(cid):
    return ref.case_tick_plan(ref.by_id(cid))


def test_the_warp_launch_plan_at_the_boundaries_worked_out_by_hand():
    assert all(ref.nodes(s) == n for s, n in ((1, 2), (8, 2), (9, 3), (64, 9), (128, 17), (1920, 241), (24576, 3073)))
    assert all((ref.nodes(w), ref.nodes(h)) == wref.mesh_size(w, h) for w in range(1, 200) for h in (1, 7, 8, 9, 307))
    # 380 items: a second trip with 124 live lanes; 121 nodes of which the strip clamps 11 rows; the last cell row has 4 rows
    p = wp("vector-partial-trips")
    assert (p["items"][0], p["trips"][0], p["items"][0] - 256, p["nx"] * p["ny"], p["node_rows"][0], 76 % 8) == (380, 2, 124, 121, 11, 4)
    # 289 nodes: two trips of the node loop; 1 024 items: four full trips
    p = wp("vector-node-trips")
    assert (p["node_rows"][0] * p["nx"], p["items"][0], p["trips"][0], p["nstrips"]) == (289, 1024, 4, 1)
    # 144 x 136: 128 + 8 rows, nine pieces a row, the mask from (8, 4) to (136, 132): both x edges cut an item
    p = wp("vector-mask-inside-an-item")
    assert (p["rows"], p["items"], ref.mask(144, 136)) == ((128, 8), (1152, 72), (8, 4, 136, 132)) and 8 % 16 and 136 % 16
    assert p["node_rows"] == (17, 2) and p["zero_hist"] == 1
    assert ref.mask(64, 64) == (0, 0, 64, 64) and ref.mask(16, 136) == (0, 4, 16, 132) and ref.mask(128, 128) == (0, 0, 128, 128)
    # a lane per pixel: by the width, and at a width of 16 by the destination alone
    assert wp("per-pixel-20x12")["vec"] == 0 and wp("per-pixel-two-strips")["items"] == (128 * 20, 8 * 20)
    assert wp("per-pixel-by-alignment")["vec"] == 0 and wp("vector-64x64")["vec"] == 1
    assert ref.warp_plan(64, 64, 2, ref.BASE, 4100)["vec"] == 0 and ref.warp_plan(64, 64, 2, 0, 4100)["vec"] == 1, "no destination: nothing to align"
    # the halving: 17 node rows of 241 nodes are 8 bytes over 32 KiB, of 239 nodes 264 under
    assert ref.node_bytes(128, 241) == 32776 and ref.node_bytes(128, 239) == 32504
    p = wp("strip-halved")
    assert (p["strip_rows"], p["nstrips"], p["rows"], p["node_rows"], p["lds"]) == (64, 2, (64, 8), (9, 2), 9 * 241 * 8)
    assert ref.warp_plan(1904, 72)["strip_rows"] == 128 and ref.warp_plan(1904, 72)["nstrips"] == 1, "1 904 is not halved"
    # 32 768 / 8 = 4 096 nodes: 17 rows of 240, 9 of 455, 5 of 819, 3 of 1 365
    assert [ref.strip_rows_of(w) for w in (1904, 1920, 3632, 3648, 6544, 6560, 10912, 10928)] == [128, 64, 64, 32, 32, 16, 16, 8]
    # over 48 KiB: 2 node rows of 3 073 nodes; the last width served and the first refused
    p, q, r = wp("nodes-over-48k"), wp("nodes-at-the-limit"), wp("too-wide")
    assert (p["lds"], p["attr"], ref.warp_plan(24560, 8)["lds"], ref.warp_plan(24560, 8)["attr"]) == (49168, 1, 49136, 0)
    assert (q["lds"], q["attr"], q["verdict"]) == (61424, 1, "ok") and (r["verdict"], r["lds"]) == ("too_wide", 61456)
    assert ref.width_limit() == 30720 == ref.by_id("too-wide")["w"]
    assert ref.warp_plan(30712, 8)["verdict"] == "ok" and ref.warp_plan(30712, 8)["lds"] == ref.NODE_BYTES_MAX and ref.warp_plan(30713, 8)["verdict"] == "too_wide"
    # a taller crop at the limit: every strip is one cell row and asks for the same bytes
    p = ref.warp_plan(30704, 20)
    assert (p["strip_rows"], p["nstrips"], p["rows"], p["node_rows"]) == (8, 3, (8, 4), (2, 2))
    assert ref.warp_plan(16, 1 << 20, 1 << 18)["verdict"] == "too_many" and ref.warp_plan(16, 128, 0x7FFFFFFF)["verdict"] == "ok"


def test_the_warped_ticks_plan_at_the_boundaries_worked_out_by_hand():
    p = tp("baseline-64x64")
    assert (p["items"], p["trips"], p["last_live"], p["nx"] * p["ny"], p["lds"], p["attr"]) == (256, 1, 256, 81, 8872, 0)
    p = tp("idle-waves")
    assert (p["items"], p["nx"] * p["ny"], 256 - p["items"]) == (120, 42, 136), "lanes 120 .. 255: eight of wave 1 and two whole waves"
    p = tp("partial-second-trip")
    assert (p["items"], p["trips"], p["last_live"]) == (380, 2, 124)
    p = tp("two-levels-partial")
    assert (p["items"], p["last_live"], p["l1_items"]) == (504, 248, 252)
    p = tp("flagship-128")
    assert (p["items"], p["trips"], p["last_live"], p["nx"] * p["ny"], p["node_trips"], p["lds"]) == (1024, 4, 256, 289, 2, 2 * 16400 + 2 * 4112 + 2312)
    p = tp("mask-off-zero")
    assert (p["items"], ref.mask(144, 136)[:2]) == (1224, (8, 4))
    p = tp("attr-by-the-nodes")
    assert (p["plain"], p["plain_attr"], p["nx"] * p["ny"], p["lds"], p["attr"], 307 % 8) == (49152, 0, 440, 52672, 1, 3)
    p, q = tp("lds-border-fits"), tp("lds-border-over")
    assert (p["fits"], p["spare"], q["fits"], q["plain_fits"]) == (True, 192, False, True)
    assert [ref.tick_path(ref.by_id(i)) for i in ("lds-border-fits", "lds-border-over")] == [1, 2]
    assert all(ref.case_tick_plan(c)["nodes_at"] % 16 == 0 for c in ref.TICK_CASES), "the node region starts on 16 bytes"


WARP_SERVED = [c for c in ref.WARP_CASES if ref.case_warp_plan(c)["verdict"] == "ok"]


@pytest.mark.parametrize("c", [c for c in WARP_SERVED if ref.case_warp_plan(c)["vec"]], ids=lambda c: c["id"])
def test_the_vector_path_makes_every_item_of_every_strip_once_and_reads_nodes_of_its_strip(c):
    pl = ref.case_warp_plan(c)
    w, h = c["w"], c["h"]
    made = np.zeros((h, w // 16), np.int64)
    for strip in range(pl["nstrips"]):
        got, items = ref.vector_items(pl, strip)
        assert items == pl["items"][0 if strip < pl["nstrips"] - 1 or pl["nstrips"] == 1 else 1]
        assert len({(t, lane) for t, lane, _, _ in got}) == len(got) == items
        assert max(t for t, _, _, _ in got) + 1 == ref.trips(items)
        cy0 = strip * pl["strip_rows"] // 8
        node_rows = pl["node_rows"][0 if strip < pl["nstrips"] - 1 or pl["nstrips"] == 1 else 1]
        for _, _, y, x in got:
            made[y, x // 16] += 1
            # the four node rows and columns an item reads lie in the strip's LDS copy: rows (y >> 3) - cy0 and the next, columns x >> 3 .. + 2
            assert 0 <= (y >> 3) - cy0 and (y >> 3) - cy0 + 1 < node_rows and (x >> 3) + 2 < pl["nx"]
        assert node_rows * pl["nx"] * ref.POINT_BYTES <= pl["lds"], "a strip's nodes lie in the launch's LDS"
    assert (made == 1).all()


@pytest.mark.parametrize("c", ref.GPU_CASES, ids=lambda c: c["id"])
def test_every_device_case_reaches_the_paths_it_is_listed_for(c):
    assert c["tags"], "a case without a path has no reason to be in the list"
    got = ref.reach(c)
    assert set(c["tags"]) <= set(ref.VOCABULARY), set(c["tags"]) - set(ref.VOCABULARY)
    assert set(c["tags"]) <= got, (c["id"], sorted(set(c["tags"]) - got))
    assert got <= set(ref.VOCABULARY), got - set(ref.VOCABULARY)
    if "levels" in c:
        assert all(ref.tick_small_plan(c, s)["verdict"] == "ok" for s in c["subpixel"]), "the one-workgroup class on the published 25-block grid"
        assert c["w"] * c["h"] * c["S"] * c["T"] <= 5 * 6 * 96 * 84 or c["T"] <= 4, "device bytes and ticks stay small"
    else:
        assert ref.case_frames(c) * c["w"] * c["h"] <= 1 << 21, "small device bytes"


def test_the_device_cases_reach_every_path_between_them():
    """The census."""
    reached = set()
    for c in ref.GPU_CASES:
        reached |= ref.reach(c)
    missing = set(ref.VOCABULARY) - reached
    assert not missing, f"paths no device case reaches: {sorted(missing)}"
    assert {v for v in ref.VERDICTS[1:] if "w_" + v not in reached} == set(ref.UNREACHABLE_WARP_VERDICTS)
    ids = [c["id"] for c in ref.GPU_CASES + ref.WARP_PLAN_ONLY]
    assert len(set(ids)) == len(ids)


def test_the_census_fails_when_an_edge_case_is_removed(monkeypatch):
    """Every case the edges were added for is the only one on some path."""
    every = list(ref.GPU_CASES)
    for c in every:
        if c["id"] in ("vector-64x64", "per-pixel-20x12", "two-strips-16x136"):   # (the sizes the kernel arrived with: others repeat their paths)
            continue
        monkeypatch.setattr(ref, "GPU_CASES", [x for x in every if x is not c])
        with pytest.raises(AssertionError, match="paths no device case reaches"):
            test_the_device_cases_reach_every_path_between_them()


def test_the_model_is_the_library_on_the_one_launch_question(aof):
    """aof_bank_warp_one_launch answers without a GPU: (does the warped tick run as one launch, its dynamic LDS bytes)."""
    for c in ref.TICK_CASES + [ref.TICK_BASELINE]:
        pl = ref.case_tick_plan(c)
        for sub in c["subpixel"]:
            p = aof.px4flow_params(c["w"], c["h"], pyramid_levels=c["levels"], mean_subtract=c["mean_subtract"], subpixel=sub)
            assert aof.check_params(p) == 0, c["id"]
            assert aof.bank_warp_one_launch(p) == (ref.tick_path(c) == 1, pl["lds"]), c["id"]
            assert aof.warp_mesh_size(p) == (pl["nx"], pl["ny"]), c["id"]
            assert [tuple(aof.grid(p, l))[4:] for l in range(c["levels"])] == [(5, 5)] * c["levels"], (c["id"], "the published 25-block grid")


def test_the_inputs_of_the_tick_cases_are_what_the_cases_say(aof, orc, synth):
    """On the numpy model's crops and the oracle's records alone (bank_warp_tick_cases.prepare asserts them): every warped,
    valid stream publishes a record with quality > 0, the run holds due and not-due frames, every warped crop differs from
    the plain crop, one stream idles and one is refused.  And the runs are the ones the cases list."""
    runs = tc.every_run()
    assert len({tc.run_id(*r) for r in runs}) == len(runs) == sum(len(c["subpixel"]) + len(c["formats"]) for c in ref.TICK_CASES)
    assert sum(1 for r in runs if r[3]) == sum(1 for c in ref.TICK_CASES if c["burst"])
    for c, sub, fmt, burst in runs:
        q = tc.prepare(aof, orc, synth, c, sub, fmt, burst)
        assert len(q.want) == c["T"] + (tc.K if burst else 0) and q.path == ref.tick_path(c)
        if burst:
            assert sum(row[s][0] == tc.FRAME for row in q.want[c["T"]:] for s in range(c["S"])) == int(q.given[q.burst_at].sum()) - int(q.given[q.burst_at][tc.REFUSED])


def test_the_mid_loop_flush_is_unreachable():
    """k_bank_warp flushes a lane's 12-bit counters inside the item loop every 255 trips.  Over every width that is a multiple
    of 16 below the refusal, and every strip height the halving can leave (a strip has at most strip_rows rows, whatever the
    crop's height), the loop ends before its 255th trip: the flush behind the loop is the only one that runs, and a lane
    counts at most 16 pixels a trip into fields that hold 4 095."""
    limit, most = ref.width_limit(), (0, 0, 0)
    heights = set()
    for w in range(16, limit, 16):
        strip = ref.strip_rows_of(w)
        heights.add(strip)
        assert ref.warp_plan(w, strip)["verdict"] == "ok"
        for rows in (strip, strip - 1, 1):          # (fewer rows: fewer items)
            pl = ref.warp_plan(w, rows)
            assert pl["vec"] == 1 and pl["trips"][0] == ref.trips(rows * (w // 16))
            most = max(most, (pl["trips"][0], w, rows))
    assert heights == {128, 64, 32, 16, 8}
    assert most[0] < ref.LANE_ITEMS and 16 * most[0] < 4096, most
    assert most[0] <= 60, ("the bound derived by hand", most)
    assert ref.warp_plan(limit, 8)["verdict"] == "too_wide"
