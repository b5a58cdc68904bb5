"""The model of the small-pair kernels' plans (tests/small_plan_ref.py) at its boundaries, worked out by hand; the coverage
of its decodes on every case -- every byte of every buffer a `load` names written by one (trip, k, lane) and none of any
other, every level-1 pixel written once, every (block, dy) searched by one (trip, lane), every refinement quad in one wave,
every LDS read inside the allocation with the bytes read beyond a frame in that frame's pad, every (pair, block) of a
grouped launch owned by one lane --; every device case reaching the paths it is listed for; and the census: a path of the
vocabulary that no device case takes fails.  No GPU.  tests/test_host_asan.py holds small_plan_make and lane8_group_plan to
the same model, tests/test_gpu_small_plan.py runs GPU_CASES."""
import numpy as np
import pytest

import small_plan_ref as ref

EVERY_CASE = ref.CPU_CASES + ref.GPU_CASES
SERVED = [c for c in EVERY_CASE if ref.case_plan(c)["verdict"] == "ok" and all(1 <= ref.blocks(g) <= 256 for g in ref.grids(c)[: c["levels"]])]
# the level-1 predictors level 0 is tried under: none, every alignment of the window's first byte, the largest of a level-1
# search with half-pixel refinement (2 * 4 + 1) on either side
PREDICTORS = [(px, py) for px in (-9, -8, -3, -2, -1, 0, 1, 2, 3, 8, 9) for py in (-9, 0, 9)]


def by_id(cid):
    return next(c for c in EVERY_CASE if c["id"] == cid)


def shape(c):
    return c["w"], c["h"], tuple(ref.blocks(g) for g in ref.grids(c))


def test_the_grid_rule_gives_the_shapes_worked_out_by_hand():
    assert shape(by_id("nb-8-nx-1")) == (16, 72, (8, 0)) and ref.grids(by_id("nb-8-nx-1"))[0][4] == 1
    assert shape(by_id("nb-127-chunks-over-a-trip")) == (16, 1025, (127, 0))
    assert shape(by_id("nb-256-nx-1")) == (16, 2056, (256, 0)) and shape(by_id("nb-257-nx-1")) == (16, 2064, (257, 0))
    assert shape(by_id("nb-225-one-trip")) == (128, 128, (225, 0)) and shape(by_id("nb-255")) == (128, 144, (255, 0))
    assert shape(by_id("nb-256-half-pixel")) == (144, 138, (256, 0))
    assert shape(by_id("d1-66")) == (64, 98, (66, 0)) and shape(by_id("d1-64")) == (80, 74, (64, 0)) and shape(by_id("d1-16")) == (48, 42, (16, 0))
    assert shape(by_id("l1-1x8")) == (32, 144, (51, 8)) and ref.grids(by_id("l1-1x8"))[1][4:] == (1, 8)
    assert shape(by_id("l1-7-blocks")) == (32, 142, (48, 7))
    assert shape(by_id("lds-fit-one-level"))[:2] == (368, 217) and shape(by_id("lds-over-one-level"))[:2] == (368, 218)
    assert shape(by_id("lds-fit-two-levels"))[:2] == (64, 998) and shape(by_id("lds-over-two-levels"))[:2] == (64, 1000)
    assert shape(by_id("attr-48k-not-set"))[:2] == (80, 307) and shape(by_id("attr-set"))[:2] == (80, 308)
    # the published sparse grid: 5 x 5 whatever the frame
    assert all(ref.blocks(g) == 25 for c in EVERY_CASE if c["px4"] for g in ref.grids(c)[: c["levels"]])


def test_the_plans_at_the_boundaries_worked_out_by_hand():
    # the LDS limit: 160 KiB less 4 KiB of static arrays = 159 744 bytes of frames and pads
    assert ref.LDS_LIMIT - ref.STATIC_LDS == 159744
    assert 2 * (368 * 217 + 16) == 159744 == ref.case_plan(by_id("lds-fit-one-level"))["lds"]
    assert ref.case_plan(by_id("lds-over-one-level"))["lds"] == 159744 + 2 * 368 and ref.case_plan(by_id("lds-over-one-level"))["verdict"] == "lds"
    # two levels: 2 x (63 872 + 16) + 2 x 15 984 (15 968 + 16, a multiple of 16 already)
    assert 2 * (64 * 998 + 16) + 2 * (32 * 499 + 16) == 159744 == ref.case_plan(by_id("lds-fit-two-levels"))["lds"]
    assert ref.case_plan(by_id("lds-over-two-levels"))["lds"] == 160064 and ref.case_plan(by_id("lds-over-two-levels"))["verdict"] == "lds"
    # the attribute: above 48 KiB, so not AT 49 152
    a, b = ref.case_plan(by_id("attr-48k-not-set")), ref.case_plan(by_id("attr-set"))
    assert (a["lds"], a["attr"]) == (49152, 0) and (b["lds"], b["attr"]) == (49152 + 160, 1)
    assert all(ref.case_plan(by_id(i))["attr"] == 1 for i in ("lds-fit-one-level", "lds-fit-two-levels"))
    # pass A: 2 048 chunks a trip; 128 x 128 is one trip exactly, 16 x 1025 two chunks more
    assert ref.TRIP_A == 2048
    p = ref.case_plan(by_id("nb-225-one-trip"))
    assert ref.pass_a(p, 3)["items"] == 2048 and p["trips_a"] == (1, 1, 1)
    p = ref.case_plan(by_id("nb-127-chunks-over-a-trip"))
    assert ref.pass_a(p, 3)["items"] == 2050 and p["trips_a"] == (1, 1, 2) and ref.pass_a(p, 3)["per_frame"] % 64 == 1
    # pass C: 9 items a block; 8 blocks fill 72 lanes (two waves search, two only meet the barriers), 28 and 29 sit either
    # side of a second trip, 256 blocks are nine trips exactly
    want = {"nb-8-nx-1": (72, 1), "nb-28": (252, 1), "nb-29": (261, 2), "nb-255": (2295, 9), "nb-256-nx-1": (2304, 9), "nb-256-half-pixel": (2304, 9)}
    for cid, (items, trips) in want.items():
        p = ref.case_plan(by_id(cid))
        assert (p["nb"][0] * 9, p["trips_c"][0]) == (items, trips), cid
    c = ref.pass_c(ref.case_plan(by_id("nb-8-nx-1")), 0)
    assert set((c["lane"] // 64).tolist()) == {0, 1}
    # D1: four lanes a block in whole waves: 16 blocks are one wave, 64 one trip, 66 leave 8 live and 56 padding lanes in the
    # second trip's first wave
    for cid, lanes, trips in (("d1-16", 64, 1), ("d1-64", 256, 1), ("d1-66", 320, 2), ("nb-256-half-pixel", 1024, 4)):
        p = ref.case_plan(by_id(cid))
        d = ref.pass_d1(p, 0)
        assert (d["q"].size, p["trips_d1"][0]) == (lanes, trips), cid
    d = ref.pass_d1(ref.case_plan(by_id("d1-66")), 0)
    second = d["trip"] == 1
    assert int(d["live"][second].sum()) == 8 and int((~d["live"][second]).sum()) == 56 and set(d["wave"][second].tolist()) == {0}
    # the level-1 buffers: rounded up to 16 bytes where the level-1 frame is not (24 x 41 = 984 = 16 x 61 + 8)
    p = ref.case_plan(by_id("l1-rounded-buffer"))
    assert p["f1"][1] - p["f1"][0] == 984 + 16 + 8 and p["lds"] == 2 * (48 * 82 + 16) + 2 * 1008
    # without half-pixel refinement and at a height of a multiple of 8, the last block's window ends on the frame's last
    # byte: the fifth dword of its last row lies wholly in the pad -- for buffer 1 of level 1 in the allocation's last 16 bytes
    p = ref.case_plan(by_id("nb-255"))
    assert int(ref.pass_c(p, 0)["needed_end"].max()) == 128 * 144 and int(ref.pass_c(p, 0)["window"][1].max()) == 128 * 144 + 4
    p = ref.case_plan(by_id("l1-1x8"))
    c = ref.pass_c(p, 1)
    assert int(c["needed_end"].max()) == 16 * 72 and p["lds"] - 16 == p["f1"][1] + 16 * 72 < p["f1"][1] + int(c["window"][1].max()) == p["lds"] - 12


def test_every_verdict_is_the_first_condition_that_fails():
    ok = dict(w=64, h=64, levels=2, g0=(4, 4, 8, 8, 7, 7), g1=(4, 4, 8, 8, 3, 3), n_pairs=3, pair_stride=4096, prev=ref.BASE, cur=ref.BASE + 4096,
              subpixel=1)
    assert ref.small_plan(**ok)["verdict"] == "ok"
    breaks = dict(levels=dict(levels=3), tile=dict(tile=16), pairs=dict(n_pairs=1 << 23), grid0=dict(g0=(4, 4, 8, 8, 257, 1)), bins0=dict(rng0=16),
                  width=dict(w=72), stride=dict(pair_stride=4104), prev=dict(prev=ref.BASE + 8), cur=dict(cur=ref.BASE + 4100),
                  subdirs0=dict(subdirs0=0), height=dict(l1_h=31), grid1=dict(g1=None), bins1=dict(rng1=16), subdirs1=dict(subdirs1=0),
                  lds=dict(h=4096))
    names = list(breaks)
    assert names == list(ref.VERDICTS[1:])
    for i, name in enumerate(names):
        later = dict(ok)
        for other in names[i:]:      # with every later condition broken as well the first one still names the verdict
            if other == "levels":    # (three levels are not two: the level-1 conditions are then not looked at)
                continue
            later.update(breaks[other])
        later.update(breaks[name])
        if name in ("height", "grid1", "bins1", "subdirs1", "lds"):
            later["levels"] = 2
        assert ref.small_plan(**later)["verdict"] == name, name
    assert ref.small_plan(**{**ok, **breaks["levels"]})["verdict"] == "levels"
    # one pair has no stride to be off; 2^23 - 1 pairs are the most (pair * 256 in 31 bits)
    assert ref.small_plan(**{**ok, "n_pairs": 1, "pair_stride": 4104})["verdict"] == "ok"
    assert ref.small_plan(**{**ok, "n_pairs": (1 << 23) - 1})["verdict"] == "ok"
    # one level: level 1 is not looked at
    assert ref.small_plan(**{**ok, "levels": 1, "g1": None, "h": 63})["verdict"] == "ok"


def test_which_kernels_serve_a_batch():
    c = by_id("nb-28")
    assert ref.kind(c, 128) == "small" and ref.kind(c, 129) == "separate" and ref.kind(c, 5, split=True) == "separate"
    assert ref.counters(c, 128) == [0, 0, 0, 1, 0] == ref.counters(c, 129)          # (one level, no sums: the counters cannot tell)
    c = by_id("nb-8-nx-1")
    assert ref.counters(c, 128) == [0, 0, 0, 1, 0] and ref.counters(c, 129) == [1, 0, 0, 1, 0] == ref.counters(c, 33, split=True)
    c = by_id("l1-1x8")
    assert ref.counters(c) == [0, 0, 0, 1, 0] and ref.counters(c, 6, split=True) == [1, 1, 0, 1, 0]
    assert ref.counters(c, 129) == [1, 0, 0, 1, 0]                                    # (k_coarse, then the grouped level-0 search)
    # every fallback shows in the counters: it has sums or two levels
    for c in ref.GPU_CASES:
        if ref.kind(c) == "separate":
            assert ref.counters(c) != [0, 0, 0, 1, 0] and (c["mean_subtract"] or c["levels"] == 2), c["id"]
    assert ref.counters(by_id("nb-257-nx-1")) == [1, 0, 0, 1, 1]                      # (257 blocks: the flat search and K3)
    assert ref.counters(by_id("l1-7-blocks")) == [1, 0, 0, 1, 0] and ref.counters(by_id("lds-over-two-levels")) == [1, 1, 0, 1, 0]


@pytest.mark.parametrize("c", SERVED, ids=lambda c: c["id"])
def test_passes_a_and_b_write_every_byte_of_the_named_buffers_once(c):
    pl = ref.case_plan(c)
    w, h, two = c["w"], c["h"], c["levels"] == 2
    frame0, frame1 = w * h, (w // 2) * (h // 2)
    for load in (1, 2, 3):
        lds = np.zeros(pl["lds"], dtype=np.int64)
        a = ref.pass_a(pl, load)
        assert a["trip"].size == 0 or int(a["trip"].max()) + 1 == pl["trips_a"][load - 1]
        # one (trip, k, lane) per item
        key = (a["trip"] * ref.LOADS + a["k"]) * ref.THREADS + a["lane"]
        assert np.unique(key).size == key.size
        at = np.array(pl["f0"])[a["buf"]] + 16 * a["chunk"]
        for b in range(16):
            np.add.at(lds, at + b, 1)
        for buf in (0, 1):
            named = (load >> buf) & 1
            assert (lds[pl["f0"][buf]:pl["f0"][buf] + frame0] == named).all(), (load, buf)
            lds[pl["f0"][buf]:pl["f0"][buf] + frame0] = 0
        assert not lds.any(), "pass A wrote outside the level-0 frames"
        if not two:
            continue
        b_ = ref.pass_b(pl, load)
        assert int(b_["trip"].max()) + 1 == pl["trips_b"][0 if load < 3 else 1]
        assert np.unique(b_["trip"] * ref.THREADS + b_["lane"]).size == b_["lane"].size
        # reads: two 16-byte chunks of rows 2 y1 and 2 y1 + 1 of the buffer's level-0 frame
        src = (2 * b_["y1"] + 1) * w + 16 * b_["piece"] + 16
        assert int(src.max()) <= frame0 and ((load >> b_["buf"]) & 1).all()
        at = np.array(pl["f1"])[b_["buf"]] + b_["y1"] * (w // 2) + 8 * b_["piece"]
        for b in range(8):
            np.add.at(lds, at + b, 1)
        for buf in (0, 1):
            named = (load >> buf) & 1
            assert (lds[pl["f1"][buf]:pl["f1"][buf] + frame1] == named).all(), (load, buf)
            lds[pl["f1"][buf]:pl["f1"][buf] + frame1] = 0
        assert not lds.any(), "pass B wrote outside the level-1 frames"


@pytest.mark.parametrize("c", SERVED, ids=lambda c: c["id"])
def test_passes_c_and_d1_search_every_block_once_and_read_inside_the_allocation(c):
    pl = ref.case_plan(c)
    starts = sorted([*pl["f0"], *(pl["f1"] if c["levels"] == 2 else ())]) + [pl["lds"]]
    assert all(s % 16 == 0 for s in starts[:-1])
    for level in range(c["levels"]):
        W, H = ref.level_frame(pl, level)
        frame, nb = W * H, pl["nb"][level]
        bufs = pl["f1"] if level else pl["f0"]
        preds = PREDICTORS if level == 0 and c["levels"] == 2 else [(0, 0)]
        for pred in preds:
            s = ref.pass_c(pl, level, pred)
            assert s["trip"].size == nb * 9 and int(s["trip"].max()) + 1 == pl["trips_c"][level]
            assert np.unique(s["trip"] * ref.THREADS + s["lane"]).size == nb * 9
            assert np.unique(s["block"] * 9 + s["dy"]).size == nb * 9 and int(s["block"].max()) == nb - 1 and set(s["dy"].tolist()) == set(range(9))
            if pred == (0, 0):
                assert s["searched"].all(), "without a predictor every window of the grid lies in the frame"
            spans = [s["tile"], s["window"]]
            if pl["subpixel"]:
                d = ref.pass_d1(pl, level, pred)
                assert d["q"].size % 64 == 0 and int(d["trip"].max()) + 1 == pl["trips_d1"][level]
                # a quad lies in one wave of one trip, and every block has one
                quad = d["q"] // 4
                for field in ("trip", "wave", "block"):
                    assert (d[field].reshape(-1, 4) == d[field].reshape(-1, 4)[:, :1]).all(), field
                assert (d["part"].reshape(-1, 4) == np.arange(4)).all() and (quad[d["live"]] < nb).all() and int(d["live"].sum()) == 4 * nb
                spans.append(d["span"])
            for lo, hi in spans:
                if lo.size == 0:
                    continue
                assert int(lo.min()) >= 0, "a read in front of its frame"
                over = int(hi.max()) - frame
                for b in bufs:       # (either buffer holds either frame of the pair)
                    nxt = starts[starts.index(b) + 1]
                    # whatever is read beyond the frame lies in its own pad: in front of the next buffer, inside the allocation
                    assert b + frame + max(over, 0) <= nxt <= pl["lds"], (level, pred, over)
                assert over <= ref.PAD


GROUPED = [c for c in EVERY_CASE if c["group"] or c["over_128"]]


@pytest.mark.parametrize("c", GROUPED, ids=lambda c: c["id"])
def test_every_pair_and_block_of_a_grouped_launch_has_one_lane(c):
    counts = dict(ref.group_counts(c))
    if c["over_128"]:
        counts["over-128"] = 129
    nb = ref.blocks(ref.grids(c)[0])
    for name, n in counts.items():
        pl = ref.case_group_plan(c, n)
        assert pl["ppw"] == 256 // nb and pl["wgs"] == -(-n // pl["ppw"]) and pl["ppw"] * nb <= 256
        owned = np.zeros((n, nb), dtype=np.int64)
        for wg in range(pl["wgs"]):
            pair, blk = ref.grouped(pl, wg)
            live = pair >= 0
            assert (pair[live] < n).all() and (pair[live] // pl["ppw"] == wg).all(), "a lane owns a pair of another workgroup, or one beyond n"
            np.add.at(owned, (pair[live], blk[live]), 1)
            if wg == pl["wgs"] - 1:
                assert int(live.sum()) == pl["last_live"]
            else:
                assert int(live.sum()) == pl["ppw"] * nb
        assert (owned == 1).all(), name
    # 19 bins of a search range of 4 (55 at level 0 of two levels), two histograms a pair
    assert ref.case_group_plan(c, 1)["lds"] == (256 // nb) * 2 * (55 if c["levels"] == 2 else 19) * 4


def test_the_grouped_plan_at_the_boundaries_worked_out_by_hand():
    ppw = {cid: ref.case_group_plan(by_id(cid), 1)["ppw"] for cid in ("nb-8-nx-1", "nb-9", "nb-85", "nb-86", "nb-128", "nb-129", "nb-255", "nb-256-nx-1")}
    assert ppw == {"nb-8-nx-1": 32, "nb-9": 28, "nb-85": 3, "nb-86": 2, "nb-128": 2, "nb-129": 1, "nb-255": 1, "nb-256-nx-1": 1}
    assert 28 * 9 == 252                                   # nine blocks: four idle lanes behind the 28 pairs
    pair, _ = ref.grouped(ref.case_group_plan(by_id("nb-9"), 28), 0)
    assert [len(set(pair[64 * k:64 * k + 64].tolist()) - {-1}) for k in range(4)] == [8, 8, 8, 7] and int((pair < 0).sum()) == 4
    assert ref.group_counts(by_id("nb-8-nx-1")) == {"ppw-1": 31, "ppw": 32, "ppw+1": 33, "kppw+1": 65}
    assert ref.case_group_plan(by_id("nb-8-nx-1"), 33)["last_live"] == 8 and ref.case_group_plan(by_id("nb-8-nx-1"), 31)["last_live"] == 248
    assert ref.case_group_plan(by_id("nb-257-nx-1"), 3)["ppw"] == 0 and ref.case_group_plan(by_id("l1-7-blocks"), 3, level=1)["ppw"] == 0
    assert max(n for c in ref.GPU_CASES for n in ref.group_counts(c).values()) < 300


@pytest.mark.parametrize("c", ref.GPU_CASES, ids=lambda c: c["id"])
def test_every_device_case_reaches_the_paths_it_is_listed_for(c):
    assert c["tags"], "a case without a path has no reason to be in the list"
    got = ref.reach(c)
    assert set(c["tags"]) <= set(ref.VOCABULARY), set(c["tags"]) - set(ref.VOCABULARY)
    assert set(c["tags"]) <= got, (c["id"], sorted(set(c["tags"]) - got))
    assert got <= set(ref.VOCABULARY), got - set(ref.VOCABULARY)
    # small device bytes: no frame beyond 80 KB, no launch of the one kernel beyond 129 pairs
    assert c["w"] * c["h"] <= 82 * 1000 and c["n_pairs"] <= 128
    if c["over_128"]:
        assert ref.kind(c, 129) == "separate" and ref.kind(c, 128) == "small"
    if min(ref.blocks(g) for g in ref.grids(c)[: c["levels"]]) < 10:
        assert ref.params_kw(c)["min_valid"] == 0
    if c["percall"]:
        assert ref.kind(c, 1) == "small"
    assert ref.kind(c) == ("separate" if any(t.startswith("fallback_") for t in got) else "small")


def test_the_device_cases_reach_every_path_between_them():
    """The census."""
    reached = set()
    for c in ref.GPU_CASES:
        reached |= ref.reach(c)
    missing = set(ref.VOCABULARY) - reached
    assert not missing, f"paths no device case reaches: {sorted(missing)}"
    # every verdict is a fallback some device case takes, or one no launch can have
    assert {v for v in ref.VERDICTS[1:] if "fallback_" + v not in reached} == set(ref.UNREACHABLE_VERDICTS)
    ids = [c["id"] for c in EVERY_CASE + ref.PLAN_ONLY]
    assert len(set(ids)) == len(ids)
    # the per-call forms: both fits of the LDS limit, the attribute, two levels with the buffer border inside a wave, both
    # values of SUBPIXEL
    per_call = {c["id"] for c in ref.GPU_CASES if c["percall"]}
    assert {"lds-fit-one-level", "lds-fit-two-levels", "attr-set", "l1-rounded-buffer", "per-call-integer"} <= per_call


def test_the_census_fails_when_any_device_case_is_removed(monkeypatch):
    """Every device case is the only one on some path."""
    every = list(ref.GPU_CASES)
    for c in every:
        monkeypatch.setattr(ref, "GPU_CASES", [x for x in every if x is not c])
        with pytest.raises(AssertionError, match="paths no device case reaches"):
            test_the_device_cases_reach_every_path_between_them()


def test_the_frames_of_the_device_cases_are_what_the_cases_say(aof, orc, synth):
    """The parameter check takes every case and the product's grids are the model's; and on the oracle's records, every
    input does what it is there for (small_plan_ref.check_inputs: gated, skipped, rejected and tied blocks, both sides of
    both thresholds, saturation both ways, neighbours that differ)."""
    for c in ref.GPU_CASES:
        frames = ref.hard_pairs(c, synth)
        p = ref.case_params(c, aof, orc, synth, frames)
        assert aof.check_params(p) == 0, c["id"]
        for level in range(c["levels"]):
            assert tuple(aof.grid(p, level)) == ref.grids(c)[level], c["id"]
        po = orc.params_from(p)
        outs = [orc.flow_pair(po, a, b, want_l1=True) for a, b in zip(frames[0], frames[1])]
        ref.check_inputs(c, p, *frames, outs)
