"""The model of the flat lane-per-block 8x8 launches (tests/lane8_plan_ref.py) on the CPU: hand-worked boundaries of every
rule of the plan as literals; xcd_remap a permutation of [0, total) for every total up to 4 096 and for every case's
workgroup count, an XCD's logical ids contiguous; on every case that can be decoded lane by lane each (pair, block) item owned
by exactly one (workgroup, chunk, lane), nothing owned beyond `items`, every pair in one slice, one finaliser wave per pair,
every live lane voting for its item's pair, the arrivals a finaliser waits for equal to the lanes that vote for its pair; and
the census of the device cases.  tests/test_host_asan.py holds the C++ plan to the same model."""
import numpy as np
import pytest

import lane8_plan_ref as ref


def lane_by_lane(c):
    """The plan of a case whose lanes can be decoded one by one (one slice, at most 2^23 lanes), else None."""
    pl = ref.plan_of(c)
    return pl if pl["slices"] == 1 and pl["grid"] * pl["threads"] * max(pl["spw"], 1) <= 1 << 23 else None


DECODED = [c for c in ref.CPU_CASES + ref.GPU_CASES if lane_by_lane(c) is not None]


def plan(nb, n, **kw):
    return ref.flat_plan(nb, n, kw.pop("pair_stride", 307200), 640, 480, **kw)


def test_hand_worked_boundaries():
    # the threads switch: 6 x 256 x 1024 items
    below, at = plan(1, 1572863), plan(1, 1572864)
    assert (below["threads"], below["wgs"], below["last_live"]) == (64, 24576, 63)
    assert (at["threads"], at["wgs"], at["last_live"]) == (256, 6144, 256)
    fused = plan(1024, 1536, fused=True)            # 1 572 864 items again: 256 lanes, four finaliser waves per workgroup
    assert (fused["threads"], fused["wgs"], fused["finalisers"], fused["grid"]) == (256, 6144, 384, 6528)
    assert plan(1024, 1537, fused=True)["finalisers"] == 385 and plan(1024, 1539, fused=True)["finalisers"] == 385
    small = plan(257, 65, fused=True)
    assert (small["threads"], small["wgs"], small["finalisers"], small["grid"], small["last_live"]) == (64, 262, 65, 327, 1)
    # a 256-lane fused launch within the vote memory needs at least 768 blocks per pair
    assert -(-ref.LARGE_ITEMS // ref.VOTE_PAIRS) == 768
    # spw = clamp(chunks / 1536, 1, 8)
    walk = lambda chunks: plan(256, chunks, prune=1)
    for chunks, spw, wgs, last in ((3071, 1, 3071, 1), (3072, 2, 1536, 2), (3073, 2, 1537, 1), (12287, 7, 1756, 2), (12288, 8, 1536, 8),
                                   (13824, 8, 1728, 8), (13830, 8, 1729, 6), (1, 1, 1, 1)):
        w = walk(chunks)
        assert (w["chunks"], w["spw"], w["wgs"], w["last_chunks"]) == (chunks, spw, wgs, last), chunks
    # 289 blocks: 2 720 / 2 721 / 2 722 pairs are 3 071 / 3 072 / 3 073 chunks
    assert [plan(289, n, prune=1)["chunks"] for n in (2720, 2721, 2722)] == [3071, 3072, 3073]
    one = plan(289, 1, prune=1)
    assert (one["chunks"], one["spw"], one["wgs"], one["last_live"]) == (2, 1, 2, 33)
    # the report: one workgroup in `stride`, at most 256 slots
    assert (walk(256)["stride"], walk(256)["expected"]) == (1, 256) and (walk(257)["stride"], walk(257)["expected"]) == (2, 129)
    assert (walk(13830)["stride"], walk(13830)["expected"]) == (7, 247)
    # ADAPTIVE considers pruning from 2 048 chunks on
    assert plan(256, 2047)["prune_large"] == 0 and plan(256, 2048)["prune_large"] == 1
    # the slice length: 0x7FFF0000 / nb pairs, 2^24 - 1 at the most
    assert plan(127, 5)["per"] == (1 << 24) - 1 and plan(129, 5)["per"] == 16646652 and plan(4661, 5)["per"] == 460720
    two = [plan(4661, 460720 + 100, slice=k) for k in range(2)]
    assert [p["slices"] for p in two] == [2, 2] and [p["pairs"] for p in two] == [460720, 100] and two[1]["done"] == 460720
    assert two[1]["frame_off"] == 460720 * 307200 and two[1]["block_off"] == 460720 * 4661 and two[1]["sums_off"] == 4 * 460720
    three = [plan(4661, 2 * 460720 + 1, slice=k, prune=1) for k in range(3)]
    assert [p["pairs"] for p in three] == [460720, 460720, 1] and [p["expected"] for p in three] == [256, 0, 0]
    assert three[0]["items"] == 460720 * 4661 < 1 << 31
    # the votes verdict: the first condition that fails
    assert plan(300, 10, prune=1, votes=None)["votes"] == "pruned" and plan(300, 10, votes=None)["votes"] == "memory"
    assert plan(300, 10, rng=15, votes=(1, 0, 0))["votes"] == "fault" and plan(64, 10, rng=15)["votes"] == "bins"
    assert plan(64, 10, rng=13, votes=(1, 1, 111))["votes"] == "stride" and plan(64, 4000)["votes"] == "grid"
    assert plan(65, 2048)["votes"] == "ok" and plan(65, 2049)["votes"] == "capacity"


def test_xcd_remap_is_a_permutation_with_contiguous_xcds():
    totals = set(range(1, 4097)) | {ref.plan_of(c)["grid"] for c in ref.CASES} | {ref.plan_of(c)["wgs"] for c in ref.CASES}
    for total in sorted(t for t in totals if 0 < t < 1 << 22):
        b = np.arange(total, dtype=np.int64)
        wg = ref.xcd_remap(b, total)
        assert wg.min() == 0 and wg.max() == total - 1 and np.unique(wg).size == total, total
        for xcd in range(min(8, total)):
            ids = wg[b % 8 == xcd]
            assert (np.diff(ids) == 1).all(), (total, xcd)      # consecutive slots of an XCD: consecutive logical ids
    # the largest grids any case plans: the ends of the map
    for total in (t for t in totals if t >= 1 << 22):
        ends = np.array([0, 1, 7, 8, total - 9, total - 8, total - 1], dtype=np.int64)
        assert (ref.xcd_remap(ends, total) < total).all() and (ref.xcd_remap(ends, total) >= 0).all()


@pytest.mark.parametrize("c", DECODED, ids=lambda c: c["id"])
def test_every_item_has_one_owner(c):
    pl = lane_by_lane(c)
    o = ref.owners(pl)
    assert pl["items"] == pl["pairs"] * pl["nb"] < 1 << 31
    owned = o["item"][o["live"]]
    assert owned.size == pl["items"] and (np.bincount(owned, minlength=pl["items"]) == 1).all(), "each item owned exactly once"
    assert (o["item"][~o["live"]] >= pl["items"]).all() and (owned < pl["items"]).all(), "no lane owns an item at or beyond `items`"
    assert (o["pair"][o["live"]] * pl["nb"] + o["blk"][o["live"]] == owned).all()
    # the last workgroup, and the plan's account of it
    last = o["wg"] == pl["wgs"] - 1
    if pl["kind"] == "walk":
        ran = (o["ran"] & last).reshape(-1, ref.THREADS).any(axis=1).sum()
        assert ran == pl["last_chunks"] and 1 <= pl["last_chunks"] <= pl["spw"]
        top = o["item0"] == (pl["chunks"] - 1) * ref.THREADS
        assert (o["live"] & top).sum() == pl["last_live"]
        # chunks of a workgroup are consecutive: the carried start row goes from chunk c to chunk c + 1 of the same lanes
        item0 = o["item0"].reshape(pl["wgs"], pl["spw"], ref.THREADS)[:, :, 0]
        assert (np.diff(item0, axis=1) == ref.THREADS).all()
        assert pl["stride"] >= 1 and pl["expected"] == -(-pl["wgs"] // pl["stride"]) <= ref.PRUNE_SLOTS
        assert ((pl["wgs"] - 1) // pl["stride"]) < ref.PRUNE_SLOTS, "the last reporting workgroup's slot is inside the array"
    else:
        assert (o["live"] & last).sum() == pl["last_live"] and 1 <= pl["last_live"] <= pl["threads"]
    if pl["kind"] != "fused":
        return
    # the reduction in the launch
    wv = ref.waves(pl)
    pair_of_item = np.where(wv["live"], wv["item"] // pl["nb"], -1)
    assert (wv["votes_for"] == pair_of_item).all(), "every live lane votes for exactly one pair: its item's"
    assert (wv["votes_for"].max(axis=1) - np.where(wv["votes_for"] < 0, 1 << 40, wv["votes_for"]).min(axis=1))[wv["wave_live"]].max() <= 1, \
        "a wave covers at most two pairs"
    # lane 0 is live or the whole wave is past the end
    assert (wv["live"][:, 0] | ~wv["live"].any(axis=1)).all()
    arrivals = np.bincount(wv["votes_for"][wv["votes_for"] >= 0], minlength=pl["pairs"])
    assert arrivals.size == pl["pairs"] and (arrivals == pl["nb"]).all(), "a finaliser waits for nb arrivals: the lanes that vote for its pair"
    fin = ref.finalisers(pl)
    served = fin[fin >= 0]
    assert served.size == pl["pairs"] and (np.sort(served) == np.arange(pl["pairs"])).all(), "one finaliser wave per pair"
    assert fin.shape == (pl["finalisers"], pl["threads"] // 64) and (fin[:-1] >= 0).all() and fin[-1, 0] >= 0
    assert pl["grid"] == pl["wgs"] + pl["finalisers"]


@pytest.mark.parametrize("c", ref.CASES, ids=lambda c: c["id"])
def test_every_pair_is_in_exactly_one_slice(c):
    a = ref.plan_args(c)
    head = ref.flat_plan(**{**a, "slice": 0})
    if head["slices"] == 0:
        assert a["n_pairs"] < 1 or a["nb"] < 1
        return
    assert head["slices"] <= 3
    done = 0
    for k in range(head["slices"]):
        pl = ref.flat_plan(**{**a, "slice": k})
        assert pl["done"] == done and 1 <= pl["pairs"] <= pl["per"] and pl["items"] <= ref.MAX_ITEMS and pl["pairs"] < 1 << 24
        assert (pl["frame_off"], pl["block_off"], pl["pred_off"], pl["sums_off"]) == (done * a["pair_stride"], done * a["nb"], done, 4 * done)
        assert (pl["expected"] > 0) == (pl["kind"] == "walk" and k == 0)
        done += pl["pairs"]
    assert done == a["n_pairs"]
    beyond = ref.flat_plan(**{**a, "slice": head["slices"]})
    assert beyond["pairs"] == 0 and beyond["grid"] == 0


def test_the_case_lists():
    ids = [c["id"] for c in ref.CASES]
    assert len(set(ids)) == len(ids) and len(ref.CASES) >= 85
    assert len(DECODED) == len(ref.CPU_CASES + ref.GPU_CASES), "every case outside PLAN_ONLY is decoded lane by lane"
    assert {ref.plan_of(c)["votes"] for c in ref.CASES} == set(ref.VOTES)
    assert {ref.plan_of(c)["supported"] for c in ref.CASES} == {0, 1}
    assert {ref.plan_of(c)["slices"] for c in ref.CASES} >= {0, 1, 2, 3}
    assert {ref.flat_plan(**ref.plan_args(c))["kind"] for c in ref.PLAN_ONLY if ref.plan_args(c)["slice"] > 0} == set(ref.KINDS)


@pytest.mark.parametrize("c", ref.GPU_CASES, ids=lambda c: c["id"])
def test_a_device_case_takes_the_paths_it_names(c):
    got = ref.reach(c)
    assert set(c["paths"]) <= set(ref.VOCABULARY), set(c["paths"]) - set(ref.VOCABULARY)
    assert set(c["paths"]) <= got, (c["id"], sorted(set(c["paths"]) - got))
    assert got <= set(ref.VOCABULARY), got - set(ref.VOCABULARY)
    pl = ref.case_plan(c)
    assert pl["supported"] == 1 and pl["slices"] == 1
    # small device bytes: under half a gigabyte of frames, the frame the smallest its grid allows
    assert 2 * c["n_pairs"] * ref.pair_stride(c) < 1 << 29
    if pl["kind"] == "walk":
        assert ref.chunk_walks(ref.case_grid(c))
        assert c["mode"] == "pruned" or pl["prune_large"] == 1, "ADAPTIVE prunes only where the launch is large"
    if c["layout"]:
        assert c["w"] % 4 != 0 and ref.pair_stride(c) % 2 == 1 and ref.pair_stride(c) > c["w"] * c["h"]


def test_the_device_cases_reach_every_path_between_them():
    """The census."""
    reached = set()
    for c in ref.GPU_CASES:
        reached |= ref.reach(c)
    missing = set(ref.VOCABULARY) - reached - set(ref.UNREACHABLE)
    assert not missing, f"paths no device case reaches: {sorted(missing)}"
    assert not reached & set(ref.UNREACHABLE)


def test_the_census_fails_when_any_device_case_is_removed(monkeypatch):
    """Every device case is the only one on some path."""
    every = list(ref.GPU_CASES)
    for c in every:
        monkeypatch.setattr(ref, "GPU_CASES", [x for x in every if x is not c])
        with pytest.raises(AssertionError, match="paths no device case reaches"):
            test_the_device_cases_reach_every_path_between_them()


def test_the_frames_of_the_device_cases_are_what_the_cases_say(aof, orc, synth):
    """The parameter check takes every case and the product's grids are the model's; on the oracle's records every content
    does what it is there for (lane8_plan_ref.check_inputs); and the frames are the pinned ones."""
    seen = {}
    for c in ref.GPU_CASES:
        p = aof.default_params(c["w"], c["h"], **ref.params_kw(c))
        assert aof.check_params(p) == 0, c["id"]
        assert tuple(aof.grid(p, 0)) == ref.case_grid(c), c["id"]
        if c["levels"] == 2:
            assert tuple(aof.grid(p, 1)) == ref.case_grid(c, 1), c["id"]
        key = (c["w"], c["h"], c["levels"], c["subpixel"], c["mean_subtract"], c["num_blocks"])
        if key in seen:
            continue
        prevs, curs = ref.pairs_for(c, synth)
        po = orc.params_from(p)
        outs = [orc.flow_pair(po, a, b) for a, b in zip(prevs, curs)]
        ref.check_inputs(c, p, prevs, curs, outs)
        seen[key] = ref.digest(prevs, curs)
        assert ref.PINNED[(c["w"], c["h"], c["levels"])] == seen[key], (c["id"], seen[key])
