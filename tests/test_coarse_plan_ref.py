"""The model of the coarse passes' plans (tests/coarse_plan_ref.py) at its boundaries, worked out by hand; the coverage of
both decodes on every case -- each level-1 pixel written once, each level-0 byte summed once, no load outside the frame,
loads ahead of a pair only into the next pair's first two batches --; every device case reaching the paths it is listed
for; and the census: a path of the vocabulary that no device case takes fails.  No GPU.  tests/test_host_asan.py holds
coarse_plan_make and pyramid_plan_make to the same model, tests/test_gpu_coarse_plan.py runs GPU_CASES."""
import numpy as np
import pytest

import coarse_plan_ref as ref

EVERY_CASE = ref.CPU_CASES + ref.GPU_CASES
CUS = ref.CENSUS_CUS


def fused_plan(w, h, n=3, cus=CUS, **kw):
    return ref.case_coarse_plan(ref.case("x", w, h, n, **kw), cus)


def test_the_sweep_plan_at_the_boundaries_worked_out_by_hand():
    def short(w, h):
        p = fused_plan(w, h)
        return p["rows_per_sweep"], p["rmax"], p["nk"], p["nk_pad"]

    # the shapes the suite had: chunks 40 -> 12 rows of lanes; 240 level-1 rows in 20 sweeps per frame, 40 in all: no padding
    assert short(640, 480) == (12, 12, 40, 40)
    assert short(672, 464) == (12, 12, 40, 40)            # 42 chunks: 12 rows (504 lanes), 232 rows in 20 sweeps
    assert short(160, 128) == (25, 51, 6, 8)              # 64 rows: 3 sweeps of 25 (8 x 25 = 200 rows loaded; 26 .. 51 rows load more)
    assert short(320, 66) == (12, 25, 6, 8)               # 33 rows: 3 sweeps of 12 (96 rows loaded; 17 rows: 2 sweeps, 136)
    assert short(96, 64) == (42, 85, 2, 8)                # 32 rows in one sweep of any r >= 32: the smallest allowed, 85 / 2
    # 2 chunks: 256 rows of lanes, one sweep per frame whatever r: the smallest allowed (128), 16 rows of 128 used
    assert short(32, 32) == (128, 256, 2, 8)
    # 512 chunks: one row per sweep, every lane busy; 16 rows: 32 sweeps, no padding; 19 rows: 38 sweeps padded to 40
    assert short(8192, 32) == (1, 1, 32, 32) and short(8192, 38) == (1, 1, 38, 40)
    # 256 chunks: two rows per sweep at most, one allowed; 16 rows: r = 2 loads 16 x 2 = 32 rows, r = 1: 32 x 1 = 32 -- the larger;
    # 19 rows: r = 2 takes 10 sweeps per frame, 20 padded to 24 = 48 rows, r = 1 38 padded to 40 = 40 rows
    assert short(4096, 32) == (2, 2, 16, 16) and short(4096, 38) == (1, 2, 38, 40)
    assert short(4112, 32) == (1, 1, 32, 32)              # 257 chunks: one row, 255 lanes idle
    assert int((~ref.coarse_lanes(fused_plan(4112, 32))[2]).sum()) == 255 and ref.coarse_lanes(fused_plan(8192, 32))[2].all()
    assert short(256, 256) == (32, 32, 8, 8)              # 16 chunks: 32 rows, 128 rows in 4 sweeps per frame
    # padding of 6, 4 and 2 sweeps with many sweeps per frame
    for (w, h), pad in (((1040, 290), 6), ((1040, 294), 6), ((1184, 98), 4), ((112, 168), 2)):
        p = fused_plan(w, h)
        assert p["nk_pad"] - p["nk"] == pad and p["nkf"] > 1, (w, h, p)
    # LDS: 2 * 16 * 5007 = 160 224 of frames, 624 keys, 1 088 of histograms and sums = 163 808 of 163 840; two rows more: 163 844
    assert fused_plan(32, 10014)["lds"] == 163808 and fused_plan(32, 10014)["nb"] == 624
    assert fused_plan(32, 10016)["verdict"] == "lds" and ref.coarse_lds(32, 10016, 625) == 163844
    assert fused_plan(8192, 38)["lds"] == 158780 and fused_plan(8192, 40)["verdict"] == "lds"
    assert fused_plan(8208, 32)["verdict"] == "chunks" and ref.coarse_lds(8208, 32, 512) < ref.LDS_LIMIT
    assert fused_plan(528, 272)["nb"] == 512 and fused_plan(448, 320)["nb"] == 513 and fused_plan(32, 32)["nb"] == 1
    assert fused_plan(640, 480)["nb"] == 39 * 29 > 1024


def test_the_launch_geometry_against_the_cu_count():
    for cus in (1, 80, 256, 304):
        # (pairs, workgroups, stagger groups): one workgroup per CU at most, the stagger from two generations on
        for n, wgs, groups in ((1, 1, 1), (cus - 1, cus - 1, 1), (cus, cus, 1), (cus + 1, cus, 1),
                               (2 * cus - 1, cus, 1), (2 * cus, cus, 3), (2 * cus + 1, cus, 3), (3 * cus + 1, cus, 3)):
            if n < 1 or (cus == 1 and n <= 2):     # (one CU: 1 and 2 pairs are CUs and 2 CUs themselves, listed as such)
                continue
            p = fused_plan(64, 48, n, cus)
            assert p["supported"] and (p["wgs"], p["stagger_groups"]) == (wgs, groups), (cus, n, p["wgs"], p["stagger_groups"])
        one = fused_plan(64, 48, 1, 1), fused_plan(64, 48, 2, 1)
        assert [(p["wgs"], p["stagger_groups"]) for p in one] == [(1, 1), (1, 3)]
    assert fused_plan(640, 480)["stagger_ticks"] == 819      # 614 400 bytes at 75 000 per us, in ticks of 10 ns
    assert fused_plan(64, 48)["stagger_ticks"] == 8


def test_every_verdict_is_the_first_condition_that_fails():
    ok = dict(w=64, h=48, pair_stride=64 * 48, prev=ref.BASE, cur=ref.BASE + 4096, grid=ref.dense_grid(64, 48, 1), rng=4, tile=8, search=4,
              subpixel=0, n_pairs=9)
    assert ref.coarse_verdict(**ok) == "ok"
    breaks = dict(tile=dict(tile=16), search=dict(search=3), subpixel=dict(subpixel=1), width=dict(w=72), height=dict(h=47),
                  stride=dict(pair_stride=64 * 48 + 8), chunks=dict(w=8208), prev=dict(prev=ref.BASE + 8), cur=dict(cur=ref.BASE + 4100),
                  grid=dict(grid=(5, 5, 8, 8, 2, 1)), bins=dict(rng=16), pairs=dict(n_pairs=1 << 31), lds=dict(w=640, h=512, grid=ref.dense_grid(640, 512, 1)))
    names = list(breaks)
    assert names == list(ref.VERDICTS[1:])
    for i, name in enumerate(names):
        assert ref.coarse_verdict(**{**ok, **breaks[name]}) == name
        later = dict(ok)
        for other in names[i:]:      # with every later condition broken as well the first one still names the verdict
            if not (name == "width" and other == "chunks") and not (other == "lds"):
                later.update(breaks[other])
        later.update(breaks[name])
        assert ref.coarse_verdict(**later) == name, (name, later)


def test_the_strip_plan_at_the_boundaries_worked_out_by_hand():
    def short(w, h, n=3, **kw):
        p = ref.case_pyramid_plan(ref.case("x", w, h, n, split=True, **kw))
        return p["vec"], p["rows_per_strip"], p["nstrips"], p["units"], p["total"], p["zero_words"]

    assert short(640, 480) == (1, 25, 10, 6, 60, 12)            # 40 chunks: 25 rows per strip, 240 rows in 10 strips
    assert short(32, 32) == (1, 512, 1, 6, 6, 12)               # 2 chunks: 512 rows asked, 16 there: one strip of 32 items
    assert short(48, 1040) == (1, 341, 2, 6, 12, 12)            # 3 chunks: 341 rows (1 023 items), 520 rows: 341 + 179
    assert short(16384, 32) == (1, 1, 16, 6, 96, 12)            # 1 024 chunks: one row per strip
    assert short(16400, 32) == (1, 1, 16, 6, 96, 12)            # 1 025 chunks: 1024 / 1025 = 0 rows, clamped to one: 1 025 items
    assert short(64, 1024) == (1, 256, 2, 6, 12, 12) and short(64, 514) == (1, 256, 2, 6, 12, 12)
    assert short(50, 46) == (0, 0, 1, 6, 6, 12)                 # 25 x 23 = 575 cells
    assert short(63, 64, levels=1) == (0, 0, 1, 6, 6, 12)       # 32 x 32 = 1 024 cells: one workgroup, four trips
    assert short(82, 50) == (0, 0, 2, 6, 12, 12)                # 41 x 25 = 1 025 cells: two workgroups
    assert short(40, 512) == (0, 0, 5, 6, 30, 12)
    assert short(64, 48, 5, sequence=True) == (1, 256, 1, 6, 6, 20)    # 6 frames, 5 pairs of sums
    assert short(64, 48, 1, sequence=True) == (1, 256, 1, 2, 2, 4)
    assert short(64, 48, mean_subtract=0)[5] == 0
    # each of the five conditions alone sends a 64 x 48 frame to the scalar kernel; in a sequence `cur` is not looked at
    for kw, why in ((dict(stride_extra=8), "stride"), (dict(prev_off=4), "prev"), (dict(cur_off=4), "cur")):
        p = ref.case_pyramid_plan(ref.case("x", 64, 48, 3, **kw))
        assert not p["vec"] and [k for k, v in p["scalar_by"].items() if v] == [why]
    assert ref.pyramid_plan(64, 48, 64 * 48, ref.BASE, ref.BASE + 4, 1, 4)["vec"] == 1


def test_sequence_frames_reach_one_or_two_records():
    pl = ref.pyramid_plan(64, 48, 64 * 48, ref.BASE, ref.BASE + 64 * 48, 1, 6)
    assert ref.sums_targets(pl, 0) == [(0, 0)] and ref.sums_targets(pl, 5) == [(4, 1)]
    assert all(ref.sums_targets(pl, f) == [(f, 0), (f - 1, 1)] for f in range(1, 5))
    hit = sorted(t for f in range(6) for t in ref.sums_targets(pl, f))
    assert hit == sorted((p, s) for p in range(5) for s in (0, 1))
    two = ref.pyramid_plan(64, 48, 64 * 48, ref.BASE, ref.BASE + 64 * 48, 1, 2)
    assert ref.sums_targets(two, 0) == [(0, 0)] and ref.sums_targets(two, 1) == [(0, 1)]
    plain = ref.pyramid_plan(64, 48, 64 * 48, ref.BASE, ref.BASE + 4096, 0, 3)
    assert [ref.sums_targets(plain, u) for u in range(6)] == [[(0, 0)], [(0, 1)], [(1, 0)], [(1, 1)], [(2, 0)], [(2, 1)]]


@pytest.mark.parametrize("c", EVERY_CASE, ids=lambda c: c["id"])
def test_coverage_of_the_decode_that_serves_the_case(c):
    kind = ref.coarse_kind(c)
    if kind == "fused":
        pl = ref.case_coarse_plan(c)
        w, h = c["w"], c["h"]
        assert pl["nk_pad"] % (2 * ref.UNROLL) == 0 and pl["nk"] <= pl["nk_pad"] < pl["nk"] + 2 * ref.UNROLL
        assert pl["rows_per_sweep"] * (w // 16) <= ref.THREADS and pl["lds"] <= ref.LDS_LIMIT
        cov = ref.coarse_coverage(pl)
        assert (cov["lds"] == 1).all(), "every level-1 pixel of prev and cur is written to LDS by exactly one (lane, sweep)"
        assert (cov["summed"] == 1).all(), "every level-0 byte enters the sums exactly once"
        assert cov["lo"] == 0 and cov["hi"] == w * h
        # the pair loop: what the filter is handed is what was loaded for it, and loads ahead go to the next pair's first two batches
        n = ref.n_pairs_of(c)
        for block in sorted({0, 1, pl["wgs"] // 2, pl["wgs"] - 1} & set(range(pl["wgs"]))):
            filtered, ahead = ref.coarse_walk(pl, n, block)
            pairs = list(range(block, n, pl["wgs"]))
            assert [f[:2] for f in filtered] == [(p, k0) for p in pairs for k0 in range(0, pl["nk_pad"], ref.UNROLL)]
            for pair, k0, tags, which in filtered:
                assert tags == [(pair, k0 + u) for u in range(ref.UNROLL)], (block, pair, k0, tags)
                assert which == pairs.index(pair) % 2
            assert len(ahead) == 2 * len(pairs)
            for pair, nxt, tags in ahead:
                assert nxt == (pair + pl["wgs"] if pair + pl["wgs"] < n else pair)
                assert all(p == nxt and 0 <= k < 2 * ref.UNROLL for p, k in tags)
            assert sorted(k for _, _, tags in ahead[:2] for _, k in tags) == list(range(2 * ref.UNROLL))
    elif kind == "k1":
        pl = ref.case_pyramid_plan(c)
        assert pl["nstrips"] >= 1 and pl["total"] < 2 ** 31 and (not pl["vec"] or pl["rows_per_strip"] >= 1)
        cov = ref.k1_coverage(pl)
        assert (cov["out"] == 1).all(), "every level-1 pixel is written once"
        assert (cov["summed"] == 1).all(), "every level-0 byte is summed once, the odd last column and row included"
        units = pl["units"]
        hits = sorted(t for u in range(units) for t in ref.sums_targets(pl, u))
        assert hits == sorted((p, s) for p in range(ref.n_pairs_of(c)) for s in (0, 1)), "every record gets its two frames once"
    else:
        assert kind == "small" and "small_class" in c["paths"]


def test_padding_sweeps_are_dropped_by_their_row_alone():
    """k_coarse drops a sweep's rows on `y1 < h1 && k < nk`.  Sweeps nk .. nk_pad - 1 count on from cur's last sweep, so
    their rows start at nkf * rpi >= h1: the row test alone drops them, and `k < nk` never decides (a model without it
    passes every coverage test).  Held here so that a sweep order in which it WOULD decide does not arrive unnoticed."""
    fused = [c for c in EVERY_CASE if ref.coarse_kind(c) == "fused"]
    padded = 0
    for c in fused:
        pl = ref.case_coarse_plan(c)
        for k in range(pl["nk"], pl["nk_pad"]):
            s = ref.coarse_sweep(pl, k)
            assert s["frame"] == 1 and (s["y1"] >= c["h"] // 2).all() and not s["kept"].any(), (c["id"], k)
            padded += 1
        last = ref.coarse_sweep(pl, pl["nk"] - 1)     # the last real sweep keeps something, all of it unless it is partial
        assert last["kept"].any()
    assert padded > 60


@pytest.mark.parametrize("c", ref.GPU_CASES, ids=lambda c: c["id"])
def test_every_device_case_reaches_the_paths_it_is_listed_for(c):
    assert c["paths"], "a case without a path has no reason to be in the list"
    got = ref.reach(c)
    assert set(c["paths"]) <= set(ref.VOCABULARY), set(c["paths"]) - set(ref.VOCABULARY)
    assert set(c["paths"]) <= got, (c["id"], sorted(set(c["paths"]) - got))
    assert got <= set(ref.VOCABULARY), got - set(ref.VOCABULARY)
    for cus in (CUS, 304, 64):
        assert ref.device_bytes(c, cus) <= 125 * 10 ** 6
    # small grids stay out of the small class by their pair count
    g0 = ref.dense_grid(c["w"], c["h"], 0, c["tile"], c["search"], c["subpixel"])
    if g0[4] * g0[5] <= 256 and "small_class" not in c["paths"] and not c["sequence"] and not isinstance(c["n_pairs"], tuple):
        assert c["n_pairs"] >= 129, c["id"]
    if "small_class" not in c["paths"]:   # (64 x 48 at any pair count: six level-1 blocks are too few for the grouped search)
        assert all(ref.coarse_kind(c, cus) != "small" for cus in (1, 64, CUS, 304)), c["id"]
    # the kernels that make the pass, as the device test asserts them with the launch counters
    want = ref.counters(c)
    if "fused" in got:
        assert want == dict(K_PYRAMID=1, K_SEARCH_L1=0, K_REDUCE_L1=0)
    if "two_levels_k1" in got:
        assert want["K_PYRAMID"] == 1 and want["K_SEARCH_L1"] == 1
    if "small_class" in got:
        assert want["K_PYRAMID"] == 0


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


def test_the_old_parity_rows_take_the_kernels_the_model_says():
    """tests/test_gpu_parity.py::test_fused_coarse_kernel_equals_the_split_kernels at seven pairs: 96 x 96 (121 and 25
    blocks) is a small-class batch; 48 x 32 has two level-1 blocks, too few for the grouped search, and runs k_coarse."""
    assert ref.coarse_kind(ref.case("x", 96, 96, 7)) == "small" and ref.coarse_kind(ref.case("x", 96, 96, 129)) == "fused"
    assert ref.coarse_kind(ref.case("x", 48, 32, 7)) == "fused"
    for w, h in ((160, 128), (640, 480), (320, 66), (672, 464)):
        assert ref.coarse_kind(ref.case("x", w, h, 7)) == "fused"
        assert ref.coarse_kind(ref.case("x", w, h, 7, split=True)) == "k1"


def test_the_frames_of_the_device_cases_are_what_the_cases_say(aof, orc, synth):
    """The parameter check takes every case; the generation cases' contents differ between consecutive pairs of a
    workgroup in pixel sums, delta, gated blocks and level-1 records, and hold the orderings the two histogram sets and
    the key array are there for; the edge cases' last column and row move the rounded mean."""
    for c in ref.GPU_CASES:
        p = aof.default_params(c["w"], c["h"], **ref.params_kw(c))
        assert aof.check_params(p) == 0, c["id"]
        for level in range(c["levels"]):
            assert tuple(aof.grid(p, level)) == ref.dense_grid(c["w"], c["h"], level, c["tile"], c["search"], c["subpixel"]), c["id"]
    c = ref.GENERATIONS[-1]
    facts = ref.oracle_facts(aof, orc, synth, c)
    for n in (2 * CUS - 1, 2 * CUS, 2 * CUS + 1, 3 * CUS + 1):
        ref.check_chains(facts, ref.pair_contents(n, len(facts), CUS), CUS, orderings=True)
    ref.check_chains(facts, ref.pair_contents(CUS + 1, len(facts), CUS), CUS, orderings=False)
    edges = [c for c in ref.GPU_CASES if c["edge"]]
    assert len(edges) >= 4
    for c in edges:
        prevs, curs, _ = ref.distinct_frames(c, synth)
        ref.check_edge_moves_delta(c, prevs, curs)
