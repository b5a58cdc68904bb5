"""Every path from block records to the 16-byte flow record, held to designed motion fields (tests/vote_field_ref.py):
blocks, half-pixel directions and flow records byte for byte against the oracle, and the flow records against
reduce_model as well.  Each case first asserts, on the ORACLE's records, that its field reaches the branches it is
there for (vote_field_ref.check_reaches), then runs the device, then asserts with the profiling counters which kernel
finalised.  Large launches are replicas of the few distinct designed pairs.

Which launch takes which search, coarse pass and in-launch reduction is the batch plan's rule: csrc/aof_batch_plan.hpp
(plan_batch, choose_lane8) and its model tests/batch_plan_ref.py (DESIGN.md "Which kernel serves which configuration").
Behind a search that does not reduce itself K3 chooses its own form (k_reduce.hip launch_reduce, aof_params.cpp
reduce_chunks):

  more than 256 blocks                     1 024 lanes per pair for up to 512 pairs of at least 2 048 blocks, 512 lanes
                                           for up to 1 024 such pairs, else 256 lanes
  more than 8 192 blocks                   k_reduce_chunk over ceil(blocks / 4 096) chunks of ceil(blocks / chunks)
                                           records, then k_reduce on the parts
  grids of 8..256 blocks                   K3's one-wave-per-pair form, behind the generic search (force_generic) and
                                           behind the 16x16 search
  more than 64 bins (two levels, S >= 5)   K3 hands the bins to one thread: finalise_flow
"""
import numpy as np
import pytest

import cols_plan_ref
import vote_field_ref as vf
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

_CACHE = {}


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def tiled(torch, arr, reps, device):
    t = torch.from_numpy(arr).to(device)
    return t.repeat((reps,) + (1,) * (t.dim() - 1)).contiguous()


def assert_replicas(aof, blocks, flows, ref, what, sub=None):
    """Launch entry i against distinct pair i % k of the oracle's (blocks, flows, subdirs)."""
    rb, rf, rs = ref
    gb, gf = aof.blocks_view(blocks), aof.flows_view(flows)
    gs = sub.cpu().numpy() if sub is not None else None
    for i in range(gb.shape[0]):
        j = i % rb.shape[0]
        assert gb[i].tobytes() == rb[j].tobytes(), (what, i, np.flatnonzero(gb[i] != rb[j])[:8])
        if gs is not None:
            bad = np.flatnonzero(gs[i] != rs[j])
            assert bad.size == 0, (what, i, bad[:8], gs[i][bad[:8]], rs[j][bad[:8]])
        assert gf[i].tobytes() == rf[j].tobytes(), (what, i, gf[i], rf[j])


def stack_refs(rs, subdirs):
    return (np.stack([r["blocks"] for r in rs]), np.stack([r["flow"] for r in rs]),
            np.stack([r["subdirs"] for r in rs]) if subdirs else None)


def one_level(aof, orc, case, sub, name):
    """The distinct pairs of a case and design with the oracle's records, made and checked once: the oracle votes as
    designed, its flow records are reduce_model's, and the field reaches what the design is there for."""
    key = (case, sub, name)
    if key not in _CACHE:
        p = vf.one_level_params(aof.default_params, case, sub)
        po = orc.params_from(p)
        pairs = vf.one_level_pairs(p, case, name)
        rs = [orc.flow_pair(po, prev, cur) for _, prev, cur in pairs]
        cs = []
        for (d, _, _), r in zip(pairs, rs):
            got = vf.design_of_records(p, r["blocks"], r["subdirs"])
            assert vf.same_field(p, d, got) == [], key
            assert same_bytes(vf.reduce_model(d, p), r["flow"]), key
            cs.append(vf.census(got, p))
        vf.check_reaches(name, p, cs)
        models = np.stack([vf.reduce_model(d, p) for d, _, _ in pairs])
        _CACHE[key] = (p, np.stack([x[1] for x in pairs]), np.stack([x[2] for x in pairs]), stack_refs(rs, bool(sub)), models, cs)
    return _CACHE[key]


KERNELS = ("K_PYRAMID", "K_SEARCH_L1", "K_REDUCE_L1", "K_SEARCH", "K_REDUCE")


def run(aof, torch, device, p, prevs, curs, n_pairs, setup=None):
    """One launch of n_pairs pairs, replicas of the distinct ones: (blocks, flows, subdirs, {kernel: launches})."""
    eng = aof.FlowEngine(p, 0)
    if setup:
        setup(eng)
    reps = -(-n_pairs // prevs.shape[0])
    tp, tc = tiled(torch, prevs, reps, device), tiled(torch, curs, reps, device)
    sub = torch.full((n_pairs, eng.nblocks(0)), 0x77, dtype=torch.uint8, device=device) if p.subpixel else None
    eng.set_profiling(True)
    blocks, flows, _ = eng.flow_batch(tp, tc, subdirs=sub, n_pairs=n_pairs)
    torch.cuda.synchronize()
    launches = {k: len(eng.profile_ms(getattr(aof, k))) for k in KERNELS}
    eng.set_profiling(False)
    variant = eng.variant
    eng.close()
    return blocks, flows, sub, launches, variant


def hold(aof, what, blocks, flows, sub, ref, models):
    """Device against the oracle (records, directions, flow records) and against reduce_model (flow records)."""
    assert_replicas(aof, blocks, flows, ref, what, sub)
    gf = aof.flows_view(flows)
    for i in range(gf.shape[0]):
        assert same_bytes(gf[i], models[i % models.shape[0]]), (what, i, gf[i], models[i % models.shape[0]])


def k3_lanes(n_pairs, nblocks):
    """launch_reduce's choice (the chunked form apart)."""
    if nblocks <= 256:
        return 64
    if nblocks >= 2048 and n_pairs <= 512:
        return 1024
    if nblocks >= 2048 and n_pairs <= 1024:
        return 512
    return 256


def ids(rows):
    return ["-".join(str(v) for v in r) for r in rows]


# ---- one level, 8x8 +-4 ------------------------------------------------------------------------------------------------
SMALL = [(case, sub, name) for case in ("b108", "b81", "b90", "b99") for sub in (0, 1) for name in vf.designs_of(case, sub)]


@pytest.mark.parametrize("case,sub,name", SMALL, ids=ids(SMALL))
def test_grids_of_up_to_256_blocks(aof, orc, gpu_device, case, sub, name):
    """nblocks % 4 = 0, 1, 2, 3.  The grouped search's own tail; then K3 with one wave per pair behind the generic search,
    whose quads, tail records and `subdirs` words these are."""
    import torch
    p, prevs, curs, ref, models, cs = one_level(aof, orc, case, sub, name)
    n = prevs.shape[0]
    assert cs[0]["blocks"] == vf.ONE_LEVEL[case]["blocks"] <= 256 and cs[0]["tail"] == cs[0]["blocks"] % 4
    blocks, flows, s, launches, variant = run(aof, torch, gpu_device, p, prevs, curs, n)
    assert variant == "lane8" and launches["K_SEARCH"] == 1 and launches["K_REDUCE"] == 0, (launches, variant)
    hold(aof, (case, sub, name, "grouped"), blocks, flows, s, ref, models)
    blocks, flows, s, launches, variant = run(aof, torch, gpu_device, p, prevs, curs, n, lambda e: e.force_generic(True))
    assert variant == "generic" and launches["K_REDUCE"] == 1 and k3_lanes(n, cs[0]["blocks"]) == 64, (launches, variant)
    hold(aof, (case, sub, name, "K3, one wave per pair"), blocks, flows, s, ref, models)


NARROW = [("b432", sub, name) for sub in (0, 1) for name in vf.designs_of("b432", sub)]


@pytest.mark.parametrize("case,sub,name", NARROW, ids=ids(NARROW))
def test_k3_with_256_lanes(aof, orc, gpu_device, case, sub, name):
    """432 blocks: the flat search and K3, then the generic search's writers of records and directions and the same K3."""
    import torch
    p, prevs, curs, ref, models, cs = one_level(aof, orc, case, sub, name)
    n = prevs.shape[0]
    for generic in (False, True):
        blocks, flows, s, launches, variant = run(aof, torch, gpu_device, p, prevs, curs, n, lambda e: e.force_generic(generic))
        assert variant == ("generic" if generic else "lane8") and launches["K_REDUCE"] == 1, (launches, variant)
        assert k3_lanes(n, 432) == 256
        hold(aof, (case, sub, name, variant), blocks, flows, s, ref, models)


WIDE = [(case, n, name) for case, ns in (("b2048", (4, 512, 513, 1024)), ("b2016", (4,))) for n in ns for name in vf.WIDE]


@pytest.mark.parametrize("case,n_pairs,name", WIDE, ids=ids(WIDE))
def test_k3_with_512_and_1024_lanes(aof, orc, gpu_device, case, n_pairs, name):
    """520x264 is exactly 2 048 blocks, the boundary: 1 024 lanes up to 512 pairs, 512 lanes up to 1 024; 512x264 (2 016
    blocks) stays at 256 lanes."""
    import torch
    p, prevs, curs, ref, models, cs = one_level(aof, orc, case, 0, name)
    lanes = k3_lanes(n_pairs, cs[0]["blocks"])
    assert lanes == {("b2048", 4): 1024, ("b2048", 512): 1024, ("b2048", 513): 512, ("b2048", 1024): 512, ("b2016", 4): 256}[(case, n_pairs)]
    blocks, flows, s, launches, variant = run(aof, torch, gpu_device, p, prevs, curs, n_pairs)
    assert variant == "lane8" and launches["K_REDUCE"] == 1 and flows.shape[0] == n_pairs, (launches, variant)
    hold(aof, (case, n_pairs, name, lanes), blocks, flows, s, ref, models)


CHUNKED = [(case, sub, name) for case in ("b8320", "b8192") for sub in (0, 1) for name in vf.ONE_LEVEL[case]["designs"]]


@pytest.mark.parametrize("case,sub,name", CHUNKED, ids=ids(CHUNKED))
def test_k3_in_chunks_and_its_neighbour(aof, orc, gpu_device, case, sub, name):
    """8 320 blocks: three chunks of 2 774 records, the last one 2 772 (a count that the chunks do not divide);
    8 192 blocks: the largest grid that K3 takes in one step."""
    import torch
    p, prevs, curs, ref, models, cs = one_level(aof, orc, case, sub, name)
    assert cs[0]["chunks"] == (3 if case == "b8320" else 0)
    if cs[0]["chunks"]:
        assert cs[0]["chunk_sizes"] == [2774, 2774, 2772]
    blocks, flows, s, launches, variant = run(aof, torch, gpu_device, p, prevs, curs, prevs.shape[0])
    assert variant == "lane8" and launches["K_REDUCE"] == 1, (launches, variant)
    hold(aof, (case, sub, name), blocks, flows, s, ref, models)


EXHAUSTIVE = ("one", "checker", "odd-one-out", "silent-rows", "uniform-random", "min-valid")
WALK = ("rows", "row-once", "aba-rows", "cols", "silent-rows", "odd-one-out", "checker")
LONG_WALKS = 2048      # pairs of 200x152 (all that the context's vote memory holds) at which cols_plan_make gives segments of 8 rows
IN_LAUNCH = [(case, sub, mode, name) for case, sub in (("b432", 0), ("b432", 1), ("vga", 0))
             for mode, names in (("exhaustive", EXHAUSTIVE), ("pruned", WALK)) for name in names]


@pytest.mark.parametrize("case,sub,mode,name", IN_LAUNCH, ids=ids(IN_LAUNCH))
def test_reduction_in_the_search_launch(aof, orc, gpu_device, case, sub, mode, name):
    """vote_and_arrive (exhaustive; and the half-pixel column walk) and WalkVotes (the column walk) with their finaliser
    wave: no K3 launch, and the K3 run's bytes."""
    import torch
    p, prevs, curs, ref, models, cs = one_level(aof, orc, case, sub, name)
    search = aof.SEARCH_EXHAUSTIVE if mode == "exhaustive" else aof.SEARCH_PRUNED
    n = prevs.shape[0]
    b3, f3, s3, launches, variant = run(aof, torch, gpu_device, p, prevs, curs, n, lambda e: e.set_search_mode(search))
    assert variant == "lane8" and launches["K_REDUCE"] == 1, (launches, variant)
    hold(aof, (case, sub, mode, name, "K3"), b3, f3, s3, ref, models)

    def fused(e):
        e.set_search_mode(search)
        e.set_reduce_fusion(True)
    blocks, flows, s, launches, variant = run(aof, torch, gpu_device, p, prevs, curs, n, fused)
    assert launches["K_SEARCH"] == 1 and launches["K_REDUCE"] == 0, (launches, "the reduction ran in the search launch")
    assert torch.equal(flows, f3) and torch.equal(blocks, b3) and (s is None or torch.equal(s, s3))
    hold(aof, (case, sub, mode, name, "in the launch"), blocks, flows, s, ref, models)
    if (case, sub, mode) == ("b432", 0, "pruned"):
        # two pairs walk their columns two rows at a time (aof_cols8_plan.hpp: short segments fill the device); 2 048
        # replicas walk eight rows: A, B, A and silent steps inside ONE walk
        plan = cols_plan_ref.plan(24, 18, LONG_WALKS)
        assert plan["head"]["len"] == 8 and plan["tail_pairs"] == 0 and cols_plan_ref.plan(24, 18, n)["head"]["len"] == 2
        blocks, flows, s, launches, variant = run(aof, torch, gpu_device, p, prevs, curs, LONG_WALKS, fused)
        assert launches["K_SEARCH"] == 1 and launches["K_REDUCE"] == 0, launches
        hold(aof, (case, sub, mode, name, "in the launch, long walks"), blocks, flows, s, ref, models)


SMALL_CLASS = [(case, n, name) for case in ("px4", "small99") for n in (1, 128, 129, 304) for name in vf.ONE_LEVEL[case]["designs"]]


@pytest.mark.parametrize("case,n_pairs,name", SMALL_CLASS, ids=ids(SMALL_CLASS))
def test_small_pairs(aof, orc, gpu_device, case, n_pairs, name):
    """The 64x64 PX4Flow grid (5 x 5 tiles, step 10, half-pixel refinement) and a dense 96x80: up to 128 pairs in
    k_flow_small, more in the grouped search; both finalise themselves."""
    import torch
    sub = 1 if case == "px4" else 0
    p, prevs, curs, ref, models, cs = one_level(aof, orc, case, sub, name)
    if n_pairs == 1:
        prevs, curs, models = prevs[:1], curs[:1], models[:1]
        ref = tuple(None if r is None else r[:1] for r in ref)
    blocks, flows, s, launches, variant = run(aof, torch, gpu_device, p, prevs, curs, n_pairs)
    assert launches == dict(K_PYRAMID=0, K_SEARCH_L1=0, K_REDUCE_L1=0, K_SEARCH=1, K_REDUCE=0), launches
    assert flows.shape[0] == n_pairs
    hold(aof, (case, n_pairs, name), blocks, flows, s, ref, models)


# ---- 16x16 tiles, one level ------------------------------------------------------------------------------------------
TILE16 = [("t16", sub, name) for sub in (0, 1) for name in vf.ONE_LEVEL["t16"]["designs"]]


@pytest.mark.parametrize("case,sub,name", TILE16, ids=ids(TILE16))
def test_16x16_tiles_through_k3(aof, orc, gpu_device, case, sub, name):
    """63 blocks, +-8: 35 bins, peaks at bins 0 and 34 with half-pixel refinement; K3 with one wave per pair."""
    import torch
    p, prevs, curs, ref, models, cs = one_level(aof, orc, case, sub, name)
    assert cs[0]["bins"] == 35 and cs[0]["blocks"] == 63
    blocks, flows, s, launches, variant = run(aof, torch, gpu_device, p, prevs, curs, prevs.shape[0])
    assert variant != "lane8" and launches["K_REDUCE"] == 1, (launches, variant)
    hold(aof, (case, sub, name, variant), blocks, flows, s, ref, models)


# ---- two levels ------------------------------------------------------------------------------------------------------
def two_level_launches(case, split):
    if case == "c96":      # 99 and 20 blocks: k_flow_small, or K1 and two grouped searches
        return dict(K_PYRAMID=1, K_SEARCH_L1=1, K_REDUCE_L1=0, K_SEARCH=1, K_REDUCE=0) if split else \
            dict(K_PYRAMID=0, K_SEARCH_L1=0, K_REDUCE_L1=0, K_SEARCH=1, K_REDUCE=0)
    if case == "c208":     # 450 and 96 blocks: k_coarse, or K1 and the grouped level-1 search; level 0 flat with K3
        return dict(K_PYRAMID=1, K_SEARCH_L1=1 if split else 0, K_REDUCE_L1=0, K_SEARCH=1, K_REDUCE=1)
    return dict(K_PYRAMID=1, K_SEARCH_L1=1, K_REDUCE_L1=1, K_SEARCH=1, K_REDUCE=1)      # +-5 and 16x16: K3 at both levels


def two_level(aof, orc, case, kind, name, hist_filter=1):
    key = (case, kind, name, hist_filter)
    if key not in _CACHE:
        p = vf.two_level_params(aof.default_params, case, hist_filter=hist_filter)
        po = orc.params_from(p)
        rs, models, cs = [], [], []
        if kind == "level1":
            pairs = vf.level1_pairs(p, case, name)
            for d1, prev, cur in pairs:
                r = orc.flow_pair(po, prev, cur, want_l1=True)
                got1 = vf.design_of_records(p, r["blocks_l1"], None, 1)
                assert vf.same_field(p, d1, got1) == [], key
                c = vf.census(got1, p, 1)
                if name != "pred-3.0":
                    assert c["pred_half_x"] and c["pred_half_y"], key
                else:
                    assert c["pred_negative_x"] != c["pred_negative_y"] and not c["pred_half_x"], key
                m1 = vf.reduce_model(d1, p, 1)
                assert (r["flow"]["pred_x"], r["flow"]["pred_y"]) == (m1["pred_x"], m1["pred_y"]), key
                models.append(vf.pair_model(p, vf.design_of_records(p, r["blocks"], None, 0), d1))
                rs.append(r)
            frames = [(x[1], x[2]) for x in pairs]
        else:
            pairs = vf.residual_pairs(p, case, name)
            for d0, P, prev, cur in pairs:
                r = orc.flow_pair(po, prev, cur)
                got = vf.design_of_records(p, r["blocks"], None, 0)
                assert vf.same_field(p, d0, got) == [] and (r["flow"]["pred_x"], r["flow"]["pred_y"]) == P, key
                cs.append(vf.census(got, p))
                assert cs[-1]["bins"] == vf.TWO_LEVEL[case].get("bins", 55) and cs[-1]["serial"] == (cs[-1]["bins"] > 64)
                models.append(vf.pair_model(p, d0, P=P))
                rs.append(r)
            vf.check_reaches(name, p, cs)
            frames = [(x[2], x[3]) for x in pairs]
        for m, r in zip(models, rs):
            assert same_bytes(m, r["flow"]), (key, m, r["flow"])
        _CACHE[key] = (p, np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), stack_refs(rs, False), np.stack(models))
    return _CACHE[key]


def hold_two_level(aof, torch, device, case, what, p, prevs, curs, ref, models, splits):
    for split in splits:
        blocks, flows, s, launches, variant = run(aof, torch, device, p, prevs, curs, prevs.shape[0],
                                                  lambda e: e.set_split_coarse(split))
        assert launches == two_level_launches(case, split), (what, split, launches)
        hold(aof, what + (split,), blocks, flows, s, ref, models)


PREDICTORS = [(case, hf, field) for case in sorted(vf.TWO_LEVEL) for hf in (1, 0) for field in sorted(vf.LEVEL1_FIELDS)]


@pytest.mark.parametrize("case,hist_filter,field", PREDICTORS, ids=ids(PREDICTORS))
def test_predictor_of_a_level1_field(aof, orc, gpu_device, case, hist_filter, field):
    """floor_div(2 v + w, 2 w) - centre at exactly +-2.5 and +-3.5 (half up: -2 and +3, -3 and +4; negated: +3 and -2),
    and for the plain average a negative, inexact quotient (pred-3.0), in k_flow_small, k_coarse, the grouped level-1
    search and K3."""
    import torch
    p, prevs, curs, ref, models = two_level(aof, orc, case, "level1", field, hist_filter)
    want = {"pred-2.5": [(-2, 3), (3, -2), (-2, 3)], "pred-3.5": [(-3, 4), (4, -3), (-3, 4)], "pred-3.0": [(-3, 3), (3, -3), (-3, 3)]}
    assert [(int(m["pred_x"]), int(m["pred_y"])) for m in models] == want[field]
    hold_two_level(aof, torch, gpu_device, case, (case, hist_filter, field), p, prevs, curs, ref, models,
                   (False, True) if case.startswith("c") else (False,))


RESIDUALS = [(case, name) for case in sorted(vf.TWO_LEVEL) for name in vf.RESIDUALS]


@pytest.mark.parametrize("case,name", RESIDUALS, ids=ids(RESIDUALS))
def test_level0_votes_under_a_predictor(aof, orc, gpu_device, case, name):
    """Residuals around P at level 0: 55 bins through the wave finaliser (96x80, 208x152), 67 and 103 bins through the
    one-thread walk (8x8 +-5, 16x16 +-8): a tie, a spread window, the lowest and highest votes the two searches reach,
    min_valid and min_valid + 1 voters."""
    import torch
    p, prevs, curs, ref, models = two_level(aof, orc, case, "residual", name)
    hold_two_level(aof, torch, gpu_device, case, (case, name), p, prevs, curs, ref, models,
                   (False, True) if case.startswith("c") else (False,))
