"""The 16x16 search at every edge of its block-row plan (tests/tile16_rows_ref.py: CASES), against the oracle byte for byte.

Every case runs the exhaustive scan, the pruned search and the adaptive search under each forced verdict 0 .. 4 on the SAME
frames: records and flows always, directions with half-pixel refinement, level-1 records with two levels; every pruned run
also against the exhaustive run's bytes.  Outputs and workspace are junk on entry; the frames sit in one arena between
guard zones, the last pair's last byte against one, and frames and guards must hold afterwards what they held.  The last
test holds the union of the walked cases' paths to the model's vocabulary."""
import time

import numpy as np
import pytest

import batch_plan_ref as plan_ref
import tile16_rig as rig
import tile16_rows_ref as ref
from plan_rig import time_limit   # noqa: F401  (this module's fixture too: every test under a limit of its own)
from tile16_rig import assert_matches, run

pytestmark = pytest.mark.gpu

KERNELS = ("K_PYRAMID", "K_SEARCH_L1", "K_REDUCE_L1", "K_SEARCH", "K_REDUCE")
_oracle, _walked = {}, {}


def oracle_of(aof, orc, synth, c, k):
    """(params, prevs, curs, names, the oracle's records) of batch k of a case, computed once."""
    if (c["id"], k) not in _oracle:
        p = rig.case_params(aof, c)
        assert aof.check_params(p) == 0
        prevs, curs, names = rig.case_frames(c, synth, ref, k)
        refs = rig.oracle_refs(orc, p, prevs, curs)
        for a in (prevs, curs):
            a.setflags(write=False)
        _oracle[(c["id"], k)] = (p, prevs, curs, names, refs)
    return _oracle[(c["id"], k)]


def planned(c, n, mode):
    """The batch plan of the case's launch (level 1 searched by a kernel of its own, so that its records can be read)."""
    pl = plan_ref.plan(plan_ref.call(c["id"], c["w"], c["h"], n, tile=16, search=8, subpixel=c["sub"], levels=c["levels"], mean_subtract=c["eq"],
                                     mode=mode, split=c["levels"] == 2))
    return pl, plan_ref.tile16_plan(pl["a0"], forced=1 if mode == plan_ref.ADAPTIVE else 0)


def walk(aof, torch, device, c, k, p, prevs, curs, names, refs):
    """Every form on one batch.  Returns the launches of the exhaustive run by profiling counter."""
    n, two = prevs.shape[0], c["levels"] == 2
    arena = rig.FrameArena(torch, device, prevs, curs)
    eng = aof.FlowEngine(p, 0)
    assert eng.variant == "tile16_lds" and eng.search_mode == aof.SEARCH_ADAPTIVE
    if two:
        eng.set_split_coarse(True)
    eng.set_search_mode(aof.SEARCH_EXHAUSTIVE)
    eng.set_profiling(True)
    ex = run(aof, eng, p, arena.tp, arena.tc, device)
    counts = {name: len(eng.profile_ms(getattr(aof, name))) for name in KERNELS}
    eng.set_profiling(False)
    arena.assert_untouched((c["id"], k, "exhaustive"))
    assert_matches(ex, refs, names, "exhaustive", two)
    eng.set_search_mode(aof.SEARCH_PRUNED)
    got = run(aof, eng, p, arena.tp, arena.tc, device)
    arena.assert_untouched((c["id"], k, "pruned"))
    assert_matches(got, refs, names, "pruned", two, ex)
    eng.set_search_mode(aof.SEARCH_ADAPTIVE)
    for v in ref.HINTS:
        got = run(aof, eng, p, arena.tp, arena.tc, device, [v])
        arena.assert_untouched((c["id"], k, v))
        assert_matches(got, refs, names, f"verdict {v}", two, ex)
        assert (got["hints"] == (v | rig.PATTERN)).all(), (v, [hex(x) for x in got["hints"]])
    eng.close()
    return counts


def scrub(aof, torch, device, p, shape):
    """One launch of the same shape on frames of 0xFF: whatever a later launch fails to stage is not, by luck, what an
    earlier launch of the same frames left in LDS."""
    eng = aof.FlowEngine(p, 0)
    white = torch.full(shape, 0xFF, dtype=torch.uint8, device=device)
    run(aof, eng, p, white, white.clone(), device)
    eng.close()


@pytest.mark.parametrize("c", ref.CASES, ids=lambda c: c["id"])
def test_block_row_case(aof, orc, synth, gpu_device, c):
    import torch
    t0 = time.perf_counter()
    reached = set()
    for k in range(c["batches"]):
        p, prevs, curs, names, refs = oracle_of(aof, orc, synth, c, k)
        n = prevs.shape[0]
        assert n == ref.batch_pairs(c, k) and (n <= 4 or c["id"].startswith(("place-", "shifts-x")))
        # the plan: the 16x16 kernel at level 0 in every mode, inside its LDS; level 1 by the kernel the batch plan names
        for mode in (plan_ref.EXHAUSTIVE, plan_ref.PRUNED, plan_ref.ADAPTIVE):
            pl, t16 = planned(c, n, mode)
            assert pl["valid"] and pl["kind"][0] == "tile16" and t16["verdict"] == "ok" and pl["prune"][0] == mode, (mode, pl["kind"], t16)
            assert t16["lds"] <= plan_ref.T16_LDS_LIMIT and t16["total"] == n * c["ny"] and t16["refine"] == c["sub"]
            assert (pl["kind"][1] == "tile16") == (c["levels"] == 2), pl["kind"]
        if c["id"] == "quads-129-half-pixel":
            assert t16["lds"] > 110 * 1024 and t16["attr"] == 1, t16["lds"]
        preds = rig.preds_of(refs) if c["levels"] == 2 else None
        reached |= ref.paths(c, preds, n_pairs=n)
        if preds is not None:
            rig.assert_predictor_census(c, preds, prevs, curs, ref)
        if c["frames"] == "corners":
            # the designed blocks are what they are built to be: the match at the reach with SAD 1, the direction won by the
            # one ring byte; and the LDS of the card holds nothing of these frames before the first form runs
            for by, bx, d in rig.corner_blocks(c):
                b, sd = refs[-1]["blocks"].reshape(c["ny"], c["nx"])[by, bx], refs[-1]["subdirs"].reshape(c["ny"], c["nx"])[by, bx]
                assert (int(b["dx"]), int(b["dy"]), int(b["sad"]), int(sd)) == (*rig.CORNER_DIRS[d], 1, d), (k, by, bx, b, sd)
            scrub(aof, torch, gpu_device, p, prevs.shape)
        counts = walk(aof, torch, gpu_device, c, k, p, prevs, curs, names, refs)
        want = planned(c, n, plan_ref.EXHAUSTIVE)[0]["counters"]
        assert counts == {name: want[name] for name in KERNELS}, (c["id"], counts, want)
        if c["frames"] == "ring":
            # the last pair's bottom corner block matched at the reach: its ring lies on the frame's last row
            b = refs[-1]["blocks"].reshape(c["ny"], c["nx"])[-1, -1 if k % 2 == 0 else 0]
            assert (int(b["dx"]), int(b["dy"])) == ((8, 8) if k % 2 == 0 else (-8, 8)) and b["sad"] < p.value_threshold, (k, b)
    if c.get("b2"):
        for i, name in enumerate(names):
            for hint in (1, 2, 3, 4):
                sizes, _ = rig.b2_list_sizes(prevs[i], curs[i], c["nx"], c["ny"], hint)
                assert not name.startswith("unrelated") or min(sizes) > ref.THREADS, (name, hint, sizes)
                assert not name.startswith("clean") or max(sizes) <= ref.THREADS, (name, hint, sizes)
    _walked[c["id"]] = reached
    print(f"{c['id']}: {time.perf_counter() - t0:.2f} s")


def test_staging_borders_are_named_by_the_model():
    by_id = {c["id"]: c for c in ref.CASES}
    for name, border in (("", ref.PLAIN_BORDER), ("-half-pixel", ref.REFINE_BORDER)):
        one, two = by_id["stage8-last-one-trip" + name], by_id["stage8-first-two-trips" + name]
        assert (one["w"], two["w"]) == border
        assert "stage8:one-trip" in ref.paths(one) and "stage8:second-trip" not in ref.paths(one)
        assert "stage8:second-trip" in ref.paths(two)
    # <false, false> and <true, false> under verdict 0 stage with one chunk per lane: a partial last trip either side of the border
    for w in ref.PLAIN_BORDER:
        nx, ny = ref.grid(w, 48, 0)
        for prune in (0, 1):
            g = ref.workgroup(w, 48, 0, nx, ny, 0, 0, 0, 0, 2, w * 48, prune, False, 0)
            assert g["stage"] == 1 and g["stage_partial"], (w, prune)


def test_the_walked_cases_reach_every_path_of_the_model():
    assert set(_walked) == {c["id"] for c in ref.CASES}, "every case of the list runs before this test (run the whole file)"
    assert set().union(*_walked.values()) == set(ref.VOCABULARY)
