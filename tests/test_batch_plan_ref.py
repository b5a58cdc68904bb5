"""Facts of the batch plan that its model (tests/batch_plan_ref.py, held to csrc/aof_batch_plan.hpp field by field by
tests/test_host_asan.py) shows without a device."""
import batch_plan_ref as ref


def test_no_valid_call_plans_the_separate_refinement_pass():
    """plan_level() sets `refine` for a 16x16 search with half-pixel refinement and no place for the directions.  batch_view()
    always gives one (the caller's, or l0_subdirs / l1_subdirs of the workspace), so the 16x16 kernel refines out of its tile
    in every call and K2b (k_refine.hip) is never launched: `refine` is false at both levels of every valid case."""
    cases = ref.batch_cases()
    planned = [(c, ref.plan(c)) for c in cases]
    valid = [(c, pl) for c, pl in planned if pl["valid"]]
    assert len(valid) >= 200 and any(pl["kind"][0] == "tile16" and c["subpixel"] for c, pl in valid) and any(pl["kind"][1] == "tile16" for c, pl in valid)
    assert [c["id"] for c, pl in valid if pl["refine"][0] or pl["refine"][1]] == []
    # the flag is not dead in the 16x16 plan itself: a search given no direction array would leave them to K2b
    behind = next(a for a in ref.tile16_cases() if a["id"] == "half-pixel-k2b-behind")
    assert behind["subpixel"] and not behind["subdirs"] and not ref.tile16_refines(behind) and ref.tile16_plan(behind)["refines"] == 0
