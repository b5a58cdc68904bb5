"""The designed inputs of the wave-per-block search (tests/generic_edges_ref.py) on the oracle alone: every configuration's
census holds without a device, the plan model sends every configuration to the generic kernel, and between them the
configurations meet every situation the device test is there for."""
import pytest

import batch_plan_ref as plan_ref
import generic_edges_ref as ref

SWEEP, TWO, HANDOVER = ref.sweep_configs(), ref.two_level_configs(), ref.handover_configs()


def test_the_lists_are_the_ones_asked_for():
    assert len(SWEEP) == 32 and len({c["id"] for c in SWEEP}) == 32
    assert sorted((c["tile"], c["search"]) for c in SWEEP if not c["forced"] and c["sub"]) == [(8, s) for s in (1, 2, 3, 5, 6, 7, 8)] + [(16, s) for s in range(1, 8)]
    assert sorted((c["tile"], c["search"], c["sub"]) for c in SWEEP if c["forced"]) == [(8, 4, 0), (8, 4, 1), (16, 8, 0), (16, 8, 1)]
    assert all(c["w"] < 100 and c["h"] < 100 and ref.grid_of(c)[4:] == (3, 2) and ref.grid_of(c, c["w"] + 3)[4:] == (3, 2) for c in SWEEP)
    assert all((c["w"] + 3) % 4 != c["w"] % 4 and (c["w"] % 4 != 0 or (c["w"] + 3) % 4 != 0) for c in SWEEP)
    assert len(TWO) == 20 and all(c["w"] <= 100 and c["w"] % 2 == 0 and ref.grid_of(c, level=1)[4:] == (2, 2) for c in TWO)
    assert all(ref.grid_of(dict(c, w=c["w"] - 2, h=c["h"] - 2), level=1) is None or ref.grid_of(dict(c, w=c["w"] - 2, h=c["h"] - 2), level=1)[4] < 2 for c in TWO)
    reasons = [r for _, _, r in HANDOVER]
    assert {r: reasons.count(r) for r in set(reasons)} == {"grid": 6, "width": 6, "stride": 4, "prev": 6, "cur": 6, None: 16}
    assert all(c["w"] < 100 and c["h"] < 100 for c, _, _ in HANDOVER)


@pytest.mark.parametrize("c", SWEEP, ids=lambda c: c["id"])
def test_the_sweep_inputs_meet_their_census_on_the_oracle(aof, orc, synth, c):
    pl = plan_ref.plan(ref.plan_call(c, 12))
    assert pl["valid"] and pl["kind"][0] == "generic" and not pl["small"] and pl["coarse"] == "none"
    if c["tile"] == 8 or not c["sub"]:       # (16x16 +-8 with half-pixel: the smallest frame is 66 wide, which the 16x16 plan refuses anyway)
        assert c["forced"] == (plan_ref.plan(dict(ref.plan_call(c, 12), force_generic=False))["kind"][0] != "generic")
    for w in (c["w"], c["w"] + 3):
        met = set()
        for group in ref.groups_of(c):
            p, names, prevs, curs, metas, refs = ref.oracle_of(aof, orc, synth, c, group, w)
            met |= ref.census(c, group, w, p, names, prevs, curs, metas, refs, orc)
        assert met >= ref.wanted_sweep(c, w), (c["id"], w, ref.wanted_sweep(c, w) - met)


@pytest.mark.parametrize("c", TWO, ids=lambda c: c["id"])
def test_the_two_level_inputs_meet_their_census_on_the_oracle(aof, orc, synth, c):
    p, names, prevs, curs, metas, refs = ref.oracle_of(aof, orc, synth, c, "std")
    met = ref.census_two_levels(c, p, names, prevs, curs, metas, refs, orc)
    assert met >= ref.wanted_two_levels(c), (c["id"], ref.wanted_two_levels(c) - met)


@pytest.mark.parametrize("case", HANDOVER, ids=lambda x: x[0]["id"])
def test_the_handover_cases_are_refused_for_the_reason_they_name(aof, orc, synth, case):
    c, layout, reason = case
    ref.census_handover(c, layout, reason, 12)
    for group in ref.groups_of(c):
        p, names, prevs, curs, metas, refs = ref.oracle_of(aof, orc, synth, c, group)
        met = ref.census(c, group, c["w"], p, names, prevs, curs, metas, refs, orc)
        assert group != "std" or met >= {"corners", "ties"} | ({"ties-across-trips"} if c["search"] >= 4 else set()) | ({"every-direction"} if c["sub"] else set())
