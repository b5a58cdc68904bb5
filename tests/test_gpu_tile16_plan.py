"""The 16x16 search at the edge of its LDS: the last width whose block row fits the kernel's tile and the next multiple of
16, for the exhaustive scan and for the pruned tables, each from the model (batch_plan_ref.tile16_edge_width), against the
oracle.

The last fitting width of the exhaustive scan is the largest dynamic-LDS opt-in the launcher ever makes; one step wider the
plan hands the configuration to the generic kernel.  One step beyond the pruned tables' last width the plan keeps the 16x16
kernel and clears the prune flag (search_kind): no probe and no fill run, the hints stay as the workspace held them."""
import numpy as np
import pytest

import batch_plan_ref as plan_ref
from tile16_rig import JUNK, PATTERN, assert_matches, oracle_refs, run

pytestmark = pytest.mark.gpu

H = 48                                   # two block rows
NAMES = ["clean", "noise8", "reach", "unrelated"]
_cache = {}


def designed(aof, orc, synth, W):
    """Four pairs of W x 48 frames and the oracle's records of them (computed once per width): a clean translation, one
    under +-8 LSB of noise, one at the corner of the +-8 reach, and a frame against unrelated noise."""
    if W not in _cache:
        p = aof.default_params(W, H, tile=16, search=8, value_threshold=12000, min_valid=0)
        assert aof.check_params(p) == 0 and W * H < 160 * 1024
        pairs = [synth.make_pair(W, H, 8, 5200, shift=(5, -3)), synth.make_pair(W, H, 8, 5201, shift=(-2, 6), noise=8),
                 synth.make_pair(W, H, 8, 5202, shift=(-8, 8))]
        rng = np.random.default_rng(52)
        pairs.append((pairs[0][0], rng.integers(0, 256, (H, W), dtype=np.uint8)))
        prevs, curs = np.stack([q[0] for q in pairs]), np.stack([q[1] for q in pairs])
        _cache[W] = (p, prevs, curs, oracle_refs(orc, p, prevs, curs))
    return _cache[W]


def planned(W, mode):
    pl = plan_ref.plan(plan_ref.call("edge", W, H, 4, tile=16, search=8, mode=mode))
    return pl, plan_ref.tile16_plan(pl["a0"])


@pytest.mark.parametrize("over", [0, 16], ids=["last-fitting", "first-over"])
def test_exhaustive_scan_at_the_last_width_that_fits_and_the_first_that_does_not(aof, orc, synth, gpu_device, over):
    import torch
    last = plan_ref.tile16_edge_width(prune=0)
    W = last + over
    pl, t16 = planned(W, plan_ref.EXHAUSTIVE)
    assert (t16["lds"] <= plan_ref.T16_LDS_LIMIT) == (not over)
    assert (pl["kind"][0], t16["verdict"]) == (("generic", "lds") if over else ("tile16", "ok"))
    assert over or (t16["attr"] == 1 and t16["total"] == 4 * 2)
    p, prevs, curs, refs = designed(aof, orc, synth, W)
    eng = aof.FlowEngine(p, 0)
    eng.set_search_mode(aof.SEARCH_EXHAUSTIVE)
    assert eng.variant == ("generic" if over else "tile16_lds")
    got = run(aof, eng, p, torch.from_numpy(prevs).to(gpu_device), torch.from_numpy(curs).to(gpu_device), gpu_device)
    assert_matches(got, refs, NAMES, W)
    assert np.array_equal(got["hints"], np.full(4, JUNK * 0x01010101, np.uint32)), "no probe, no fill"
    eng.close()


@pytest.mark.parametrize("over", [0, 16], ids=["last-fitting", "first-over"])
def test_adaptive_mode_at_the_last_width_whose_pruned_tables_fit_and_the_first_beyond(aof, orc, synth, gpu_device, over):
    import torch
    last = plan_ref.tile16_edge_width(prune=1)
    assert last + 16 <= plan_ref.tile16_edge_width(prune=0), "the exhaustive tile still fits one step beyond the tables"
    W = last + over
    pl, t16 = planned(W, plan_ref.ADAPTIVE)
    assert pl["kind"][0] == "tile16" and t16["verdict"] == "ok" and pl["prune"][0] == (0 if over else 2)
    p, prevs, curs, refs = designed(aof, orc, synth, W)
    eng = aof.FlowEngine(p, 0)
    assert eng.search_mode == aof.SEARCH_ADAPTIVE and eng.variant == "tile16_lds"
    got = run(aof, eng, p, torch.from_numpy(prevs).to(gpu_device), torch.from_numpy(curs).to(gpu_device), gpu_device, (0,))
    assert_matches(got, refs, NAMES, W)
    # the pruned form: the fill kernel set every pair's verdict; one step wider the search is the exhaustive scan and
    # nothing writes the hints
    want = np.full(4, PATTERN if not over else JUNK * 0x01010101, np.uint32)
    assert np.array_equal(got["hints"], want), (W, got["hints"])
    assert plan_ref.tile16_plan(pl["a0"], forced=1)["front"] == ("none" if over else "fill")
    eng.close()
