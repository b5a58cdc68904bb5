"""The column walk (k_search_lane8_cols / k_flow_lane8_cols) at every edge of its segment plan: each case of
cols_plan_ref.GPU_CASES is a launch whose plan -- head and tail segment lengths, the border between the two classes, the
padding of a pair's units, the `aligned` flag -- the model of tests/cols_plan_ref.py has worked out, and whose paths the
census of tests/test_cols_plan_ref.py counts.  Here the launch runs: six to eight distinct small pairs, the oracle once
per distinct pair, the pairs replicated to the case's pair count, and EVERY pair's block records, flow record and
half-pixel directions compared with the oracle byte for byte.  The outputs are the caller's, cut from one arena between
guard zones and filled with a sentinel before every launch: a slot nobody wrote, or a write behind the end, fails.  Two
launches per engine (the vote memory must be zero again after the first)."""
import numpy as np
import pytest

import cols_plan_ref as ref
from plan_rig import SENTINEL, Arena, tiled, time_limit   # (time_limit: this module's fixture too, every test under a limit of its own)

pytestmark = pytest.mark.gpu

_oracle = {}


def oracle_for(aof, orc, synth, c):
    """The distinct pairs of a case and the oracle's answers, computed once per frame geometry and shared (read-only)."""
    key = (c["w"], c["h"], c["subpixel"], c["levels"], ref.distinct_pairs(c))
    if key not in _oracle:
        p = aof.default_params(c["w"], c["h"], **ref.params_kw(c))
        prevs, curs = ref.pairs_for(c, synth)
        out = [orc.flow_pair(orc.params_from(p), prevs[i], curs[i]) for i in range(prevs.shape[0])]
        want = dict(blocks=np.stack([np.ascontiguousarray(o["blocks"]).view(np.uint32).ravel() for o in out]),
                    subdirs=np.stack([np.asarray(o["subdirs"], dtype=np.uint8).ravel() for o in out]),
                    flows=np.stack([np.frombuffer(o["flow"].tobytes(), dtype=np.uint8) for o in out]),
                    px=tuple(int(o["flow"]["pred_x"]) for o in out))
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _oracle[key] = (prevs, curs, want)
    return _oracle[key]


def every_pair_equals_the_oracle(c, arena, want, what):
    blocks, subdirs, flows = arena.outputs()
    k = want["blocks"].shape[0]
    idx = np.arange(c["n_pairs"]) % k
    head_pairs = ref.case_plan(c)["head_pairs"]
    for name, got, exp in (("blocks", blocks, want["blocks"]), ("flows", flows, want["flows"]),
                           ("subdirs", subdirs, want["subdirs"] if c["subpixel"] else None)):
        if exp is None:   # no half-pixel step: nobody may have touched the directions
            assert (got == SENTINEL).all(), (c["id"], what, "directions written without the half-pixel step")
            continue
        bad = np.flatnonzero((got != exp[idx]).any(axis=1))
        if bad.size:
            i = int(bad[0])
            where = np.flatnonzero(got[i] != exp[idx[i]])
            pytest.fail(f"{c['id']} {what}: {name} of {bad.size} pairs differ from the oracle's; pairs {bad[:6].tolist()} .. {bad[-3:].tolist()} "
                        f"(head pairs: {head_pairs}); pair {i} (content {idx[i]}) at {where[:8].tolist()}: "
                        f"{got[i][where[:8]].tolist()} for {exp[idx[i]][where[:8]].tolist()}")


def k3_launches(aof, torch, eng, call):
    eng.set_profiling(True)
    call()
    torch.cuda.synchronize()
    n = len(eng.profile_ms(aof.K_REDUCE))
    eng.set_profiling(False)
    return n


@pytest.mark.parametrize("c", ref.GPU_CASES, ids=lambda c: c["id"])
def test_every_pair_of_the_launch_equals_the_oracle(aof, orc, synth, gpu_device, c):
    import torch
    p = aof.default_params(c["w"], c["h"], **ref.params_kw(c))
    g = aof.grid(p, 0)
    assert (g[4], g[5]) == (c["nx"], c["ny"]) and (g[2], g[3]) == (8, 8) and g[0] == 4 + c["subpixel"]
    prevs, curs, want = oracle_for(aof, orc, synth, c)
    n, nb, k = c["n_pairs"], c["nx"] * c["ny"], prevs.shape[0]
    pl = ref.case_plan(c)
    assert pl["head_pairs"] % k != 0, "both classes see every content"
    if c["levels"] == 2:
        assert want["px"] == c["px"][:k], "the predictors the model derived the misalignments from"
    tp, tc = tiled(torch, prevs, n, gpu_device), tiled(torch, curs, n, gpu_device)
    assert tp.shape == (n, c["h"], c["w"]) and tp.is_contiguous() and tp.data_ptr() % 4 == 0 and tc.data_ptr() % 4 == 0
    assert int(c["w"] % 4 == 0 and (c["w"] * c["h"]) % 4 == 0) == pl["aligned"]
    arena = Arena(torch, gpu_device, n, nb, aof.workspace_layout(p, n).total_bytes)
    eng = aof.FlowEngine(p, 0)
    assert eng.variant == "lane8"
    out = arena.args(torch, c["subpixel"])
    run = lambda: eng.flow_batch(tp, tc, **out)
    if c["mode"] == "pruned":
        eng.set_search_mode(aof.SEARCH_PRUNED)
    else:
        assert eng.search_mode == aof.SEARCH_ADAPTIVE
        eng.set_search_belief(1 if c["mode"] == "adaptive1" else 0)
    eng.set_reduce_fusion(c["fused"])
    if c["mode"] == "adaptive0":
        # a context told that pruning does not pay looks again with its 16th launch: the pruned kernel, the first block of
        # every wave judging
        arena.refill()
        for _ in range(15):
            run()
        torch.cuda.synchronize()
        assert eng.search_stats()["pruned_launches"] == 0, eng.search_stats()
    for launch in range(2):
        arena.refill()
        if launch == 1 and c["mode"] == "adaptive1":
            # told again: what the first launch reported about these frames (a flat pair and a noise pair among them) does
            # not overrule the caller, so the second launch is the column walk as well, on the vote memory the first left
            eng.set_search_belief(1)
        k3 = k3_launches(aof, torch, eng, run)
        st = eng.search_stats()
        if c["mode"] != "adaptive0" or launch == 0:
            assert k3 == (0 if ref.votes(c) else 1), (c["id"], launch, "K3 launches behind the search", st)
        if c["mode"] == "adaptive1":
            assert st["pruned_launches"] == launch + 1, st
        if c["mode"] == "adaptive0" and launch == 0:
            assert st["pruned_launches"] == 1, st
        every_pair_equals_the_oracle(c, arena, want, f"launch {launch} {st}")
    if c["graph"]:
        # the same launch captured on one stream and replayed twice into sentinel-filled outputs
        assert ref.votes(c) and pl["tail_pairs"] > 0
        side = torch.cuda.Stream(gpu_device)
        side.wait_stream(torch.cuda.current_stream(gpu_device))
        with torch.cuda.stream(side):   # (warm-up on a side stream, as torch asks for)
            run()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run()
        for replay in range(2):
            arena.refill()
            graph.replay()
            torch.cuda.synchronize()
            every_pair_equals_the_oracle(c, arena, want, f"replay {replay}")
        del graph
    eng.close()
    del tp, tc, arena, out
    torch.cuda.empty_cache()
