"""The flat lane-per-block 8x8 launches -- k_search_lane8 with K3 behind it, k_flow_lane8_flat with the reduction in the
launch, the chunk walk k_search_lane8_pruned -- at every edge of their launch plan.  Each case of lane8_plan_ref.GPU_CASES is
a launch whose plan (threads, workgroups, finalisers, chunks per workgroup, the live lanes of the last workgroup) the model of
tests/lane8_plan_ref.py has worked out and whose paths the census of tests/test_lane8_plan_ref.py counts.  Here it runs: seven
designed pairs per geometry (deltas of 0, -40, +35 and one that saturates next to each other, unrelated noise, a flat pair,
exact ties; at two levels seven different predictors), the oracle once per distinct pair, the pairs replicated to the case's
pair count with content i % 7 -- seven is coprime to 2, 4, 8 and 64, so every content meets every lane position, chunk slot and
finaliser slot.  A case first asserts what ran (the variant, the launch counts of the search and of K3, the ADAPTIVE
counters), then EVERY pair's block records, flow record and half-pixel directions are compared with the oracle byte for byte.
The outputs are the caller's, cut from one arena between guard zones and filled with a sentinel before every launch; two
launches per engine.  No tolerance anywhere."""
import numpy as np
import pytest

import lane8_plan_ref as ref
from plan_rig import GUARD, SENTINEL, Arena, tiled, time_limit   # (time_limit: this module's fixture too, every test under a limit of its own)

pytestmark = pytest.mark.gpu

_oracle = {}


def oracle_for(aof, orc, synth, c, p):
    """The seven pairs of a case's geometry and the oracle's answers, computed once per geometry and shared (read-only)."""
    key = (c["w"], c["h"], c["levels"], c["subpixel"], c["mean_subtract"], c["num_blocks"])
    if key not in _oracle:
        prevs, curs = ref.pairs_for(c, synth)
        out = [orc.flow_pair(orc.params_from(p), prevs[i], curs[i]) for i in range(ref.DISTINCT)]
        ref.check_inputs(c, p, prevs, curs, out)        # before the device runs
        want = dict(blocks=np.stack([np.ascontiguousarray(o["blocks"]).view(np.uint32).ravel() for o in out]),
                    subdirs=np.stack([np.asarray(o["subdirs"], dtype=np.uint8).ravel() for o in out]),
                    flows=np.stack([np.frombuffer(o["flow"].tobytes(), dtype=np.uint8) for o in out]))
        for v in (prevs, curs, *want.values()):
            v.setflags(write=False)
        _oracle[key] = (prevs, curs, want)
    return _oracle[key]


def odd_layout(torch, device, src, n, stride):
    """src [k, h, w] replicated to n frames in an arena of their own: frame 0 one byte behind a 256-byte boundary, `stride`
    bytes from frame to frame, the last frame ending on the last byte in front of a guard zone."""
    h, w = src.shape[1:]
    data = 1 + (n - 1) * stride + h * w
    buf = torch.full((GUARD + data + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
    view = torch.as_strided(buf, (n, h, w), (stride, w, 1), GUARD + 1)
    view.copy_(tiled(torch, src, n, device))
    assert buf.data_ptr() % 256 == 0 and view.data_ptr() % 2 == 1 and view.stride(0) % 2 == 1
    assert view.data_ptr() + (n - 1) * stride + h * w == buf.data_ptr() + GUARD + data
    return buf, view


def every_pair_equals_the_oracle(c, arena, want, what):
    blocks, subdirs, flows = arena.outputs()      # (and every guard zone is intact)
    idx = np.arange(c["n_pairs"]) % ref.DISTINCT
    for name, got, exp in (("blocks", blocks, want["blocks"]), ("flows", flows, want["flows"]),
                           ("subdirs", subdirs, want["subdirs"] if c["subpixel"] else None)):
        if exp is None:   # no half-pixel step: nobody may have touched the directions
            assert (got == SENTINEL).all(), (c["id"], what, "directions written without the half-pixel step")
            continue
        bad = np.flatnonzero((got != exp[idx]).any(axis=1))
        if bad.size:
            i = int(bad[0])
            where = np.flatnonzero(got[i] != exp[idx[i]])
            pytest.fail(f"{c['id']} {what}: {name} of {bad.size} of {c['n_pairs']} pairs differ from the oracle's; pairs {bad[:6].tolist()} .. "
                        f"{bad[-3:].tolist()}; pair {i} (content {idx[i]}) at {where[:8].tolist()}: {got[i][where[:8]].tolist()} for "
                        f"{exp[idx[i]][where[:8]].tolist()}")


def modes_of(c, pl):
    """The case's mode, and for a chunk walk large enough for ADAPTIVE to prune the other two as well."""
    if pl["kind"] != "walk" or not pl["prune_large"]:
        return [c["mode"]]
    return [c["mode"]] + [m for m in ("pruned", "adaptive-1", "adaptive1") if m != c["mode"]]


@pytest.mark.parametrize("c", ref.GPU_CASES, ids=lambda c: c["id"])
def test_every_pair_of_the_launch_equals_the_oracle(aof, orc, synth, gpu_device, c):
    import torch
    p = aof.default_params(c["w"], c["h"], **ref.params_kw(c))
    assert aof.check_params(p) == 0 and tuple(aof.grid(p, 0)) == ref.case_grid(c)
    prevs, curs, want = oracle_for(aof, orc, synth, c, p)
    prevs, curs = prevs.copy(), curs.copy()      # (the shared ones are read-only; torch wants arrays it may write)
    n, nb = c["n_pairs"], c["nb"]
    pl = ref.case_plan(c)
    stride = ref.pair_stride(c)
    if c["layout"]:
        keep_prev, tp = odd_layout(torch, gpu_device, prevs, n, stride)
        keep_cur, tc = odd_layout(torch, gpu_device, curs, n, stride)
    else:
        tp, tc = tiled(torch, prevs, n, gpu_device), tiled(torch, curs, n, gpu_device)
        assert tp.is_contiguous() and tc.is_contiguous()
    assert tp.shape == (n, c["h"], c["w"]) and tp.stride(0) == tc.stride(0) == stride
    arena = Arena(torch, gpu_device, n, nb, aof.workspace_layout(p, n).total_bytes)
    out = arena.args(torch, c["subpixel"])
    for mode in modes_of(c, pl):
        eng = aof.FlowEngine(p, 0)
        assert eng.variant == "lane8"
        if mode in ("exhaustive", "pruned"):
            eng.set_search_mode(aof.SEARCH_EXHAUSTIVE if mode == "exhaustive" else aof.SEARCH_PRUNED)
        else:
            assert eng.search_mode == aof.SEARCH_ADAPTIVE
        eng.set_reduce_fusion(c["fused"])
        for launch in range(2):
            if mode.startswith("adaptive"):
                # told before every launch: what the first one reported about these frames (a flat pair and a noise pair among
                # them) does not overrule the caller
                eng.set_search_belief(1 if mode == "adaptive1" else -1)
            arena.refill()
            eng.set_profiling(True)
            eng.flow_batch(tp, tc, **out)
            torch.cuda.synchronize()
            searches, k3 = len(eng.profile_ms(aof.K_SEARCH)), len(eng.profile_ms(aof.K_REDUCE))
            eng.set_profiling(False)
            st = eng.search_stats()
            what = f"{mode} launch {launch} ({pl['kind']}, {pl['threads']} lanes, {pl['wgs']} + {pl['finalisers']} workgroups, spw {pl['spw']}) {st}"
            # what ran, before any byte is compared
            assert searches == 1, (c["id"], what)
            assert k3 == (0 if pl["kind"] == "fused" else 1), (c["id"], what, "K3 launches behind the search")
            if mode.startswith("adaptive"):
                assert st["pruned_launches"] == launch + 1 and st["exhaustive_launches"] == 0, (c["id"], what)
            else:
                assert st["pruned_launches"] == 0 and st["exhaustive_launches"] == 0, (c["id"], what)
            every_pair_equals_the_oracle(c, arena, want, what)
        eng.close()
    if c["layout"]:      # the guard zones around the frames: nobody writes frames, and the arena is what the case says
        for buf in (keep_prev, keep_cur):
            host = buf.cpu().numpy()
            assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all()
        del keep_prev, keep_cur
    del tp, tc, arena, out
    torch.cuda.empty_cache()
