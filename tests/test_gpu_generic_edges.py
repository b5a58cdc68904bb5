"""The wave-per-block search (csrc/k_search_generic.hip) against the CPU oracle at every edge of its launch, byte for byte:
block records, half-pixel directions and flow records, at two levels the workspace's level-1 records, directions and flow
records as well.  No tolerance anywhere.  The inputs and what each is there for: tests/generic_edges_ref.py; every case
first asserts its census on the oracle's records (the same census tests/test_generic_edges_ref.py runs without a device),
then that the context (or, where only the frame layout refuses the 16x16 kernel, the launch) takes the generic kernel, and
only then compares the device.  Outputs and workspace lie between sentinel-filled guard zones of one arena
(tests/plan_rig.py), the frames between guard zones of their own; all of them are checked after every launch.

  radius sweep   tile 8 with S in 1, 2, 3, 5, 6, 7, 8 and tile 16 with S in 1 .. 7, without and with half-pixel refinement
                 (28 configurations that are generic by themselves), and 8x8 +-4 and 16x16 +-8 under force_generic; the
                 smallest frame of 3 x 2 blocks and one 3 pixels wider; 1, 2 and 37 pairs beside the whole batch.
  two levels     tile 8 with S in 1, 3, 8 and tile 16 with S in 2, 7, mean_subtract and subpixel 0 and 1: predictors of both
                 signs, and under them level-0 winners on every corner of the scan, out to 3S.
  handover       every refusal of the 16x16 plan that a small frame reaches (grid, width, stride, prev, cur; "lds" is held by
                 tests/test_gpu_tile16_plan.py), and the same strides and pointer offsets on 8x8 +-3.
                 FlowEngine.variant is the plan at aligned addresses of a whole-frame stride: it says "generic" for the grid
                 and width refusals.  For the stride and pointer refusals it cannot; there the launch is known to be the
                 generic kernel's because nothing wrote the workspace's hints (the 16x16 kernel of an adaptive context is
                 preceded by its probe, which writes one word per pair -- the aligned twin of the case shows it).

The lane-per-block kernels' own refusal (more than 4 GB between a wave's first and last pair) is out of reach of a test of a
few seconds; the 32 768-pair split of the launch over grid y / z is held by the large-batch test of tests/test_gpu_parity.py."""
import numpy as np
import pytest

import generic_edges_ref as ref
from plan_rig import SENTINEL, Arena
from plan_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

GUARD, FRAME_SENTINEL = 4096, 0x5C


class Frames:
    """prev and cur of a launch, each in a buffer of its own between two guard zones: pair i of n holds content i % k and
    starts `off` + i * stride bytes behind a 256-byte boundary."""

    def __init__(self, torch, device, prevs, curs, n, stride, prev_off=0, cur_off=0):
        k, h, w = prevs.shape
        at = torch.arange(n, device=device) % k
        self.bufs, views = [], []
        for src, off in ((prevs, prev_off), (curs, cur_off)):
            buf = torch.full((GUARD + off + n * stride + GUARD,), FRAME_SENTINEL, dtype=torch.uint8, device=device)
            view = torch.as_strided(buf, (n, h, w), (stride, w, 1), GUARD + off)
            view.copy_(torch.from_numpy(src.copy()).to(device)[at])
            assert buf.data_ptr() % 256 == 0 and view.data_ptr() - buf.data_ptr() == GUARD + off and view.stride(0) == stride
            self.bufs.append(buf), views.append(view)
        self.prev, self.cur = views
        self.held = [b.cpu().numpy().copy() for b in self.bufs]
        assert all((x[:GUARD] == FRAME_SENTINEL).all() and (x[-GUARD:] == FRAME_SENTINEL).all() for x in self.held)

    def assert_untouched(self, what):
        for name, buf, held in zip(("prev", "cur"), self.bufs, self.held):
            bad = np.flatnonzero(buf.cpu().numpy() != held)
            assert bad.size == 0, (what, name, "frames or their guards written", bad[:8])


def launch(aof, device, c, p, prevs, curs, n=None, stride_extra=0, prev_off=0, cur_off=0, variant="generic"):
    """One batch of n pairs (default: every distinct pair once) on sentinel-filled outputs and workspace."""
    import torch
    n = prevs.shape[0] if n is None else n
    eng = aof.FlowEngine(p, 0)
    if c["forced"]:
        eng.force_generic(True)
    assert eng.variant == variant, (c["id"], eng.variant)
    stride = p.width * p.height + stride_extra
    fr = Frames(torch, device, prevs, curs, n, stride, prev_off, cur_off)
    nb, L = eng.nblocks(0), aof.workspace_layout(p, n)
    arena = Arena(torch, device, n, nb, L.total_bytes)
    arena.refill()
    eng.flow_batch(fr.prev, fr.cur, pair_stride=stride, **arena.args(torch, p.subpixel))
    torch.cuda.synchronize()
    blocks, subdirs, flows = arena.outputs()          # (asserts the guard zones)
    fr.assert_untouched(c["id"])
    ws = arena.views["ws"].cpu().numpy()
    got = dict(blocks=blocks, subdirs=subdirs if p.subpixel else None, flows=flows,
               hints=ws[L.hints:L.hints + 4 * n].view(np.uint32).copy() if p.tile == 16 else None)       # (a 16x16 workspace ends in them)
    if p.pyramid_levels == 2:
        nb1 = eng.nblocks(1)
        got.update(l1=ws[L.l1_blocks:L.l1_blocks + 4 * n * nb1].view(np.uint32).reshape(n, nb1), f1=ws[L.l1_flows:L.l1_flows + 16 * n].reshape(n, 16),
                   s1=ws[L.l1_subdirs:L.l1_subdirs + n * nb1].reshape(n, nb1) if p.subpixel else None)
    eng.close()
    return got


def assert_oracle(got, refs, names, what):
    """Pair i of the launch against the oracle's records of content i % k."""
    k = len(refs)
    for i in range(got["blocks"].shape[0]):
        r, key = refs[i % k], (what, i, names[i % k])
        assert got["blocks"][i].tobytes() == r["blocks"].tobytes(), (key, got["blocks"][i], r["blocks"].view(np.uint32))
        assert got["flows"][i].tobytes() == r["flow"].tobytes(), (key, got["flows"][i], r["flow"])
        if got["subdirs"] is not None:
            assert got["subdirs"][i].tobytes() == r["subdirs"].tobytes(), (key, got["subdirs"][i], r["subdirs"])
        if "l1" in got:
            assert got["l1"][i].tobytes() == r["blocks_l1"].tobytes(), (key, "level-1 records")
            assert got["f1"][i].tobytes() == r["flow_l1"].tobytes(), (key, "level-1 flow record", got["f1"][i], r["flow_l1"])
            if got["s1"] is not None:
                assert got["s1"][i].tobytes() == r["subdirs_l1"].tobytes(), (key, "level-1 directions")


@pytest.mark.parametrize("c", ref.sweep_configs(), ids=lambda c: c["id"])
def test_every_radius_of_both_tiles_equals_the_oracle(aof, orc, synth, gpu_device, c):
    """Candidate trips, byte phases, key width and refinement: every group of designed pairs in one launch each, at the
    smallest frame and one 3 pixels wider; the published-gates batch also as 1, 2 and 37 pairs."""
    for w in (c["w"], c["w"] + 3):
        designs = {group: ref.oracle_of(aof, orc, synth, c, group, w) for group in ref.groups_of(c)}
        met = set()
        for group, (p, names, prevs, curs, metas, refs) in designs.items():
            met |= ref.census(c, group, w, p, names, prevs, curs, metas, refs, orc)
        assert met >= ref.wanted_sweep(c, w), (c["id"], w, ref.wanted_sweep(c, w) - met)
        for group, (p, names, prevs, curs, metas, refs) in designs.items():
            assert_oracle(launch(aof, gpu_device, c, p, prevs, curs), refs, names, (c["id"], group, w))
            if group == "std" and w == c["w"]:
                for n in (1, 2, 37):
                    assert_oracle(launch(aof, gpu_device, c, p, prevs, curs, n), refs, names, (c["id"], group, w, n))


@pytest.mark.parametrize("c", ref.two_level_configs(), ids=lambda c: c["id"])
def test_both_levels_under_a_predictor_equal_the_oracle(aof, orc, synth, gpu_device, c):
    """The window test under predictors of both signs, blocks pushed out of the frame, the equalising delta of both signs
    with its clamps; level 1's records, directions and flow record (with the predictor) from the workspace."""
    p, names, prevs, curs, metas, refs = ref.oracle_of(aof, orc, synth, c, "std")
    met = ref.census_two_levels(c, p, names, prevs, curs, metas, refs, orc)
    assert met >= ref.wanted_two_levels(c), (c["id"], ref.wanted_two_levels(c) - met)
    assert_oracle(launch(aof, gpu_device, c, p, prevs, curs), refs, names, c["id"])
    assert_oracle(launch(aof, gpu_device, c, p, prevs, curs, 37), refs, names, (c["id"], 37))


@pytest.mark.parametrize("case", ref.handover_configs(), ids=lambda x: x[0]["id"])
def test_every_refusal_of_the_16x16_plan_ends_in_the_generic_kernel(aof, orc, synth, gpu_device, case):
    c, layout, reason = case
    params_decide = reason in ("grid", "width", None)
    for group in ref.groups_of(c):
        p, names, prevs, curs, metas, refs = ref.oracle_of(aof, orc, synth, c, group)
        ref.census(c, group, c["w"], p, names, prevs, curs, metas, refs, orc)
        ref.census_handover(c, layout, reason, len(names))
        got = launch(aof, gpu_device, c, p, prevs, curs, variant="generic" if params_decide else "tile16_lds", **layout)
        assert c["tile"] == 8 or (got["hints"] == SENTINEL * 0x01010101).all(), (c["id"], "a 16x16 launch's probe wrote the hints", got["hints"])
        assert_oracle(got, refs, names, (c["id"], group))


@pytest.mark.parametrize("sub", [0, 1])
def test_the_aligned_twin_of_the_layout_refusals_runs_the_16x16_kernel(aof, orc, synth, gpu_device, sub):
    """What tells the two kernels apart in the test above: on the same frames at aligned addresses the adaptive context's
    probe writes every pair's hint."""
    c = next(c for c, layout, reason in ref.handover_configs() if reason == "stride" and c["sub"] == sub)
    p, names, prevs, curs, metas, refs = ref.oracle_of(aof, orc, synth, c, "std")
    assert ref.plan_ref.plan(ref.plan_call(c, len(names)))["kind"][0] == "tile16"
    got = launch(aof, gpu_device, c, p, prevs, curs, variant="tile16_lds")
    assert (got["hints"] != SENTINEL * 0x01010101).all(), got["hints"]
    assert_oracle(got, refs, names, (c["id"], "aligned"))
