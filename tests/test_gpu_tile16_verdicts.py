"""Every verdict of the 16x16 adaptive search, forced on hard inputs, and the probe that chooses them held to a host model.

k_tile16_probe writes a verdict per pair into the workspace's hints (0 the exhaustive scan; 1, 2, 3, 4 step A on two-,
one-, four- or eight-row lower bounds) and k_search_tile16<true, ..> follows it.  The verdict is about speed only: every
branch must write the oracle's records bit for bit.  aof_debug_tile16_verdicts sets the verdicts (a fill kernel instead of
the probe), so each branch meets every kind of input here -- not only the pairs the probe would send it -- and
tile16_probe_ref.py restates the probe, whose words must come out of the kernel exactly."""
import errno

import numpy as np
import pytest

import tile16_probe_ref as probe_ref
from tile16_rig import JUNK, PATTERN, assert_matches, hard_batch, oracle_refs, run

pytestmark = pytest.mark.gpu

ROTATION = [0, 1, 2, 3, 4]
SETTINGS = [[0], [1], [2], [3], [4], ROTATION]
OPTION_SETS = {
    "one_level": dict(),
    "half_pixel": dict(subpixel=1),
    "two_level_equalised": dict(pyramid_levels=2, mean_subtract=1),
    "two_level_half_pixel": dict(pyramid_levels=2, subpixel=1),
}


def forced_words(verdicts, n):
    return np.array([verdicts[i % len(verdicts)] | PATTERN for i in range(n)], np.uint32)


def check_every_setting(aof, orc, p, prevs, curs, names, device, l1=False, settings=SETTINGS):
    """Every setting on one batch: records against the oracle (computed once) and the exhaustive scan, hints as forced."""
    import torch
    refs = oracle_refs(orc, p, prevs, curs)
    eng = aof.FlowEngine(p, 0)
    assert eng.variant == "tile16_lds" and eng.search_mode == aof.SEARCH_ADAPTIVE
    if l1:
        eng.set_split_coarse(True)
    tp, tc = torch.from_numpy(prevs).to(device), torch.from_numpy(curs).to(device)
    eng.set_search_mode(aof.SEARCH_EXHAUSTIVE)
    ex = run(aof, eng, p, tp, tc, device)
    assert_matches(ex, refs, names, "exhaustive", l1)
    eng.set_search_mode(aof.SEARCH_ADAPTIVE)
    for v in settings:
        got = run(aof, eng, p, tp, tc, device, v)
        assert_matches(got, refs, names, v, l1, ex)
        assert np.array_equal(got["hints"], forced_words(v, len(names))), (v, [hex(x) for x in got["hints"]])
    eng.close()
    return refs


@pytest.mark.parametrize("opts", list(OPTION_SETS))
def test_every_verdict_on_hard_inputs(aof, orc, synth, gpu_device, opts):
    kw = OPTION_SETS[opts]
    two = kw.get("pyramid_levels") == 2
    W, H = 320, 256
    p = aof.default_params(W, H, tile=16, search=8, value_threshold=12000, **kw)
    prevs, curs, names = hard_batch(synth, W, H, two)
    refs = check_every_setting(aof, orc, p, prevs, curs, names, gpu_device, l1=two)
    if two:
        # the inputs reach what they are there for: a predictor without a row shift and with a column shift that is no
        # multiple of 16 (the last block row's displaced copy ends on the frame's last byte: the tail guard, origin 0), and
        # one that pushes the edge blocks' windows out of the frame
        hz, far = refs[names.index("horizontal")]["flow"], refs[names.index("reach")]["flow"]
        assert int(hz["pred_y"]) == 0 and int(hz["pred_x"]) % 16 != 0, hz
        assert int(far["pred_x"]) < 0 and int(far["pred_y"]) > 8, far
        assert (refs[names.index("reach")]["blocks"]["sad"] == 0xFFFF).any()


def test_every_pruned_verdict_on_c5_frames(aof, orc, synth, gpu_device):
    """1280 x 960: on the noisy and the unrelated pair step B2's list outgrows one round of the workgroup's 512 lanes, so
    the switch that drops its four-row bound after the first round is evaluated; on the clean pair it is not."""
    W, H = 1280, 960
    p = aof.default_params(W, H, tile=16, search=8, value_threshold=12000)
    clean_p, clean_c, _ = synth.make_pair(W, H, 8, 4200)
    noisy_p, noisy_c, _ = synth.make_pair(W, H, 8, 4201, noise=40)
    unrelated = np.random.default_rng(42).integers(0, 256, (H, W), dtype=np.uint8)
    prevs, curs = np.stack([clean_p, noisy_p, clean_p]), np.stack([clean_c, noisy_c, unrelated])
    check_every_setting(aof, orc, p, prevs, curs, ["clean", "noise40", "unrelated"], gpu_device,
                        settings=[[1], [2], [3], [4]])


@pytest.mark.parametrize("size", [(32, 5008), (48, 2000), (64, 64), (16 * 30, 48)])
def test_rotation_on_narrow_tall_and_tiny_grids(aof, orc, synth, gpu_device, size):
    W, H = size
    p = aof.default_params(W, H, tile=16, search=8, value_threshold=12000, min_valid=0)
    assert aof.check_params(p) == 0
    prevs, curs, _ = synth.make_batch(W, H, 3, 8, 4300 + W, noise=0)
    rng = np.random.default_rng(43)
    curs[1] = np.clip(curs[1].astype(np.int16) + rng.integers(-40, 41, curs[1].shape), 0, 255).astype(np.uint8)
    curs[2] = np.clip(curs[2].astype(np.int16) + rng.integers(-12, 13, curs[2].shape), 0, 255).astype(np.uint8)
    check_every_setting(aof, orc, p, prevs, curs, ["clean", "noise40", "noise12"], gpu_device, settings=[ROTATION])


def test_rotation_captured_into_a_graph(aof, orc, synth, gpu_device):
    """The fill kernel is a launch like the probe: captured with the rest of the batch, a replay writes the verdicts
    and records again, the eager bytes."""
    import torch
    W, H = 320, 256
    p = aof.default_params(W, H, tile=16, search=8, value_threshold=12000, pyramid_levels=2, mean_subtract=1)
    prevs, curs, names = hard_batch(synth, W, H, True)
    n = len(names)
    eng = aof.FlowEngine(p, 0)
    eng.set_split_coarse(True)
    tp, tc = torch.from_numpy(prevs).to(gpu_device), torch.from_numpy(curs).to(gpu_device)
    eager = run(aof, eng, p, tp, tc, gpu_device, ROTATION)
    assert np.array_equal(eager["hints"], forced_words(ROTATION, n))
    L = aof.workspace_layout(p, n)
    ws = torch.full((L.total_bytes,), JUNK, dtype=torch.uint8, device=gpu_device)
    blocks = torch.zeros((n, eng.nblocks(0)), dtype=torch.int32, device=gpu_device)
    flows = torch.zeros((n, 16), dtype=torch.uint8, device=gpu_device)
    side = torch.cuda.Stream(gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):   # (warm-up on the capture stream, as torch asks for)
        eng.flow_batch(tp, tc, blocks=blocks, flows=flows, workspace=ws)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.flow_batch(tp, tc, blocks=blocks, flows=flows, workspace=ws)
    nb1 = eng.nblocks(1)
    for rep in range(2):
        ws.fill_(JUNK); blocks.zero_(); flows.zero_()
        g.replay()
        torch.cuda.synchronize()
        w = ws.cpu().numpy()
        assert aof.blocks_view(blocks).tobytes() == eager["blocks"].tobytes(), rep
        assert aof.flows_view(flows).tobytes() == eager["flows"].tobytes(), rep
        assert w[L.l1_blocks:L.l1_blocks + 4 * n * nb1].tobytes() == eager["l1"].tobytes(), rep
        assert np.array_equal(w[L.hints:L.hints + 4 * n].view(np.uint32), eager["hints"]), rep
    del g
    eng.close()


# ---- the hook itself ----

def test_hook_rejects_what_its_header_rejects(aof, gpu_device):
    import ctypes
    lib, EINVAL = aof.lib, -errno.EINVAL
    one = (ctypes.c_uint8 * 9)(*([1] * 9))
    assert lib.aof_debug_tile16_verdicts(None, one, 1) == EINVAL
    eng8 = aof.FlowEngine(aof.default_params(320, 256), 0)            # 8x8 tiles
    assert lib.aof_debug_tile16_verdicts(eng8._ctx, one, 1) == EINVAL
    with pytest.raises(aof.AofError):
        eng8.debug_tile16_verdicts([1])
    eng8.close()
    eng = aof.FlowEngine(aof.default_params(320, 256, tile=16, search=8), 0)
    ctx = eng._ctx
    assert lib.aof_debug_tile16_verdicts(ctx, one, -1) == EINVAL
    assert lib.aof_debug_tile16_verdicts(ctx, one, 9) == EINVAL
    assert lib.aof_debug_tile16_verdicts(ctx, None, 2) == EINVAL
    for bad in ([5], [0, 1, 2, 3, 4, 255]):
        assert lib.aof_debug_tile16_verdicts(ctx, (ctypes.c_uint8 * len(bad))(*bad), len(bad)) == EINVAL, bad
    assert lib.aof_debug_tile16_verdicts(ctx, one, 8) == 0
    assert lib.aof_debug_tile16_verdicts(ctx, None, 0) == 0
    eng.close()


def test_count_zero_gives_the_decision_back_to_the_probe(aof, synth, gpu_device):
    import torch
    W, H = 320, 256
    p = aof.default_params(W, H, tile=16, search=8, value_threshold=12000)
    prevs, curs, _ = synth.make_batch(W, H, 2, 8, 4400)
    tp, tc = torch.from_numpy(prevs).to(gpu_device), torch.from_numpy(curs).to(gpu_device)
    want = [probe_ref.level0_word(p, prevs[i], curs[i]) for i in range(2)]
    assert [w & 0xFF for w in want] == [2, 2]                          # clean translations
    eng = aof.FlowEngine(p, 0)
    forced = run(aof, eng, p, tp, tc, gpu_device, [0])
    assert forced["hints"].tolist() == [PATTERN, PATTERN]
    back = run(aof, eng, p, tp, tc, gpu_device, [])
    assert back["hints"].tolist() == want
    assert back["blocks"].tobytes() == forced["blocks"].tobytes()
    eng.close()


def test_fixed_modes_and_tables_too_wide_for_lds_leave_the_hints_alone(aof, orc, synth, gpu_device):
    """EXHAUSTIVE and PRUNED run no probe and no fill; neither does an ADAPTIVE context whose pruned tables do not fit LDS
    (3 200 px: the search drops to the exhaustive scan).  The hints region keeps what the workspace held."""
    import torch
    junk = np.full(2, JUNK * 0x01010101, np.uint32)
    W, H = 320, 256
    p = aof.default_params(W, H, tile=16, search=8, value_threshold=12000)
    prevs, curs, names = synth.make_batch(W, H, 2, 8, 4500, noise=8)
    refs = oracle_refs(orc, p, prevs, curs)
    eng = aof.FlowEngine(p, 0)
    eng.debug_tile16_verdicts([3, 4])
    tp, tc = torch.from_numpy(prevs).to(gpu_device), torch.from_numpy(curs).to(gpu_device)
    for mode in (aof.SEARCH_EXHAUSTIVE, aof.SEARCH_PRUNED):
        eng.set_search_mode(mode)
        got = run(aof, eng, p, tp, tc, gpu_device)
        assert_matches(got, refs, ["a", "b"], mode)
        assert np.array_equal(got["hints"], junk), (mode, got["hints"])
    eng.close()
    W, H = 3200, 48
    p = aof.default_params(W, H, tile=16, search=8, value_threshold=12000, min_valid=0)
    assert aof.check_params(p) == 0
    prevs, curs, _ = synth.make_batch(W, H, 2, 8, 4510, noise=8)
    refs = oracle_refs(orc, p, prevs, curs)
    eng = aof.FlowEngine(p, 0)
    assert eng.variant == "tile16_lds" and eng.search_mode == aof.SEARCH_ADAPTIVE
    eng.debug_tile16_verdicts([3, 4])
    got = run(aof, eng, p, torch.from_numpy(prevs).to(gpu_device), torch.from_numpy(curs).to(gpu_device), gpu_device)
    assert_matches(got, refs, ["a", "b"], "wide")
    assert np.array_equal(got["hints"], junk), got["hints"]
    eng.close()


# ---- the probe against its host model ----

def probe_batches(synth, orc, aof):
    """(name, params, prevs, curs, predictors): the shapes and option sets the probe runs on."""
    out = []
    W, H = 1280, 960
    sweep = [synth.make_pair(W, H, 8, 4600 + k, noise=k) for k in (0, 4, 8, 16, 40)]
    rng = np.random.default_rng(46)
    prevs = np.stack([s[0] for s in sweep] + [sweep[0][0], np.full((H, W), 90, np.uint8)])
    curs = np.stack([s[1] for s in sweep] + [rng.integers(0, 256, (H, W), dtype=np.uint8), np.full((H, W), 90, np.uint8)])
    out.append(("c5", aof.default_params(W, H, tile=16, search=8, value_threshold=12000), prevs, curs))
    W, H = 320, 256
    for name, kw in (("one_level", dict()), ("equalised", dict(mean_subtract=1)), ("half_pixel", dict(subpixel=1)),
                     ("two_level", dict(pyramid_levels=2, mean_subtract=1)),
                     ("two_level_half_pixel", dict(pyramid_levels=2, subpixel=1))):
        prevs, curs, _ = hard_batch(synth, W, H, kw.get("pyramid_levels") == 2)
        out.append((name, aof.default_params(W, H, tile=16, search=8, value_threshold=12000, **kw), prevs, curs))
    for W, H in ((32, 5008), (48, 2000), (64, 64), (16 * 30, 48)):
        prevs, curs, _ = synth.make_batch(W, H, 3, 8, 4700 + W, noise=0)
        curs[1] = np.clip(curs[1].astype(np.int16) + rng.integers(-40, 41, curs[1].shape), 0, 255).astype(np.uint8)
        curs[2] = np.clip(curs[2].astype(np.int16) + rng.integers(-8, 9, curs[2].shape), 0, 255).astype(np.uint8)
        out.append((f"{W}x{H}", aof.default_params(W, H, tile=16, search=8, value_threshold=12000, min_valid=0), prevs, curs))
    return out


def test_probe_words_equal_the_host_model(aof, orc, synth, gpu_device):
    """Every hint word -- verdict and separation figure -- of three identical launches equals the model's.  The deeper
    look's two passes share the two-row bound table, so without the barrier between them a verdict could depend on wave
    timing; three launches of the same batch must agree with the model every time."""
    import torch
    seen = set()
    for name, p, prevs, curs in probe_batches(synth, orc, aof):
        n = prevs.shape[0]
        if p.pyramid_levels == 2:
            po = orc.params_from(p)
            preds = [(int(f["pred_x"]), int(f["pred_y"])) for f in (orc.flow_pair(po, prevs[i], curs[i])["flow"] for i in range(n))]
        else:
            preds = [(0, 0)] * n
        want = np.array([probe_ref.level0_word(p, prevs[i], curs[i], preds[i]) for i in range(n)], np.uint32)
        seen |= set((want & 0xFF).tolist())
        if name == "c5":
            # the round-5 sweep (profiles/r05_tile16_one_row_bounds.txt): 0, 4, 8, 16, 40 LSB -> 2, 1, 3, 4, 0
            assert (want[:5] & 0xFF).tolist() == [2, 1, 3, 4, 0], [(w & 0xFF, w >> 8) for w in want]
        eng = aof.FlowEngine(p, 0)
        if p.pyramid_levels == 2:
            eng.set_split_coarse(True)   # (level 1 runs a probe of its own first; level 0's overwrites its words)
        tp, tc = torch.from_numpy(prevs).to(gpu_device), torch.from_numpy(curs).to(gpu_device)
        for launch in range(3):
            got = run(aof, eng, p, tp, tc, gpu_device)
            assert np.array_equal(got["hints"], want), (name, launch, [(hex(a), hex(b)) for a, b in zip(got["hints"], want)])
        eng.close()
    assert seen == {0, 1, 2, 3, 4}, seen
