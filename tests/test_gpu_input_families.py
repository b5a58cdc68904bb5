"""Every kernel form the batch plan can choose, on every camera-like input family of synth.py (natural, lowtex, warp,
subpel, vignette, terrace; and a panning, zooming camera sequence), byte for byte against the oracle: records,
half-pixel directions and flow records.  These inputs drive the data-dependent shortcuts (the pruned rows and their early outs,
the start-row vote, the judging first chunk, the column walk's kept window, the refinement's early end, the in-launch
reduction, the 16x16 probe) through branches the box texture never reaches; `terrace` (exactly flat 1-LSB terraces,
stripes at different shifts) with the gate off puts blocks on those shortcuts' bounds: exact ties, best SADs of 0 or
just above, direction sums that tie the integer match.  Each case also asserts that it ran the
kernel its id names.  Large launches are replicas of a few distinct pairs, so that the oracle's share stays small."""
import functools
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAMILIES = ("natural", "lowtex", "warp", "subpel", "vignette", "terrace")
NOISES = (0, 4, 16)
BASE = 3          # distinct pairs per family and launch (VGA)


def noise_for(form, family, forms):
    """The noise of one (form, family) cell: every form sees all three levels over the five families."""
    return NOISES[(forms.index(form) + FAMILIES.index(family)) % len(NOISES)]


@functools.lru_cache(maxsize=None)
def frames(family, W, H, reach, noise, n):
    synth = importlib.import_module("aero_optical_flow_amd.synth")
    prevs = np.empty((n, H, W), np.uint8)
    curs = np.empty_like(prevs)
    for i in range(n):
        kw = dict(alpha=(1.0, 1.5)[i % 2]) if family == "natural" else {}
        if family == "terrace":   # every third pair: one 1-LSB contour on a flat frame (best SADs of a few LSB in a wave of 0s)
            kw = dict(levels=(6, 6, 2)[i % 3])
        prevs[i], curs[i], _ = synth.make_family_pair(family, W, H, reach, 40 + i, noise, **kw)
    return prevs, curs


_REFS = {}


def refs(orc, p, prevs, curs, key, subdirs=False):
    """The oracle's blocks and flows (and directions) of the distinct pairs, memoised by `key`."""
    k = (key, tuple(getattr(p, n) for n, _ in p._fields_), subdirs)
    if k not in _REFS:
        po = orc.params_from(p)
        if subdirs:
            rs = [orc.flow_pair(po, prevs[i], curs[i]) for i in range(prevs.shape[0])]
            _REFS[k] = (np.stack([r["blocks"] for r in rs]), np.stack([r["flow"] for r in rs]),
                        np.stack([r["subdirs"] for r in rs]))
        else:
            b, f, _ = orc.flow_batch(po, prevs, curs, threads=16)
            _REFS[k] = (b, f, None)
    return _REFS[k]


def tiled(torch, arr, reps, device):
    t = torch.from_numpy(arr).to(device)
    return t.repeat((reps,) + (1,) * (t.dim() - 1)).contiguous()


def assert_replicas(aof, blocks, flows, ref, what, sub=None):
    rb, rf, rs = ref
    gb, gf = aof.blocks_view(blocks), aof.flows_view(flows)
    k = rb.shape[0]
    gs = sub.cpu().numpy() if sub is not None else None
    for i in range(gb.shape[0]):
        j = i % k
        assert gb[i].tobytes() == rb[j].tobytes(), (what, i, np.flatnonzero(gb[i] != rb[j])[:8])
        if gs is not None:
            bad = np.flatnonzero(gs[i] != rs[j])
            assert bad.size == 0, (what, i, bad[:8], gs[i][bad[:8]], rs[j][bad[:8]])
        assert gf[i].tobytes() == rf[j].tobytes(), (what, i, gf[i], rf[j])


def run(aof, torch, eng, prevs, curs, reps, device, subpixel=False, workspace=None):
    tp, tc = tiled(torch, prevs, reps, device), tiled(torch, curs, reps, device)
    sub = torch.full((tp.shape[0], eng.nblocks(0)), 0x77, dtype=torch.uint8, device=device) if subpixel else None
    blocks, flows, _ = eng.flow_batch(tp, tc, subdirs=sub, workspace=workspace)
    torch.cuda.synchronize()
    return blocks, flows, sub


def k3_count(aof, torch, eng, call):
    eng.set_profiling(True)
    out = call()
    torch.cuda.synchronize()
    n = len(eng.profile_ms(aof.K_REDUCE))
    eng.set_profiling(False)
    return n, out


# ---- 8x8 tiles, +-4 ------------------------------------------------------------------------------------------------

VGA, NARROW, PX4 = (640, 480), (200, 152), (128, 128)
VGA_CHUNK_PAIRS = 129      # 4 661 blocks per VGA pair: 129 pairs = 2 349 chunks of 256 blocks (kPruneMinChunks 2 048)

FORMS8 = ["exhaustive-vga", "exhaustive-narrow", "exhaustive-px4", "pruned-colwalk-vga", "pruned-colwalk-narrow",
          "pruned-chunkwalk-sparse", "adaptive-judging-vga", "adaptive-belief1-vga", "adaptive-belief0-vga",
          "fused-exhaustive-vga", "fused-colwalk-vga", "half-pixel-vga", "two-level-fused-coarse", "two-level-split",
          "px4-small-path", "px4-grouped", "generic-narrow", "pruned-gate-off-narrow", "half-pixel-gate-off-narrow",
          "two-level-half-pixel-narrow", "pruned-gate-off-vga"]
GATE_OFF = dict(feature_threshold=0, value_threshold=70000)   # every block searched: near-flat blocks, exact ties


def params8(aof, form):
    if "px4" in form:
        return aof.px4flow_params(*PX4), 4
    if form == "pruned-chunkwalk-sparse":     # 19 x 19 blocks, steps 16 / 12: more than 256 blocks, not dense
        return aof.default_params(320, 240, grid_mode=1, num_blocks=20), 4
    if form.startswith("pruned-gate-off"):
        return aof.default_params(*(NARROW if "narrow" in form else VGA), **GATE_OFF), 4
    if form == "half-pixel-gate-off-narrow":
        return aof.default_params(*NARROW, subpixel=1, **GATE_OFF), 4
    if form == "two-level-half-pixel-narrow":
        return aof.default_params(*NARROW, pyramid_levels=2, mean_subtract=1, subpixel=1), 9
    if form.startswith("two-level"):     # (VGA: widths that are a multiple of 16 may take the fused coarse kernel)
        return aof.default_params(*VGA, pyramid_levels=2, mean_subtract=1), 9
    if form.startswith("half-pixel"):
        return aof.default_params(*VGA, subpixel=1), 4
    return aof.default_params(*(NARROW if "narrow" in form else VGA)), 4


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("form", FORMS8)
def test_8x8_form_on_family(aof, orc, gpu_device, form, family):
    noises = [noise_for(form, family, FORMS8)]
    if ("gate-off" in form or family == "terrace") and noises[0]:
        noises.insert(0, 0)                   # (noise-free flat blocks: ties in every row)
    for noise in noises:
        check_8x8_form(aof, orc, gpu_device, form, family, noise)


def check_8x8_form(aof, orc, gpu_device, form, family, noise):
    import torch
    p, reach = params8(aof, form)
    base = 8 if "px4" in form else BASE
    prevs, curs = frames(family, p.width, p.height, reach, noise, base)
    ref = refs(orc, p, prevs, curs, (family, noise, base), subdirs=bool(p.subpixel))
    eng = aof.FlowEngine(p, 0)
    reps = 300 // base + 1 if "px4" in form else 1    # 304 pairs: the grouped search and K3
    if form.startswith("exhaustive") or form.startswith("half-pixel"):
        eng.set_search_mode(aof.SEARCH_EXHAUSTIVE)
    elif form.startswith("pruned"):
        eng.set_search_mode(aof.SEARCH_PRUNED)
    elif form.startswith("adaptive"):
        reps = -(-VGA_CHUNK_PAIRS // base)
        if form == "adaptive-belief1-vga":
            eng.set_search_belief(1)
        elif form == "adaptive-belief0-vga":
            eng.set_search_belief(0)
    elif form == "generic-narrow":
        eng.force_generic(True)
    elif form == "px4-small-path":
        reps = 128 // base                   # 128 pairs: the one-launch path
    assert eng.variant == ("generic" if form == "generic-narrow" else "lane8"), eng.variant
    what = (form, family, noise)
    if form.startswith("fused"):
        eng.set_search_mode(aof.SEARCH_EXHAUSTIVE if form == "fused-exhaustive-vga" else aof.SEARCH_PRUNED)
        n_k3, (b3, f3, _) = k3_count(aof, torch, eng, lambda: run(aof, torch, eng, prevs, curs, 2, gpu_device))
        assert n_k3 == 1, (what, "K3 behind the search")
        assert_replicas(aof, b3, f3, ref, what + ("K3",))
        eng.set_reduce_fusion(True)
        n_k3, (blocks, flows, _) = k3_count(aof, torch, eng, lambda: run(aof, torch, eng, prevs, curs, 2, gpu_device))
        assert n_k3 == 0, (what, "the reduction ran in the search launch")
        assert torch.equal(flows, f3) and torch.equal(blocks, b3), what
        assert_replicas(aof, blocks, flows, ref, what)
        eng.close()
        return
    if form.startswith("half-pixel"):
        for mode in (aof.SEARCH_EXHAUSTIVE, aof.SEARCH_PRUNED):
            eng.set_search_mode(mode)
            blocks, flows, sub = run(aof, torch, eng, prevs, curs, 1, gpu_device, subpixel=True)
            assert_replicas(aof, blocks, flows, ref, what + (mode,), sub)
        eng.close()
        return
    if form == "two-level-split":
        eng.set_split_coarse(True)
    eng.set_profiling(True)
    blocks, flows, sub = run(aof, torch, eng, prevs, curs, reps, gpu_device, subpixel=bool(p.subpixel))
    launches = {k: len(eng.profile_ms(k)) for k in (aof.K_PYRAMID, aof.K_SEARCH_L1, aof.K_SEARCH, aof.K_REDUCE)}
    eng.set_profiling(False)
    assert_replicas(aof, blocks, flows, ref, what, sub)
    if form == "two-level-fused-coarse":      # k_coarse: sums, pyramid, level-1 search and predictor in one launch
        assert launches[aof.K_PYRAMID] == 1 and launches[aof.K_SEARCH_L1] == 0, (what, launches)
    elif form == "two-level-split":           # K1, then the level-1 search and reduction as kernels of their own
        assert launches[aof.K_PYRAMID] == 1 and launches[aof.K_SEARCH_L1] == 1, (what, launches)
    elif "px4" in form:   # k_flow_small (n <= 128) and the grouped search (more pairs) finalise the flows themselves: no K3
        assert launches[aof.K_SEARCH] == 1 and launches[aof.K_REDUCE] == 0, (what, launches)
    st = eng.search_stats()
    if form == "adaptive-judging-vga":
        assert st["pruned_launches"] == 1 and st["exhaustive_launches"] == 0 and st["belief"] == -1, (what, st)
    elif form == "adaptive-belief1-vga":
        assert st["pruned_launches"] == 1 and st["exhaustive_launches"] == 0, (what, st)
    elif form == "adaptive-belief0-vga":
        assert st["pruned_launches"] == 0 and st["exhaustive_launches"] == 1, (what, st)
        tp, tc = tiled(torch, prevs, reps, gpu_device), tiled(torch, curs, reps, gpu_device)
        for _ in range(15):   # the 16th launch looks again with the pruned kernel
            blocks, flows, _ = eng.flow_batch(tp, tc)
        torch.cuda.synchronize()
        assert_replicas(aof, blocks, flows, ref, what + ("probe launch",))
        st = eng.search_stats()
        assert st["pruned_launches"] == 1 and st["exhaustive_launches"] == 15, (what, st)
    elif form in ("exhaustive-vga", "pruned-colwalk-vga"):
        assert st["pruned_launches"] == 0 and st["exhaustive_launches"] == 0, (what, st)   # (fixed modes: no counting)
    eng.close()


@pytest.mark.parametrize("family", ["warp-camera"])
def test_8x8_sequence_view_of_a_panning_zooming_camera(aof, orc, synth, gpu_device, family):
    """pair k = (frame k, frame k + 1) of one buffer: pair_stride is one frame and cur = prev + one frame; one level,
    and two levels with equalisation through the fused coarse kernel and through K1 (which sums and filters each of the
    n + 1 frames once, in one launch, and the level-1 search that views the level-1 frames as a sequence); every
    search mode."""
    import torch
    W, H, n = 640, 480, 8
    frames_, _ = synth.make_camera_sequence(W, H, n + 1, seed=5)
    t = torch.from_numpy(frames_).to(gpu_device)
    for kw, split in ((dict(), False), (dict(pyramid_levels=2, mean_subtract=1), False),
                      (dict(pyramid_levels=2, mean_subtract=1), True)):
        p = aof.default_params(W, H, **kw)
        po = orc.params_from(p)
        rb, rf, _ = orc.flow_batch(po, frames_[:-1], frames_[1:], threads=16)
        for mode in (aof.SEARCH_EXHAUSTIVE, aof.SEARCH_PRUNED, aof.SEARCH_ADAPTIVE):
            eng = aof.FlowEngine(p, 0)
            eng.set_search_mode(mode)
            eng.set_split_coarse(split)
            assert eng.variant == "lane8"
            eng.set_profiling(True)
            blocks, flows, _ = eng.flow_batch(t[:-1], t[1:], n_pairs=n, pair_stride=W * H)
            torch.cuda.synchronize()
            launches = (len(eng.profile_ms(aof.K_PYRAMID)), len(eng.profile_ms(aof.K_SEARCH_L1)))
            eng.set_profiling(False)
            assert_replicas(aof, blocks, flows, (rb, rf, None), (family, kw, split, mode))
            want = (1, 1) if split else ((1, 0) if kw else (0, 0))
            assert launches == want, (family, kw, split, mode, launches)
            eng.close()


# ---- 16x16 tiles, +-8 ----------------------------------------------------------------------------------------------

FORMS16 = ["exhaustive", "pruned", "adaptive-probe", "verdict-rotation"]
KINDS16 = {"one-level": dict(), "half-pixel": dict(subpixel=1), "two-level-eq": dict(pyramid_levels=2, mean_subtract=1),
           "gate-off": dict(feature_threshold=0, value_threshold=70000)}


def run16(aof, orc, torch, device, p, prevs, curs, reps, form, what, ref):
    n = prevs.shape[0] * reps
    eng = aof.FlowEngine(p, 0)
    assert eng.variant == "tile16_lds", eng.variant
    if form == "exhaustive":
        eng.set_search_mode(aof.SEARCH_EXHAUSTIVE)
    elif form == "pruned":
        eng.set_search_mode(aof.SEARCH_PRUNED)
    else:
        assert eng.search_mode == aof.SEARCH_ADAPTIVE
        if form == "verdict-rotation":
            eng.debug_tile16_verdicts([0, 1, 2, 3, 4])
    L = aof.workspace_layout(p, n)
    ws = torch.full((L.total_bytes,), 0x5A, dtype=torch.uint8, device=device)
    blocks, flows, sub = run(aof, torch, eng, prevs, curs, reps, device, subpixel=bool(p.subpixel), workspace=ws)
    assert_replicas(aof, blocks, flows, ref, what, sub)
    if form in ("adaptive-probe", "verdict-rotation"):
        hints = ws[L.hints:L.hints + 4 * n].cpu().numpy().view(np.uint32) & 0xFF
        hist = np.bincount(hints, minlength=5).tolist()
        assert hints.max() <= 4, (what, hist)
        if form == "verdict-rotation":
            assert np.array_equal(hints, np.arange(n) % 5), (what, hist)
        else:
            assert hints.tolist() == hints[:prevs.shape[0]].tolist() * reps, (what, "one verdict per pair", hist)
    eng.close()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", list(KINDS16))
@pytest.mark.parametrize("form", FORMS16)
def test_16x16_form_on_family_320x240(aof, orc, gpu_device, form, kind, family):
    import torch
    kw = dict(value_threshold=12000)
    kw.update(KINDS16[kind])
    p = aof.default_params(320, 240, tile=16, search=8, **kw)
    reach = 17 if kind == "two-level-eq" else 8
    noises = [noise_for(form, family, FORMS16)]
    if ("gate-off" in kind or family == "terrace") and noises[0]:
        noises.insert(0, 0)
    for noise in noises:
        prevs, curs = frames(family, 320, 240, reach, noise, 4)
        ref = refs(orc, p, prevs, curs, (family, noise, 4), subdirs=bool(p.subpixel))
        run16(aof, orc, torch, gpu_device, p, prevs, curs, 5, form, (form, kind, family, noise), ref)


@pytest.mark.parametrize("family", FAMILIES)
def test_16x16_every_form_on_family_1280x960(aof, orc, gpu_device, family):
    import torch
    p = aof.default_params(1280, 960, tile=16, search=8, value_threshold=12000)
    noise = 0 if family == "terrace" else NOISES[FAMILIES.index(family) % len(NOISES)]
    prevs, curs = frames(family, 1280, 960, 8, noise, 2)
    ref = refs(orc, p, prevs, curs, (family, noise, 2))
    for form in FORMS16:
        run16(aof, orc, torch, gpu_device, p, prevs, curs, 3, form, (form, "1280x960", family, noise), ref)
