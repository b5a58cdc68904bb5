"""The small-pair kernels -- the one-workgroup class that runs flow_small_pair (k_flow_small, its tagged and resident forms)
and the grouped search k_flow_lane8 -- at every edge of their launch plans.  Each case of small_plan_ref.GPU_CASES is a
shape whose plan the model of tests/small_plan_ref.py has worked out and whose paths the census of
tests/test_small_plan_ref.py counts.  Here it runs, once: eight distinct pairs of a compact hard set (corners of the reach,
a flat, an identical and an unrelated pair, period-2 textures, brightness steps that saturate the equalised frame both
ways, a block row gated; two levels: shifts that push edge windows out of the frame), each asserted on the oracle's
records to do what it is there for before the device runs.  Then
  - one launch of the one-workgroup kernel (or the fallback the model names) with profiling on into sentinel-filled
    outputs: the launch counters must be the model's before any byte is compared; block records, half-pixel directions
    and flow records of every pair, with two levels the level-1 records, directions, flow record and predictor in the
    workspace, with mean_subtract the pixel sums as exact integers; the workspace's level-1 frames still the sentinel;
  - the same content through the separate kernels (set_split_coarse) at the pair counts the grouped plan names -- ppw - 1,
    ppw, ppw + 1, k ppw + 1, and 129 without the switch -- with counters that name the grouped searches and no K3, against
    the oracle and against the first launch;
  - frames at the offsets and strides the case names;
  - for the cases tagged so, the per-call forms: flow_pair_host, then five frames through stream_push without and with
    the resident kernel.
No tolerance anywhere."""
import numpy as np
import pytest

import small_plan_ref as ref
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
KERNELS = ("K_PYRAMID", "K_SEARCH_L1", "K_REDUCE_L1", "K_SEARCH", "K_REDUCE")
_oracle = {}


def oracle_for(aof, orc, synth, c):
    """The case's parameters, its eight distinct pairs and the oracle's answers, computed once per case and left unchanged:
    blocks [8, nb0] u32, subdirs [8, nb0], flows [8, 16], level-1 blocks / subdirs / flow records with the predictor, pixel
    sums [8, 4] (prev, level-1 prev, cur, level-1 cur)."""
    if c["id"] in _oracle:
        return _oracle[c["id"]]
    frames = ref.hard_pairs(c, synth)
    prevs, curs, kinds = frames
    p = ref.case_params(c, aof, orc, synth, frames)
    po = orc.params_from(p)
    two = c["levels"] == 2
    outs = [orc.flow_pair(po, a, b, want_l1=True) for a, b in zip(prevs, curs)]
    ref.check_inputs(c, p, prevs, curs, kinds, outs)       # before the device runs
    f1s = []
    for o in outs:
        if two:
            f1, px, py = orc.reduce(po, o["blocks_l1"], o["subdirs_l1"] if c["subpixel"] else None, 4)
            rec = np.zeros(1, dtype=orc.FLOW_DTYPE)
            rec[0] = f1
            rec["pred_x"], rec["pred_y"] = px, py          # (the level-1 record carries the predictor it emits)
            assert (int(o["flow"]["pred_x"]), int(o["flow"]["pred_y"])) == (px, py)
            f1s.append(np.frombuffer(rec.tobytes(), dtype=np.uint8))
    total = lambda x: int(x.sum(dtype=np.uint64))
    sums = np.array([[total(a), total(orc.pyramid_down(a)) if two else 0, total(b), total(orc.pyramid_down(b)) if two else 0]
                     for a, b in zip(prevs, curs)], dtype=np.uint64)
    assert int(sums.max()) < 2 ** 32
    u32 = lambda key: np.stack([np.ascontiguousarray(o[key]).view(np.uint32).ravel() for o in outs])
    want = dict(prevs=prevs, curs=curs, outs=outs, blocks=u32("blocks"), subdirs=np.stack([o["subdirs"] for o in outs]),
                flows=np.stack([np.frombuffer(o["flow"].tobytes(), dtype=np.uint8) for o in outs]), sums=sums.astype(np.uint32),
                b1=u32("blocks_l1") if two else None, s1=np.stack([o["subdirs_l1"] for o in outs]) if two else None,
                f1=np.stack(f1s) if two else None)
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _oracle[c["id"]] = (p, po, want)
    return _oracle[c["id"]]


def placed(torch, device, src, n, stride, off):
    """src [n, h, w] in a buffer of its own: pair i at byte off + i * stride behind a 256-byte boundary."""
    h, w = src.shape[1:]
    buf = torch.full((off + n * stride + 256,), SENTINEL, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 256 == 0
    view = torch.as_strided(buf, (n, h, w), (stride, w, 1), off)
    view.copy_(src)
    return view


def launch(aof, torch, c, p, prev, cur, n, split, device):
    """One launch with profiling on into sentinel-filled outputs: the launch counters and everything that left."""
    eng = aof.FlowEngine(p, 0)
    if split:
        eng.set_split_coarse(True)
    nb0 = eng.nblocks(0)
    L = aof.workspace_layout(p, n)
    fill = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.uint8, device=device)
    blocks, flows, ws = fill(n, nb0 * 4), fill(n, 16), fill(L.total_bytes)
    sub = fill(n, nb0) if c["subpixel"] else None
    eng.set_profiling(True)
    eng.flow_batch(prev, cur, blocks=blocks.view(torch.int32), flows=flows, subdirs=sub, workspace=ws)
    torch.cuda.synchronize()
    counts = [len(eng.profile_ms(getattr(aof, k))) for k in KERNELS]
    eng.set_profiling(False)
    host = ws.cpu().numpy()
    got = dict(counts=counts, blocks=blocks.cpu().numpy().view(np.uint32), flows=flows.cpu().numpy(),
               subdirs=sub.cpu().numpy() if c["subpixel"] else None,
               sums=host[L.sums:L.sums + 16 * n].view(np.uint32).reshape(n, 4) if c["mean_subtract"] else None)
    if c["levels"] == 2:
        nb1, w1, h1 = eng.nblocks(1), c["w"] // 2, c["h"] // 2
        got.update(b1=host[L.l1_blocks:L.l1_blocks + 4 * n * nb1].view(np.uint32).reshape(n, nb1),
                   s1=host[L.l1_subdirs:L.l1_subdirs + n * nb1].reshape(n, nb1) if c["subpixel"] else None,
                   f1=host[L.l1_flows:L.l1_flows + 16 * n].reshape(n, 16),
                   l1=np.concatenate([host[L.l1_prev:L.l1_prev + n * w1 * h1], host[L.l1_cur:L.l1_cur + n * w1 * h1]]))
    eng.close()
    return got


def same(got, want, idx, what):
    """got [n, ...] == want[idx] byte for byte; the first pair that differs is reported."""
    exp = want[idx]
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.flatnonzero((got != exp).reshape(got.shape[0], -1).any(axis=1))
    if bad.size:
        i = int(bad[0])
        where = np.flatnonzero(got[i].ravel() != exp[i].ravel())
        pytest.fail(f"{what}: {bad.size} of {got.shape[0]} pairs differ; pairs {bad[:6].tolist()} .. {bad[-3:].tolist()}; pair {i} "
                    f"(content {int(idx[i])}) at {where[:8].tolist()}: {got[i].ravel()[where[:8]].tolist()} for "
                    f"{exp[i].ravel()[where[:8]].tolist()}")


def against_the_oracle(c, got, want, idx, what):
    two = c["levels"] == 2
    same(got["blocks"], want["blocks"], idx, what + " block records")
    if c["subpixel"]:
        same(got["subdirs"], want["subdirs"], idx, what + " half-pixel directions")
    same(got["flows"], want["flows"], idx, what + " flow records")
    if two:
        same(got["b1"], want["b1"], idx, what + " level-1 block records")
        if c["subpixel"]:
            same(got["s1"], want["s1"], idx, what + " level-1 half-pixel directions")
        same(got["f1"], want["f1"], idx, what + " level-1 flow record and predictor")
    if c["mean_subtract"]:      # (one level: the level-1 columns are not part of the result)
        cols = [0, 1, 2, 3] if two else [0, 2]
        same(np.ascontiguousarray(got["sums"][:, cols]), np.ascontiguousarray(want["sums"][:, cols]), idx, what + " pixel sums")


def per_call_forms(aof, orc, c, p, po, want):
    """flow_pair_host once, then five consecutive frames through stream_push: launch per call, then the resident kernel."""
    eng = aof.FlowEngine(p, 0)
    blocks, subdirs, flow = eng.flow_pair_host(want["prevs"][2], want["curs"][2])
    o = want["outs"][2]
    assert blocks.tobytes() == o["blocks"].tobytes(), "flow_pair_host: block records"
    if c["subpixel"]:
        assert subdirs.tobytes() == o["subdirs"].tobytes(), "flow_pair_host: half-pixel directions"
    assert flow.tobytes() == o["flow"].tobytes(), "flow_pair_host: flow record"
    frames = [want["prevs"][0], want["curs"][0], want["curs"][2], want["prevs"][3], want["prevs"][6]]
    records = [orc.flow_pair(po, a, b)["flow"].tobytes() for a, b in zip(frames[:-1], frames[1:])]
    assert len(set(records)) == len(records)
    for resident in (False, True):
        eng.stream_reset()
        eng.set_stream_resident(resident)
        assert eng.stream_push(frames[0]) is None
        for k in range(1, 5):
            got = eng.stream_push(frames[k])
            assert got is not None and got.tobytes() == records[k - 1], (c["id"], "resident" if resident else "launch per call", k, got)
    st = eng.stream_stats()
    # the four pushes behind the first frame: all served by the resident kernel, the first fetching both frames, the others
    # one buffer each, 1 and 0 in turn.  (Frames beyond 64 KB are copied to the device: no resident kernel for them.)
    served = 4 if ref.resident_serves(c) else 0
    assert st["resident_fallbacks"] == 0 and st["resident_lost"] == 0 and st["resident_served"] == served and st["calls"] == 8, st
    eng.close()


@pytest.mark.parametrize("c", ref.GPU_CASES, ids=lambda c: c["id"])
def test_the_small_pair_kernels_equal_the_oracle(aof, orc, synth, gpu_device, c):
    import torch
    p, po, want = oracle_for(aof, orc, synth, c)
    n, two = c["n_pairs"], c["levels"] == 2
    kind = ref.kind(c)
    stride, prev_at, cur_at = ref.frame_layout(c)
    dev_prevs, dev_curs = (torch.from_numpy(want[k].copy()).to(gpu_device) for k in ("prevs", "curs"))

    def frames_of(count):
        idx = np.arange(count) % 8
        at = torch.from_numpy(idx).to(gpu_device)
        prev = placed(torch, gpu_device, dev_prevs[at], count, stride, c["prev_off"])
        cur = placed(torch, gpu_device, dev_curs[at], count, stride, c["cur_off"])
        assert prev.data_ptr() % 16 == prev_at % 16 and cur.data_ptr() % 16 == cur_at % 16 and prev.stride(0) == stride
        return idx, prev, cur

    # ---- the one launch (or the fallback the model names)
    idx, prev, cur = frames_of(n)
    first = launch(aof, torch, c, p, prev, cur, n, False, gpu_device)
    assert first["counts"] == ref.counters(c), (c["id"], kind, first["counts"], ref.counters(c))
    what = f"{c['id']} ({kind}, {n} pairs)"
    against_the_oracle(c, first, want, idx, what)
    if two and first["counts"][1] == 0:      # level 1 never left the chip
        assert (first["l1"] == SENTINEL).all(), "level-1 frames were written to the workspace"

    # ---- the grouped search on the same content
    counts = dict(ref.group_counts(c))
    runs = [(name, m, True) for name, m in counts.items()] + ([("over-128", 129, False)] if c["over_128"] else [])
    for name, m, split in runs:
        plan = ref.case_group_plan(c, m)
        assert plan["ppw"] > 0 and ref.kind(c, m, split) == "separate"
        idx_m, prev_m, cur_m = frames_of(m)
        got = launch(aof, torch, c, p, prev_m, cur_m, m, split, gpu_device)
        wanted = ref.counters(c, m, split)
        assert wanted[3:] == [1, 0] and got["counts"] == wanted, (c["id"], name, m, got["counts"], wanted)
        what_m = f"{c['id']} (grouped, {name}: {m} pairs, {plan['wgs']} workgroups of {plan['ppw']} pairs)"
        against_the_oracle(c, got, want, idx_m, what_m)
        if kind == "small":                   # and against the one-workgroup kernel's bytes
            shared = np.flatnonzero(idx_m < n)
            for key in ("blocks", "flows") + (("subdirs",) if c["subpixel"] else ()) + (("b1", "f1") if two else ()):
                same(np.ascontiguousarray(got[key][shared]), first[key], idx_m[shared], what_m + f" against the one launch: {key}")
        del prev_m, cur_m

    # ---- the per-call forms
    if c["percall"]:
        assert kind == "small"
        per_call_forms(aof, orc, c, p, po, want)
    del prev, cur
    torch.cuda.empty_cache()
