"""The coarse passes of a pair -- k_coarse, and K1 (k_pyramid_vec / k_pyramid_scalar) with the level-1 search behind it --
at every edge of their launch plans.  Each case of coarse_plan_ref.GPU_CASES is a launch whose sweep or strip plan the
model of tests/coarse_plan_ref.py has worked out and whose paths the census of tests/test_coarse_plan_ref.py counts.
Here it runs, once, with profiling on: the launch counters must name the kernels the model says make the coarse pass
on THIS device (its CU count decides the CU-relative pair counts, the workgroups and the stagger); then every byte that
leaves the pass is compared -- block and flow records of every pair and the level-1 records, level-1 flow record and
predictor in the workspace against the oracle, the four pixel sums per pair against numpy sums as exact integers, on
split launches the workspace's level-1 frames against the oracle's pyramid, and fused against split wherever both exist.
Launches of more pairs than a case has distinct ones replicate them so that consecutive pairs of a workgroup differ in
pixel sums, delta, gated blocks and level-1 records (asserted on the oracle's records before the device runs): a stale
histogram, key array or LDS row shows in the bytes.  Outputs and workspace are filled with a sentinel before the
launch.  No tolerance anywhere."""
import numpy as np
import pytest

import coarse_plan_ref as ref
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
KERNELS = ("K_PYRAMID", "K_SEARCH_L1", "K_REDUCE_L1", "K_SEARCH")
_oracle = {}


def device_cus(gpu_device):
    import torch
    return int(torch.cuda.get_device_properties(gpu_device).multi_processor_count)


def oracle_for(aof, orc, synth, c, cus):
    """The frames of the case's distinct pairs (a sequence: of its consecutive frames) and the oracle's answers, computed
    once per case and left unchanged: blocks [k, nb0] u32, flows [k, 16], level-1 blocks [k, nb1] u32, level-1 flow
    records with the predictor [k, 16], pixel sums [k, 4], level-1 frames."""
    key = (c["id"], cus)
    if key in _oracle:
        return _oracle[key]
    p = aof.default_params(c["w"], c["h"], **ref.params_kw(c))
    po = orc.params_from(p)
    two = c["levels"] == 2
    if c["sequence"]:
        frames = ref.sequence_frames(c, synth)
        prevs, curs = frames[:-1], frames[1:]
    else:
        prevs, curs, _ = ref.distinct_frames(c, synth, cus)
        frames = None
    blocks, flows, b1s, f1s = [], [], [], []
    for a, b in zip(prevs, curs):
        out = orc.flow_pair(po, a, b, want_l1=two)
        blocks.append(np.ascontiguousarray(out["blocks"]).view(np.uint32).ravel())
        flows.append(np.frombuffer(out["flow"].tobytes(), dtype=np.uint8))
        if two:
            b1 = out["blocks_l1"]
            f1, px, py = orc.reduce(po, b1, out["subdirs_l1"] if c["subpixel"] else None, c["search"])
            rec = np.zeros(1, dtype=orc.FLOW_DTYPE)
            rec[0] = f1
            rec["pred_x"], rec["pred_y"] = px, py      # (the level-1 record carries the predictor it emits)
            f1 = rec
            assert (int(out["flow"]["pred_x"]), int(out["flow"]["pred_y"])) == (px, py)
            b1s.append(np.ascontiguousarray(b1).view(np.uint32).ravel())
            f1s.append(np.frombuffer(f1.tobytes(), dtype=np.uint8))
    down = lambda x: orc.pyramid_down(x[: c["h"] // 2 * 2, : c["w"] // 2 * 2])   # (odd sizes: the last column / row has no level-1 pixel)
    l1p, l1c = [down(a) for a in prevs], [down(b) for b in curs]
    total = lambda x: int(x.sum(dtype=np.uint64))
    sums = np.array([[total(a), total(a1), total(b), total(b1)] for a, a1, b, b1 in zip(prevs, l1p, curs, l1c)], dtype=np.uint64)
    assert int(sums.max()) < 2 ** 32
    want = dict(prevs=prevs, curs=curs, frames=frames, blocks=np.stack(blocks), flows=np.stack(flows), sums=sums.astype(np.uint32),
                b1=np.stack(b1s) if two else None, f1=np.stack(f1s) if two else None, l1p=np.stack(l1p), l1c=np.stack(l1c))
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _oracle[key] = (p, want)
    return _oracle[key]


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
    counts = {k: len(eng.profile_ms(getattr(aof, k))) for k in KERNELS}
    eng.set_profiling(False)
    w1, h1 = c["w"] // 2, c["h"] // 2
    host = ws.cpu().numpy()
    got = dict(counts=counts, blocks=blocks.cpu().numpy().view(np.uint32), flows=flows.cpu().numpy(),
               sums=host[L.sums:L.sums + 16 * n].view(np.uint32).reshape(n, 4) if c["mean_subtract"] else None)
    if c["levels"] == 2:
        nb1 = eng.nblocks(1)
        frames = n + 1 if c["sequence"] else n
        got.update(b1=host[L.l1_blocks:L.l1_blocks + 4 * n * nb1].view(np.uint32).reshape(n, nb1),
                   f1=host[L.l1_flows:L.l1_flows + 16 * n].reshape(n, 16),
                   l1p=host[L.l1_prev:L.l1_prev + frames * w1 * h1].reshape(frames, h1, w1),
                   l1c=None if c["sequence"] else host[L.l1_cur:L.l1_cur + n * w1 * h1].reshape(n, h1, w1))
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


@pytest.mark.parametrize("c", ref.GPU_CASES, ids=lambda c: c["id"])
def test_the_coarse_pass_of_every_pair_equals_the_oracle(aof, orc, synth, gpu_device, c):
    import torch
    cus = device_cus(gpu_device)
    n = ref.n_pairs_of(c, cus)
    assert n >= 1 and ref.device_bytes(c, cus) <= 125 * 10 ** 6
    kind, want_counts = ref.coarse_kind(c, cus), ref.counters(c, cus)
    assert kind == ref.coarse_kind(c), "the case takes the kernel the census counted it for on this device too"
    p, want = oracle_for(aof, orc, synth, c, cus)
    k = want["prevs"].shape[0]
    two = c["levels"] == 2
    wgs = min(n, cus)
    idx = np.arange(n) if c["sequence"] else ref.pair_contents(n, k, wgs)
    if c["distinct"] == 50:
        # consecutive pairs of a workgroup differ in sums, delta, gated blocks and level-1 records; where most workgroups
        # walk two pairs or more, a gated pair follows a voted one, a voted one a gated one, a delta of 0 one that is not
        assert kind == "fused" and k == 50 and ref.case_coarse_plan(c, cus)["wgs"] == wgs
        facts = ref.oracle_facts(aof, orc, synth, c, cus)
        ref.check_chains(facts, idx, wgs, orderings=n >= wgs + k)
    if c["edge"]:
        ref.check_edge_moves_delta(c, want["prevs"], want["curs"])
    stride, prev_at, cur_at = ref.frame_layout(c)
    if c["sequence"]:
        frames = placed(torch, gpu_device, torch.from_numpy(want["frames"].copy()).to(gpu_device), n + 1, stride, 0)
        prev, cur = frames[:n], frames[1:]
        assert cur.data_ptr() - prev.data_ptr() == stride == c["w"] * c["h"]
    else:
        at = torch.from_numpy(idx).to(gpu_device)
        prev = placed(torch, gpu_device, torch.from_numpy(want["prevs"].copy()).to(gpu_device)[at], n, stride, c["prev_off"])
        cur = placed(torch, gpu_device, torch.from_numpy(want["curs"].copy()).to(gpu_device)[at], n, stride, c["cur_off"])
    assert prev.data_ptr() % 16 == prev_at % 16 and cur.data_ptr() % 16 == cur_at % 16 and prev.stride(0) == stride

    got = launch(aof, torch, c, p, prev, cur, n, c["split"], gpu_device)
    # which kernels made the coarse pass, before any byte is compared
    assert got["counts"] == dict(want_counts, K_SEARCH=1), (c["id"], kind, got["counts"], want_counts)
    what = f"{c['id']} ({kind}, {n} pairs, {cus} CUs)"
    same(got["blocks"], want["blocks"], idx, what + " block records")
    same(got["flows"], want["flows"], idx, what + " flow records")
    if kind == "small":
        return
    same(got["sums"], want["sums"], idx, what + " pixel sums")
    if c["sequence"]:   # the first and the last frame reach one record each, every frame between them two
        assert got["sums"][0, :2].tolist() == want["sums"][0, :2].tolist() and got["sums"][n - 1, 2:].tolist() == want["sums"][n - 1, 2:].tolist()
    if two:
        same(got["b1"], want["b1"], idx, what + " level-1 block records")
        same(got["f1"], want["f1"], idx, what + " level-1 flow record and predictor")
    if two and kind == "k1":
        if c["sequence"]:
            same(got["l1p"], np.concatenate([want["l1p"], want["l1c"][-1:]]), np.arange(n + 1), what + " level-1 frames")
        else:
            same(got["l1p"], want["l1p"], idx, what + " level-1 prev frames")
            same(got["l1c"], want["l1c"], idx, what + " level-1 cur frames")
    if kind == "fused":
        # the level-1 frames never leave LDS; and the split kernels give the same bytes
        assert (got["l1p"] == SENTINEL).all() and (got["l1c"] == SENTINEL).all(), "k_coarse wrote level-1 frames to the workspace"
        other = launch(aof, torch, c, p, prev, cur, n, True, gpu_device)
        assert other["counts"]["K_PYRAMID"] == 1 and other["counts"]["K_SEARCH_L1"] == 1, other["counts"]
        for name in ("blocks", "flows", "sums", "b1", "f1"):
            same(got[name], other[name], np.arange(n), what + f" fused against split: {name}")
    del prev, cur
    torch.cuda.empty_cache()
