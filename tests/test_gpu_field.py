"""The motion-field kernel on the device (csrc/k_field.hip behind aof_field_batch_device) against the numpy model
(tests/field_ref.py), byte for byte: designed records uploaded for every geometry of field_ref.GEOMETRIES -- below a wave, one
wave exactly, the wave / workgroup switch, odd grids whose pairs start at every alignment, grids beyond 8 192 blocks --,
1, 3, 5 and 67 pairs, with and without sub-directions, one and two passes, blocks at reach kept and left out; determinants
beyond 2^53 on the largest grids; flow_batch + field_batch end to end on zooming and rotating pairs, eagerly and from one
captured graph; and the refusals.  Inputs and outputs sit in one arena between guard zones filled with a sentinel: after every
launch everything but the field records must be as it was."""
import ctypes as C
import importlib

import numpy as np
import pytest

import field_ref as fr
from plan_rig import GUARD, SENTINEL, time_limit   # noqa: F401  (time_limit: this module's fixture too, every test under a limit of its own)

pytestmark = pytest.mark.gpu


class Arena:
    """blocks, subdirs, flows and fields of n pairs between guard zones of one allocation; the records start `skew` bytes
    (a multiple of 4) behind a 256-byte boundary, so that pair 0 can sit at any alignment a caller may choose."""

    def __init__(self, torch, device, n, nb, skew=0):
        sizes = dict(blocks=4 * n * nb, subdirs=n * nb, flows=16 * n, fields=64 * n)
        self.at, off = {}, GUARD
        for k, v in sizes.items():
            lo = off + (skew if k == "blocks" else 0)
            self.at[k] = (lo, lo + v)
            off = (lo + v + 255) // 256 * 256 + GUARD
        self.mem = torch.empty((off,), dtype=torch.uint8, device=device)
        self.n, self.nb = n, nb
        assert self.mem.data_ptr() % 256 == 0

    def view(self, k):
        return self.mem[self.at[k][0]:self.at[k][1]]

    def upload(self, torch, blocks, subdirs, flows):
        self.mem.fill_(SENTINEL)
        for k, a in (("blocks", blocks), ("subdirs", subdirs), ("flows", flows)):
            self.view(k).copy_(torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()))
        self.before = self.mem.cpu().numpy()

    def tensors(self, torch):
        return (self.view("blocks").view(torch.int32).view(self.n, self.nb), self.view("subdirs").view(self.n, self.nb),
                self.view("flows").view(self.n, 16), self.view("fields").view(self.n, 64))

    def fields_and_rest_untouched(self):
        """The field records; everything else -- inputs and guard zones -- must hold what it held before the launch."""
        after = self.mem.cpu().numpy()
        lo, hi = self.at["fields"]
        moved = np.flatnonzero(np.concatenate([after[:lo] != self.before[:lo], after[hi:] != self.before[hi:]]))
        assert moved.size == 0, ("bytes outside the field records written", moved[:8])
        got = after[lo:hi].copy()
        self.mem[lo:hi].fill_(SENTINEL)
        return got.view(fr.FIELD_DTYPE)


ROTATION = {1: 2, 3: 3, 5: 0, 67: 0}       # where a batch's cycle through the designs starts: 1, 3 and 5 pairs see all six between them


def designs_from(start):
    names = list(fr.DESIGNS)
    return names[start:] + names[:start]


@pytest.mark.parametrize("geom", fr.GEOMETRIES, ids=[g[0] for g in fr.GEOMETRIES])
def test_kernel_equals_model_on_designed_records(aof, gpu_device, geom):
    import torch
    p = fr.make_params(aof, geom)
    eng = aof.FlowEngine(p, 0)
    nb = eng.nblocks(0)
    assert nb == fr.NBLOCKS[geom[0]]
    seen = set()
    for n in (1, 3, 5) + ((67,) if nb <= 272 else ()):
        blocks, subdirs, flows = fr.batch(p, n, seed=n, designs=designs_from(ROTATION[n]))
        arena = Arena(torch, gpu_device, n, nb, skew=4 * (n % 4))
        arena.upload(torch, blocks, subdirs, flows)
        tb, ts, tf, tfld = arena.tensors(torch)
        for sub in (subdirs, None):
            for passes in (1, 2):
                for exclude in (0, 1):
                    kw = dict(passes=passes, exclude_reach=exclude)
                    eng.field_batch(tb, tf, subdirs=ts if sub is not None else None, fields=tfld, params=aof.field_params(**kw))
                    torch.cuda.synchronize()
                    got = arena.fields_and_rest_untouched()
                    want = fr.model_batch(p, blocks, sub, flows, fr.fparams(**kw))
                    assert got.tobytes() == want.tobytes(), (n, sub is None, kw, [(i, got[i], want[i]) for i in range(n) if got[i] != want[i]][:2])
                    seen |= {int(f) for f in want["flags"]}
    assert seen == {0, fr.VALID, fr.VALID | fr.REFIT}, seen
    eng.close()


@pytest.mark.parametrize("geom", [fr.LARGEST, fr.LARGEST_ODD], ids=lambda g: g[0])
def test_determinants_beyond_2_to_53_on_the_largest_grids(aof, gpu_device, geom):
    """int64 -> double on the device rounds to nearest, as the host's conversion does: D and Na beyond 2^53, exactly
    representable on the dense grid (multiples of 256), in need of rounding on the sparse one."""
    import torch
    p = fr.make_params(aof, geom)
    assert aof.check_params(p) == 0 and aof.field_supported(p)
    eng = aof.FlowEngine(p, 0)
    nb = eng.nblocks(0)
    blocks, subdirs, flows = fr.batch(p, 2, seed=3, designs=("extreme", "similarity"))
    arena = Arena(torch, gpu_device, 2, nb, skew=8)
    arena.upload(torch, blocks, subdirs, flows)
    tb, ts, tf, tfld = arena.tensors(torch)
    for kw in (dict(exclude_reach=0), dict(exclude_reach=0, passes=1)):
        eng.field_batch(tb, tf, subdirs=ts, fields=tfld, params=aof.field_params(**kw))
        torch.cuda.synchronize()
        got = arena.fields_and_rest_untouched()
        want = fr.model_batch(p, blocks, subdirs, flows, fr.fparams(**kw))
        assert got.tobytes() == want.tobytes(), (kw, got, want)
    assert (np.abs(got["det"]) > 2 ** 53).all() and abs(int(got["num_zoom"][0])) > 2 ** 53
    if geom is fr.LARGEST_ODD:
        assert float(int(got["det"][0])) != int(got["det"][0]) and float(int(got["num_zoom"][0])) != int(got["num_zoom"][0])
    eng.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------
E2E = {
    "dense128": dict(size=(128, 128), kw={}),
    "dense128-two-levels-half-pixel": dict(size=(128, 128), kw=dict(pyramid_levels=2, mean_subtract=1, subpixel=1)),
    "c5": dict(size=(1280, 960), kw=dict(tile=16, search=8, value_threshold=12000)),
}


def warp_pairs(synth, p, first):
    presets = sorted(synth.WARP_PRESETS)
    pairs = [synth.make_warp_pair(p.width, p.height, reach=2, pair_index=first + k, noise=4 * k, preset=presets[(first + k) % 5]) for k in range(2)]
    return np.stack([q[0] for q in pairs]), np.stack([q[1] for q in pairs])


def model_on_oracle(orc, p, prevs, curs):
    refs = [orc.flow_pair(orc.params_from(p), a, b) for a, b in zip(prevs, curs)]
    want = np.array([fr.model(p, r["blocks"], r["subdirs"] if p.subpixel else None, r["flow"]) for r in refs], fr.FIELD_DTYPE)
    return refs, want


@pytest.mark.parametrize("name", list(E2E))
def test_flow_batch_then_field_batch_on_warped_pairs(aof, orc, synth, gpu_device, name):
    import torch
    p = aof.default_params(*E2E[name]["size"], **E2E[name]["kw"])
    eng = aof.FlowEngine(p, 0)
    prevs, curs = warp_pairs(synth, p, 2)
    sub = torch.empty((2, eng.nblocks(0)), dtype=torch.uint8, device=gpu_device) if p.subpixel else None
    blocks, flows, _ = eng.flow_batch(torch.from_numpy(prevs).to(gpu_device), torch.from_numpy(curs).to(gpu_device), subdirs=sub)
    fields = aof.fields_view(eng.field_batch(blocks, flows, subdirs=sub))
    torch.cuda.synchronize()
    refs, want = model_on_oracle(orc, p, prevs, curs)
    gf = aof.flows_view(flows)
    for i in range(2):
        assert gf[i].tobytes() == refs[i]["flow"].tobytes()
        assert fields[i].tobytes() == want[i].tobytes(), (i, fields[i], want[i])
        assert fields[i]["accepted"] == gf[i]["count"] and fields[i]["flags"] & fr.VALID
    eng.close()


def test_one_captured_graph_of_flow_and_field_replays_on_new_frames(aof, orc, synth, gpu_device):
    import torch
    p = aof.default_params(128, 128, pyramid_levels=2, mean_subtract=1, subpixel=1)
    eng = aof.FlowEngine(p, 0)
    nb = eng.nblocks(0)
    prev = torch.zeros((2, 128, 128), dtype=torch.uint8, device=gpu_device)
    cur = torch.zeros_like(prev)
    blocks = torch.zeros((2, nb), dtype=torch.int32, device=gpu_device)
    sub = torch.zeros((2, nb), dtype=torch.uint8, device=gpu_device)
    flows = torch.zeros((2, 16), dtype=torch.uint8, device=gpu_device)
    fields = torch.zeros((2, 64), dtype=torch.uint8, device=gpu_device)
    ws = torch.zeros(aof.workspace_layout(p, 2).total_bytes, dtype=torch.uint8, device=gpu_device)
    fp = aof.field_params()

    def step():
        eng.flow_batch(prev, cur, blocks=blocks, subdirs=sub, flows=flows, workspace=ws)
        eng.field_batch(blocks, flows, subdirs=sub, fields=fields, params=fp)

    step()   # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for rep in range(2):
        prevs, curs = warp_pairs(synth, p, 10 + 2 * rep)
        prev.copy_(torch.from_numpy(prevs))
        cur.copy_(torch.from_numpy(curs))
        fields.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        _, want = model_on_oracle(orc, p, prevs, curs)
        assert aof.fields_view(fields).tobytes() == want.tobytes(), (rep, aof.fields_view(fields), want)
    eng.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(aof, gpu_device):
    import torch
    p = aof.default_params(64, 64)
    eng = aof.FlowEngine(p, 0)
    blocks, subdirs, flows = fr.batch(p, 2, seed=9)
    arena = Arena(torch, gpu_device, 2, 49)
    arena.upload(torch, blocks, subdirs, flows)
    tb, ts, tf, tfld = arena.tensors(torch)
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    ok = aof.field_params()
    good = [eng._ctx, C.byref(ok), tb.data_ptr(), ts.data_ptr(), tf.data_ptr(), 2, tfld.data_ptr(), stream]
    call = lambda a: aof.lib.aof_field_batch_device(*a)
    bad = []
    for i in (0, 1, 2, 4, 6):                                                  # NULL ctx, params, blocks, flows, fields
        a = list(good)
        a[i] = None
        bad.append(a)
    for kw in (dict(min_blocks=2), dict(passes=3), dict(passes=0), dict(exclude_reach=2), dict(gate_px=0.0), dict(gate_px=float("nan")),
               dict(gate_px=float("inf"))):
        bad.append(good[:1] + [C.byref(aof.field_params(**kw))] + good[2:])
    bad.append(good[:2] + [tb.data_ptr() + 2] + good[3:])                     # records not 4-byte aligned
    bad.append(good[:6] + [tfld.data_ptr() + 4] + good[7:])                   # field records not 8-byte aligned
    bad.append(good[:5] + [-1] + good[6:])
    bad.append(good[:5] + [2 ** 31] + good[6:])
    for a in bad:
        assert call(a) == -22, a
    wide = aof.FlowEngine(aof.default_params(8192, 2048), 0)                   # a grid beyond the fit's integer range
    assert not aof.field_supported(wide.params) and call([wide._ctx] + good[1:]) == -22
    assert b"aof_field_supported" in aof.lib.aof_last_error(wide._ctx)
    wide.close()
    torch.cuda.synchronize()
    untouched = arena.fields_and_rest_untouched()
    assert (untouched.view(np.uint8) == SENTINEL).all()
    assert call(good[:5] + [0] + good[6:]) == 0                                # no pairs: nothing to do, nothing written
    torch.cuda.synchronize()
    assert (arena.fields_and_rest_untouched().view(np.uint8) == SENTINEL).all()
    assert call(good) == 0
    torch.cuda.synchronize()
    assert arena.fields_and_rest_untouched().tobytes() == fr.model_batch(p, blocks, subdirs, flows).tobytes()
    eng.close()
